// Stand-alone run of tilingnn_amd/csrc/union_components.h -- the two per-tile steps the union kernels share -- on the host.  No
// device, no HIP header:
//   g++ -std=c++17 -O1 -fsanitize=address,undefined -I tilingnn_amd/csrc tests/host/union_components_test.cpp
// (tests/test_union_topology_host.py writes the file, builds and runs this, and compares with its own union-find).
//
// File: that of union_topology_point_test.cpp.  Per mask the program labels the components by sweeping lower_label over the
// tiles in index order until a sweep stores nothing, and prints "<components> <sweeps>" (the last, idle sweep counted); then
// "err <word>".  After that it runs `collides` over the rows of a small collision CSR of its own with entries out of range,
// whole rows and every second entry, and prints "collides <row> <first> <stride> <answer> <err>" per call.
#include <stdio.h>
#include <stdlib.h>

#include <vector>

#include "union_components.h"

using namespace tgnn::topo;

template <class T>
static std::vector<T> read_array(FILE *f, size_t count) {
    std::vector<T> v(count);
    if (count && fread(v.data(), sizeof(T), count, f) != count) {
        fprintf(stderr, "short file\n");
        exit(2);
    }
    return v;
}

int main(int argc, char **argv) {
    if (argc != 2) return 2;
    FILE *f = fopen(argv[1], "rb");
    if (!f) return 2;
    const std::vector<int64_t> head = read_array<int64_t>(f, 4);
    const std::vector<double> par = read_array<double>(f, 3);
    const int64_t n = head[0], n_pts = head[1], n_touch = head[2], n_masks = head[3];
    const std::vector<double> ring_xy = read_array<double>(f, 2 * (size_t)n_pts);
    const std::vector<int32_t> ring_ptr = read_array<int32_t>(f, (size_t)n + 1), touch_ptr = read_array<int32_t>(f, (size_t)n + 1);
    const std::vector<int32_t> touch_idx = read_array<int32_t>(f, (size_t)n_touch);
    const std::vector<int32_t> alive = read_array<int32_t>(f, (size_t)n_masks * (size_t)n);
    fclose(f);
    const Tiles g{reinterpret_cast<const Pt *>(ring_xy.data()), ring_ptr.data(), n, touch_ptr.data(), touch_idx.data(), par[0], par[1],
                  par[2]};
    int err = 0;
    std::vector<int32_t> lab((size_t)n);
    for (int64_t k = 0; k < n_masks; ++k) {
        const int32_t *al = alive.data() + k * n;
        for (int64_t i = 0; i < n; ++i) lab[i] = al[i] != 0 ? (int32_t)i : -1;
        int64_t sweeps = 0;
        for (bool stored = true; stored; ++sweeps) {
            stored = false;
            for (int64_t i = 0; i < n; ++i) stored |= lower_label(g, lab.data(), i, err);
        }
        int64_t roots = 0;
        for (int64_t i = 0; i < n; ++i) roots += lab[i] == i ? 1 : 0;
        printf("%lld %lld\n", (long long)roots, (long long)sweeps);
    }
    printf("err %d\n", err);

    // rows 0 .. 3 of four tiles: {1, 2^31 - 1}, {0, -1}, {2}, {2}; tile 1 is dead
    const int32_t col_ptr[] = {0, 2, 4, 5, 6}, col_idx[] = {1, 0x7fffffff, 0, -1, 2, 2}, al[] = {1, 0, 1, 1};
    for (int64_t i = 0; i < 4; ++i)
        for (int stride = 1; stride <= 2; ++stride)
            for (int first = 0; first < stride; ++first) {
                int e = 0;
                const bool hit = collides(col_ptr, col_idx, al, i, 4, first, stride, e);
                printf("collides %lld %d %d %d %d\n", (long long)i, first, stride, hit ? 1 : 0, e);
            }
    return 0;
}
