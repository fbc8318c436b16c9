// Stand-alone run of tilingnn_amd/csrc/union_topology_point.h -- the code union_topology_chi_kernel runs per (mask, tile, vertex)
// -- on the host: reads tiles, contact rows and masks from a file, prints the sum of the local Euler terms per mask.  No device,
// no HIP header:
//   g++ -std=c++17 -O1 -fsanitize=address,undefined -I tilingnn_amd/csrc tests/host/union_topology_point_test.cpp
// (tests/test_union_topology_host.py writes the file, builds and runs this, and compares with the loop-tracing oracle).
//
// File: int64 n_tiles, n_pts, n_touch, n_masks; double tol, dir_x, dir_y; then ring_xy [n_pts][2] f64, ring_ptr [n_tiles + 1] i32,
// touch_ptr [n_tiles + 1] i32, touch_idx [n_touch] i32, alive [n_masks][n_tiles] i32.
#include <stdio.h>
#include <stdlib.h>

#include <vector>

#include "union_topology_point.h"

using namespace tgnn::topo;

struct HostArcs {
    double lo_[kMaxWedges], hi_[kMaxWedges];
    double &lo(int q) { return lo_[q]; }
    double &hi(int q) { return hi_[q]; }
};

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
    HostArcs arcs;
    for (int64_t k = 0; k < n_masks; ++k) {
        const int32_t *al = alive.data() + k * n;
        int chi = 0;
        for (int64_t i = 0; i < n; ++i) {
            if (al[i] == 0) continue;
            for (int v = 0; v < ring_ptr[i + 1] - ring_ptr[i]; ++v) chi += point_term(g, al, i, v, arcs, err);
        }
        printf("%d\n", chi);
    }
    printf("err %d\n", err);
    return 0;
}
