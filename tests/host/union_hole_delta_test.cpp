// Stand-alone run of tilingnn_amd/csrc/union_hole_delta_point.h -- the code union_hole_delta_kernel runs per candidate and per
// (candidate, affected tile) -- on the host: reads tiles, contact rows, masks and the expected {d components, d holes} of every
// (mask, dead tile) from a file, computes both with delta_components (over labels made here by a union-find) and delta_chi, and
// compares.  No device, no HIP header:
//   g++ -std=c++17 -O1 -fsanitize=address,undefined -I tilingnn_amd/csrc tests/host/union_hole_delta_test.cpp
// (tests/test_union_hole_delta_host.py writes the file from the loop-tracing oracle, builds and runs this).
//
// File: int64 n_tiles, n_pts, n_touch, n_masks; double tol, dir_x, dir_y; then ring_xy [n_pts][2] f64, ring_ptr [n_tiles + 1] i32,
// touch_ptr [n_tiles + 1] i32, touch_idx [n_touch] i32, alive [n_masks][n_tiles] i32, want [n_masks][n_tiles][2] i32 (read for
// the dead tiles only; the sets have no collision).
// Output: one line "dc dh count" per distinct pair computed, then "pairs P mismatches M err E".  Exit status 1 on a mismatch.
#include <stdio.h>
#include <stdlib.h>

#include <map>
#include <utility>
#include <vector>

#include "union_hole_delta_point.h"

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

static int32_t find(std::vector<int32_t> &parent, int32_t a) {
    while (parent[a] != a) a = parent[a] = parent[parent[a]];
    return a;
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
    const std::vector<int32_t> want = read_array<int32_t>(f, 2 * (size_t)n_masks * (size_t)n);
    fclose(f);
    const Tiles g{reinterpret_cast<const Pt *>(ring_xy.data()), ring_ptr.data(), n, touch_ptr.data(), touch_idx.data(), par[0], par[1],
                  par[2]};
    int err = 0;
    long pairs = 0, mismatches = 0;
    std::map<std::pair<int, int>, long> seen;
    HostArcs arcs;
    std::vector<int32_t> parent((size_t)n), label((size_t)n);
    for (int64_t k = 0; k < n_masks; ++k) {
        const int32_t *al = alive.data() + k * n;
        // labels: -1 for a dead tile, else the lowest alive tile of its component (what union_hole_delta_label_kernel leaves)
        for (int32_t i = 0; i < n; ++i) parent[i] = i;
        for (int32_t i = 0; i < n; ++i) {
            if (al[i] == 0) continue;
            for (int cc = touch_ptr[i]; cc < touch_ptr[i + 1]; ++cc) {
                const int32_t j = touch_idx[cc];
                if (al[j] == 0) continue;
                const int32_t a = find(parent, i), b = find(parent, j);
                if (a != b) parent[a > b ? a : b] = a > b ? b : a;       // the lower index stays the root
            }
        }
        for (int32_t i = 0; i < n; ++i) label[i] = al[i] != 0 ? find(parent, i) : -1;
        for (int64_t t = 0; t < n; ++t) {
            if (al[t] != 0) continue;
            int touching = 0;
            const int dc = delta_components(g, label.data(), t, touching, err);
            int shared = 0, shared_touching = 0;                         // the kernel shares a row among four lanes
            for (int part = 0; part < 4; ++part) {
                int here = 0;
                shared += distinct_labels(g, label.data(), t, part, 4, here, err);
                shared_touching += here;
            }
            if (1 - shared != dc || shared_touching != touching) {
                fprintf(stderr, "mask %ld tile %ld: the row in four parts gives %d labels, whole %d\n", (long)k, (long)t, shared, 1 - dc);
                ++mismatches;
            }
            const int dchi = touching != 0 ? delta_chi(g, al, t, arcs, err) : 1;
            if (touching == 0 && delta_chi(g, al, t, arcs, err) != 1) {  // the shortcut of the kernel: a tile alone adds {+1, 0}
                fprintf(stderr, "mask %ld tile %ld touches nothing and d chi is not 1\n", (long)k, (long)t);
                ++mismatches;
            }
            const int dh = dc - dchi;
            const int32_t *w = want.data() + 2 * (k * n + t);
            ++pairs;
            ++seen[{dc, dh}];
            if (dc != w[0] || dh != w[1]) {
                if (++mismatches <= 10)
                    fprintf(stderr, "mask %ld tile %ld: {%d, %d}, expected {%d, %d}\n", (long)k, (long)t, dc, dh, w[0], w[1]);
            }
        }
    }
    for (const auto &kv : seen) printf("%d %d %ld\n", kv.first.first, kv.first.second, kv.second);
    printf("pairs %ld mismatches %ld err %d\n", pairs, mismatches, err);
    return mismatches != 0;
}
