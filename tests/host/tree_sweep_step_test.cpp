// Stand-alone run of tilingnn_amd/csrc/tree_sweep_step.h -- the rule tree_sweep_walk_kernel applies per visited node -- with the
// acceptance steps of hole_sweep_step.h, on the host: the sweep of ONE branch (node i = tile i), TWO passes over every visiting
// order of a file (the second one backwards, the state and the draw count carried over: it meets the labelled nodes), with scripted
// p and draws, checked here against the subset table of the loop-tracing oracle that the file carries.  No device, no HIP header:
//   g++ -std=c++17 -O1 -fsanitize=address,undefined -I tilingnn_amd/csrc tests/host/tree_sweep_step_test.cpp
// (tests/test_tree_search_host.py writes the file, builds and runs this, and repeats the walk on its own from the table.)
//
// File: int64 n_tiles, n_pts, n_touch, n_nbr, n_orders, check_holes; double tol, dir_x, dir_y; then ring_xy [n_pts][2] f64,
// ring_ptr [n_tiles + 1] i32, touch_ptr [n_tiles + 1] i32, touch_idx [n_touch] i32, nbr_ptr [n_tiles + 1] i32, nbr_idx [n_nbr] i32
// (scripted "collision" rows: what an acceptance labels), want [2^n_tiles][2] i32 = (components, holes) of every subset, p
// [n_tiles] f64 by position, orders [n_orders][n_tiles] u8.  Draw j of order o is ((7 o + 13 j) mod 32) / 32.
// A pass ends at a BREAK (the first pass then hands over to the second).
// Checked per evaluated visit (check_holes): d holes == want[m | 1 << t].holes - want[m].holes for the selection m; per
// acceptance: every label is the lowest alive tile of its component (a union-find made here), dead tiles -1, and the accepted and
// killed lists together fit the list length.
// Output file: int32 [n_orders][8] = {positions reached, vetoes, draws, accepted, killed, skipped, breaks, final selection as bits};
// stdout: "orders O visits V mismatches M err E".  Exit status 1 on a mismatch.
#include <stdio.h>
#include <stdlib.h>

#include <vector>

#include "tree_sweep_step.h"

using namespace tgnn;

struct HostArcs {
    double lo_[topo::kMaxWedges], hi_[topo::kMaxWedges];
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
    if (argc != 3) return 2;
    FILE *f = fopen(argv[1], "rb");
    if (!f) return 2;
    const std::vector<int64_t> head = read_array<int64_t>(f, 6);
    const std::vector<double> par = read_array<double>(f, 3);
    const int64_t n = head[0], n_pts = head[1], n_touch = head[2], n_nbr = head[3], n_orders = head[4];
    const bool check_holes = head[5] != 0;
    if (n < 1 || n > 16) return 2;
    const std::vector<double> ring_xy = read_array<double>(f, 2 * (size_t)n_pts);
    const std::vector<int32_t> ring_ptr = read_array<int32_t>(f, (size_t)n + 1), touch_ptr = read_array<int32_t>(f, (size_t)n + 1);
    const std::vector<int32_t> touch_idx = read_array<int32_t>(f, (size_t)n_touch);
    const std::vector<int32_t> nbr_ptr = read_array<int32_t>(f, (size_t)n + 1), nbr_idx = read_array<int32_t>(f, (size_t)n_nbr);
    const std::vector<int32_t> want = read_array<int32_t>(f, 2 * ((size_t)1 << n));
    const std::vector<double> p = read_array<double>(f, (size_t)n);
    const std::vector<uint8_t> orders = read_array<uint8_t>(f, (size_t)n_orders * (size_t)n);
    fclose(f);
    const topo::Tiles g{reinterpret_cast<const topo::Pt *>(ring_xy.data()), ring_ptr.data(), n, touch_ptr.data(), touch_idx.data(),
                        par[0], par[1], par[2]};
    int err = 0;
    long visits = 0, mismatches = 0;
    HostArcs arcs;
    std::vector<int32_t> alive((size_t)n), label((size_t)n), chi((size_t)n), unl((size_t)n), parent((size_t)n), out((size_t)n_orders * 8);
    for (int64_t o = 0; o < n_orders; ++o) {
        for (int64_t i = 0; i < n; ++i) alive[i] = 0, label[i] = -1, unl[i] = 1, chi[i] = sweep::kChiUnknown;
        int mask = 0, reached = 0, vetoes = 0, draws = 0, accepted = 0, killed = 0, skipped = 0, breaks = 0;
        for (int64_t step = 0; step < 2 * n; ++step) {               // two passes, the second backwards
            const int64_t pos = step < n ? step : 2 * n - 1 - step;
            const int64_t node = orders[o * n + pos], t = node;
            if (node >= n) return 2;
            ++reached;
            ++visits;
            const bool labelled = unl[node] == 0;
            double u = 0.0;
            int d = 0;
            if (tree::consumes_draw(labelled)) {
                u = (double)((7 * o + 13 * draws) % 32) / 32.0;
                ++draws;
            } else if (check_holes) {
                d = sweep::hole_delta(g, alive.data(), label.data(), chi.data(), t, arcs, err);
                const int expect = want[2 * (mask | 1 << t) + 1] - want[2 * mask + 1];
                if (d != expect && ++mismatches <= 10)
                    fprintf(stderr, "order %ld position %ld: selection %#x tile %ld: d holes %d, expected %d\n", (long)o, (long)pos, mask,
                            (long)t, d, expect);
            }
            const int code = tree::visit_code(labelled, u, p[pos], check_holes, d);
            if (code == sweep::kBreak) {                                 // this pass is over
                ++breaks;
                if (step >= n) break;
                step = n - 1;
                continue;
            }
            skipped += code == tree::kSkipped;
            vetoes += code == sweep::kVetoed;
            if (code != sweep::kAccepted) continue;
            if (!tree::lists_fit(accepted, killed, 1, n)) ++mismatches;
            unl[node] = 0;
            ++accepted;
            int32_t m = sweep::begin_merge(alive.data(), label.data(), t);
            for (int cc = touch_ptr[t]; cc < touch_ptr[t + 1]; ++cc) {
                const int32_t root = sweep::mark_root(g, label.data(), t, cc, err);
                m = root < m ? root : m;
                sweep::forget_chi(g, chi.data(), cc, err);
            }
            for (int64_t i = 0; i < n; ++i) sweep::join_member(label.data(), n, i, m);
            for (int64_t i = 0; i < n; ++i) sweep::close_root(label.data(), i, m);
            mask |= 1 << t;
            // the label invariant: -1 for a dead tile, else the lowest alive tile of its component
            for (int32_t i = 0; i < n; ++i) parent[i] = i;
            for (int32_t i = 0; i < n; ++i) {
                if (alive[i] == 0) continue;
                for (int cc = touch_ptr[i]; cc < touch_ptr[i + 1]; ++cc) {
                    const int32_t j = touch_idx[cc];
                    if (alive[j] == 0) continue;
                    const int32_t a = find(parent, i), b = find(parent, j);
                    if (a != b) parent[a > b ? a : b] = a > b ? b : a;
                }
            }
            for (int32_t i = 0; i < n; ++i) {
                const int32_t expect_label = (mask >> i & 1) ? find(parent, i) : -1;
                if ((alive[i] != 0) != ((mask >> i & 1) != 0) || label[i] != expect_label) {
                    if (++mismatches <= 10)
                        fprintf(stderr, "order %ld position %ld: selection %#x: label[%d] = %d, expected %d\n", (long)o, (long)pos, mask, i,
                                label[i], expect_label);
                }
            }
            for (int64_t cc = nbr_ptr[node]; cc < nbr_ptr[node + 1]; ++cc) {
                const int32_t v = sweep::killed_by(nbr_idx.data(), nbr_ptr[node], cc, unl.data(), n, err);
                if (v < 0) continue;
                if (!tree::lists_fit(accepted, killed, 1, n)) ++mismatches;
                unl[v] = 0;
                ++killed;
            }
        }
        int32_t *row = out.data() + o * 8;
        row[0] = reached, row[1] = vetoes, row[2] = draws, row[3] = accepted, row[4] = killed, row[5] = skipped, row[6] = breaks, row[7] = mask;
    }
    FILE *w = fopen(argv[2], "wb");
    if (!w || fwrite(out.data(), sizeof(int32_t), out.size(), w) != out.size()) return 2;
    fclose(w);
    printf("orders %ld visits %ld mismatches %ld err %d\n", (long)n_orders, visits, mismatches, err);
    return mismatches != 0;
}
