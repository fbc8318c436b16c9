// Stand-alone run of tilingnn_amd/csrc/hole_sweep_step.h -- the steps hole_sweep_walk_kernel runs per visited node -- on the
// host: the guarded walk of ONE layout (node i = tile i), TWO rounds over every visiting order of a file (the second one backwards; the
// state and the draw count carried over), with scripted thresholds and draws, checked here against the subset table of the loop-tracing oracle that the file carries.  No device, no HIP header:
//   g++ -std=c++17 -O1 -fsanitize=address,undefined -I tilingnn_amd/csrc tests/host/hole_sweep_step_test.cpp
// (tests/test_hole_sweep_host.py writes the file, builds and runs this, and repeats the walk on its own from the table.)
//
// File: int64 n_tiles, n_pts, n_touch, n_nbr, n_orders; double tol, dir_x, dir_y; then ring_xy [n_pts][2] f64, ring_ptr
// [n_tiles + 1] i32, touch_ptr [n_tiles + 1] i32, touch_idx [n_touch] i32, nbr_ptr [n_tiles + 1] i32, nbr_idx [n_nbr] i32 (scripted
// "collision" rows: what an acceptance labels), want [2^n_tiles][2] i32 = (components, holes) of every subset, thr [n_tiles] f64
// by position, orders [n_orders][n_tiles] u8.  Draw j of order o is ((7 o + 13 j) mod 32) / 32.
// Checked per visit: d holes == want[m | 1 << t].holes - want[m].holes for the selection m; per acceptance: every label is the
// lowest alive tile of its component (a union-find made here), dead tiles -1.  d components is counted at every visit; d chi
// goes through the chi_cache of the walk (forgotten for the row of every accepted tile: a stale entry would show as a wrong
// d holes), and where the cache does not know it, it is a function of (m, t): computed by sweep::chi_sum the first time a pair
// shows up and looked up afterwards.
// Output file: int32 [n_orders][6] = {positions reached, vetoes, draws, accepted, killed, final selection as bits};
// stdout: "orders O visits V evaluated E mismatches M err E hits H" (H: visits answered from the cache).  Exit status 1 on a mismatch.
#include <stdio.h>
#include <stdlib.h>

#include <vector>

#include "hole_sweep_step.h"

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
    const std::vector<int64_t> head = read_array<int64_t>(f, 5);
    const std::vector<double> par = read_array<double>(f, 3);
    const int64_t n = head[0], n_pts = head[1], n_touch = head[2], n_nbr = head[3], n_orders = head[4];
    if (n < 1 || n > 16) return 2;
    const std::vector<double> ring_xy = read_array<double>(f, 2 * (size_t)n_pts);
    const std::vector<int32_t> ring_ptr = read_array<int32_t>(f, (size_t)n + 1), touch_ptr = read_array<int32_t>(f, (size_t)n + 1);
    const std::vector<int32_t> touch_idx = read_array<int32_t>(f, (size_t)n_touch);
    const std::vector<int32_t> nbr_ptr = read_array<int32_t>(f, (size_t)n + 1), nbr_idx = read_array<int32_t>(f, (size_t)n_nbr);
    const std::vector<int32_t> want = read_array<int32_t>(f, 2 * ((size_t)1 << n));
    const std::vector<double> thr = read_array<double>(f, (size_t)n);
    const std::vector<uint8_t> orders = read_array<uint8_t>(f, (size_t)n_orders * (size_t)n);
    fclose(f);
    const topo::Tiles g{reinterpret_cast<const topo::Pt *>(ring_xy.data()), ring_ptr.data(), n, touch_ptr.data(), touch_idx.data(),
                        par[0], par[1], par[2]};
    int err = 0;
    long visits = 0, evaluated = 0, mismatches = 0;
    HostArcs arcs;
    const int kUnknown = 1 << 20;
    long hits = 0;
    std::vector<int> memo(((size_t)1 << n) * (size_t)n, kUnknown);
    std::vector<int32_t> alive((size_t)n), label((size_t)n), chi((size_t)n), unl((size_t)n), parent((size_t)n), out((size_t)n_orders * 6);
    for (int64_t o = 0; o < n_orders; ++o) {
        for (int64_t i = 0; i < n; ++i) alive[i] = 0, label[i] = -1, unl[i] = 1, chi[i] = sweep::kChiUnknown;
        int mask = 0, reached = 0, vetoes = 0, draws = 0, accepted = 0, killed = 0;
        for (int64_t step = 0; step < 2 * n; ++step) {               // two rounds, the second backwards: it meets the cache
            const int64_t pos = step < n ? step : 2 * n - 1 - step;
            const int64_t node = orders[o * n + pos], t = node;
            if (node >= n) return 2;
            ++reached;
            if (unl[node] == 0) {                                        // the break: this round is over
                if (step >= n) break;
                step = n - 1;
                continue;
            }
            ++visits;
            int d = 0, touching = 0;
            if (o < 64) {                                                // the whole cached path of the header, no look-up
                d = sweep::hole_delta(g, alive.data(), label.data(), chi.data(), t, arcs, err);
            } else if (sweep::may_change_holes(g, alive.data(), t)) {
                const int dcomp = topo::delta_components(g, label.data(), t, touching, err);
                if (touching != 0) {
                    if (chi[t] == sweep::kChiUnknown) {
                        int &known = memo[(size_t)mask * n + t];
                        if (known == kUnknown) {
                            known = sweep::chi_sum(g, alive.data(), t, arcs, err);
                            ++evaluated;
                        }
                        chi[t] = known;
                    } else {
                        ++hits;
                    }
                    d = dcomp - chi[t];
                }
            }
            const int expect = want[2 * (mask | 1 << t) + 1] - want[2 * mask + 1];
            if (d != expect && ++mismatches <= 10)
                fprintf(stderr, "order %ld position %ld: selection %#x tile %ld: d holes %d, expected %d\n", (long)o, (long)pos, mask,
                        (long)t, d, expect);
            if (d > 0) {
                ++vetoes;
                continue;
            }
            const double u = (double)((7 * o + 13 * draws) % 32) / 32.0;
            ++draws;
            if (!(thr[pos] > u)) continue;
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
                unl[v] = 0;
                ++killed;
            }
        }
        int32_t *row = out.data() + o * 6;
        row[0] = reached, row[1] = vetoes, row[2] = draws, row[3] = accepted, row[4] = killed, row[5] = mask;
    }
    FILE *w = fopen(argv[2], "wb");
    if (!w || fwrite(out.data(), sizeof(int32_t), out.size(), w) != out.size()) return 2;
    fclose(w);
    printf("orders %ld visits %ld evaluated %ld mismatches %ld err %d hits %ld\n", (long)n_orders, visits, evaluated, mismatches, err, hits);
    return mismatches != 0;
}
