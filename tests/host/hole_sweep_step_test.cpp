// Stand-alone run of tilingnn_amd/csrc/hole_sweep_step.h -- the steps hole_sweep_walk_kernel runs per visited node -- on the
// host: the guarded walk of ONE layout (node i = tile i), TWO rounds over every visiting order of a file (the second one backwards; the
// state and the draw count carried over), with scripted thresholds and draws, checked here against the subset table of the loop-tracing oracle that the file carries.  No device, no HIP header:
//   g++ -std=c++17 -O1 -fsanitize=address,undefined -I tilingnn_amd/csrc tests/host/hole_sweep_step_test.cpp
// (tests/test_hole_sweep_host.py writes the file, builds and runs this, and repeats the walk on its own from the table.)
//
// File: sweep_host.h's, with no further head word and thr as its rate.  The acceptance, the label invariant and the kill loop
// are HostWalk::accept there.
// Checked per visit: d holes == want[m | 1 << t].holes - want[m].holes for the selection m; per acceptance: every label is the
// lowest alive tile of its component (a union-find made here), dead tiles -1.  d components is counted at every visit; d chi
// goes through the chi_cache of the walk (forgotten for the row of every accepted tile: a stale entry would show as a wrong
// d holes), and where the cache does not know it, it is a function of (m, t): computed by sweep::chi_sum the first time a pair
// shows up and looked up afterwards.
// Output file: int32 [n_orders][6] = {positions reached, vetoes, draws, accepted, killed, final selection as bits};
// stdout: "orders O visits V evaluated E mismatches M err E hits H" (H: visits answered from the cache).  Exit status 1 on a mismatch.
#include "sweep_host.h"

int main(int argc, char **argv) {
    if (argc != 3) return 2;
    HostWalk w(argv[1], 5);
    const int64_t n = w.n, n_orders = w.n_orders;
    const topo::Tiles &g = w.g;
    const std::vector<double> &thr = w.rate;
    std::vector<int32_t> &alive = w.alive, &label = w.label, &chi = w.chi, &unl = w.unl;
    HostArcs &arcs = w.arcs;
    int &err = w.err, &mask = w.mask;
    long &mismatches = w.mismatches;
    long visits = 0, evaluated = 0;
    const int kUnknown = 1 << 20;
    long hits = 0;
    std::vector<int> memo(((size_t)1 << n) * (size_t)n, kUnknown);
    std::vector<int32_t> out((size_t)n_orders * 6);
    for (int64_t o = 0; o < n_orders; ++o) {
        w.reset();
        int reached = 0, vetoes = 0, draws = 0;
        for (int64_t step = 0; step < 2 * n; ++step) {               // two rounds, the second backwards: it meets the cache
            const int64_t pos = step < n ? step : 2 * n - 1 - step;
            const int64_t node = w.orders[o * n + pos], t = node;
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
            w.check_delta(d, o, pos, t);
            if (d > 0) {
                ++vetoes;
                continue;
            }
            const double u = scripted_draw(o, draws);
            ++draws;
            if (!(thr[pos] > u)) continue;
            w.accept(o, pos, node, n);                                   // (a layout's killed list holds every node of it)
        }
        int32_t *row = out.data() + o * 6;
        row[0] = reached, row[1] = vetoes, row[2] = draws, row[3] = w.accepted, row[4] = w.killed, row[5] = mask;
    }
    if (!HostWalk::write_rows(argv[2], out)) return 2;
    printf("orders %ld visits %ld evaluated %ld mismatches %ld err %d hits %ld\n", (long)n_orders, visits, evaluated, mismatches, err, hits);
    return mismatches != 0;
}
