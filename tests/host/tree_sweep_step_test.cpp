// Stand-alone run of tilingnn_amd/csrc/tree_sweep_step.h -- the rule tree_sweep_walk_kernel applies per visited node -- with the
// acceptance steps of hole_sweep_step.h, on the host: the sweep of ONE branch (node i = tile i), TWO passes over every visiting
// order of a file (the second one backwards, the state and the draw count carried over: it meets the labelled nodes), with scripted
// p and draws, checked here against the subset table of the loop-tracing oracle that the file carries.  No device, no HIP header:
//   g++ -std=c++17 -O1 -fsanitize=address,undefined -I tilingnn_amd/csrc tests/host/tree_sweep_step_test.cpp
// (tests/test_tree_search_host.py writes the file, builds and runs this, and repeats the walk on its own from the table.)
//
// File: sweep_host.h's, with check_holes as the sixth head word and p as its rate.  The acceptance, the label invariant and the
// kill loop are HostWalk::accept there.
// A pass ends at a BREAK (the first pass then hands over to the second).
// Checked per evaluated visit (check_holes): d holes == want[m | 1 << t].holes - want[m].holes for the selection m; per
// acceptance: every label is the lowest alive tile of its component (a union-find made here), dead tiles -1, and the accepted and
// killed lists together fit the list length.
// Output file: int32 [n_orders][8] = {positions reached, vetoes, draws, accepted, killed, skipped, breaks, final selection as bits};
// stdout: "orders O visits V mismatches M err E".  Exit status 1 on a mismatch.
#include "sweep_host.h"
#include "tree_sweep_step.h"

int main(int argc, char **argv) {
    if (argc != 3) return 2;
    HostWalk w(argv[1], 6);
    const int64_t n = w.n, n_orders = w.n_orders;
    const bool check_holes = w.head[5] != 0;
    const std::vector<double> &p = w.rate;
    long &mismatches = w.mismatches;
    long visits = 0;
    std::vector<int32_t> out((size_t)n_orders * 8);
    for (int64_t o = 0; o < n_orders; ++o) {
        w.reset();
        int reached = 0, vetoes = 0, draws = 0, skipped = 0, breaks = 0;
        for (int64_t step = 0; step < 2 * n; ++step) {               // two passes, the second backwards
            const int64_t pos = step < n ? step : 2 * n - 1 - step;
            const int64_t node = w.orders[o * n + pos], t = node;
            if (node >= n) return 2;
            ++reached;
            ++visits;
            const bool labelled = w.unl[node] == 0;
            double u = 0.0;
            int d = 0;
            if (tree::consumes_draw(labelled)) {
                u = scripted_draw(o, draws);
                ++draws;
            } else if (check_holes) {
                d = sweep::hole_delta(w.g, w.alive.data(), w.label.data(), w.chi.data(), t, w.arcs, w.err);
                w.check_delta(d, o, pos, t);
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
            if (!tree::lists_fit(w.accepted, w.killed, 1, n)) ++mismatches;
            w.accept(o, pos, node, n - w.accepted - 1);                  // (lists_fit for every kill, the node counted)
        }
        int32_t *row = out.data() + o * 8;
        row[0] = reached, row[1] = vetoes, row[2] = draws, row[3] = w.accepted, row[4] = w.killed, row[5] = skipped, row[6] = breaks, row[7] = w.mask;
    }
    if (!HostWalk::write_rows(argv[2], out)) return 2;
    printf("orders %ld visits %ld mismatches %ld err %d\n", (long)n_orders, visits, mismatches, w.err);
    return mismatches != 0;
}
