// The per-visit rule of csrc/tree_sweep.hip: the sweep of ONE branch of the tree search (the reference's algorithms.py:138-157,
// solve_by_treesearch) over its sampled visiting order, one position at a time.  Plain C++ like hole_sweep_step.h, whose steps an
// acceptance runs unchanged (begin_merge, mark_root, join_member, close_root, forget_chi, killed_by); a host program calls the very
// same code with one worker (tests/host/tree_sweep_step_test.cpp, under AddressSanitizer and UBSan).
//
// The rule differs from the greedy sweep's (hole_sweep.hip) in where the draw sits:
//   a node that is no longer unlabelled consumes ONE draw u: u < p passes over it (:145-146, kSkipped), else the walk ends
//   (:147-148, kBreak);
//   with check_holes a node whose tile has d holes > 0 under the branch's selection is passed over, NO draw (:151-152, kVetoed);
//   every other node is accepted, NO draw (:155-157): kRejected does not occur.
// u < p is a plain fp64 compare of two host-made numbers (p may exceed 1: the reference's quirk is kept).
#ifndef TGNN_TREE_SWEEP_STEP_H
#define TGNN_TREE_SWEEP_STEP_H
#include "hole_sweep_step.h"

namespace tgnn {
namespace tree {

constexpr int kSkipped = 5;                  // TGNN_SWEEP_SKIPPED; the other codes of a trace word are sweep::k*
// the words of a branch's row of stats_out, TGNN_TREE_STAT_*
constexpr int kStatVisited = 0, kStatVetoes = 1, kStatDraws = 2, kStatAccepted = 3, kStatKilled = 4, kStatSkipped = 5, kStatWords = 8;

// What one visit decides.  labelled: the node is no longer unlabelled; u: the branch's next uniform (read only then); p: prob_m of
// the position; d: d holes of the node's tile (looked at only with check_holes, and never for a labelled node).
TGNN_TOPO_FN int visit_code(bool labelled, double u, double p, bool check_holes, int d) {
    if (labelled) return u < p ? kSkipped : sweep::kBreak;
    return check_holes && d > 0 ? sweep::kVetoed : sweep::kAccepted;
}

TGNN_TOPO_FN bool consumes_draw(bool labelled) { return labelled; }

// Whether `more` further nodes fit the branch's killed list: accepted and killed nodes are distinct unlabelled nodes of the
// branch's state and every one of them stands in its visiting list, so both lists together never exceed the list's length -- on
// tables that keep the contract.  The walk checks instead of trusting.
TGNN_TOPO_FN bool lists_fit(int64_t n_accepted, int64_t n_killed, int64_t more, int64_t n_visit) {
    return n_accepted + n_killed + more <= n_visit;
}

}  // namespace tree
}  // namespace tgnn
#endif
