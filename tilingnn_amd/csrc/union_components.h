// The two per-tile steps that csrc/union_topology.hip, csrc/union_hole_delta.hip and csrc/union_contour.hip share: whether an alive
// tile collides with another alive tile, and one tile's step of a round of component labelling.  Plain C++ like
// union_topology_point.h (no HIP header, no global state): the kernels call these per tile (union_masks.h: label_components runs
// the rounds), and a host program calls the very same code (tests/host/union_components_test.cpp, under AddressSanitizer and
// UBSan).
#ifndef TGNN_UNION_COMPONENTS_H
#define TGNN_UNION_COMPONENTS_H
#include "union_topology_point.h"

namespace tgnn {
namespace topo {

// Whether one of the entries first, first + stride, ... of row i of the collision CSR names an alive tile other than i (the
// whole row: 0, 1; the hole-delta kernel shares a row among `stride` lanes).  alive [n].  An entry outside [0, n) sets kErrIndex
// and is passed over.
TGNN_TOPO_FN bool collides(const int32_t *col_ptr, const int32_t *col_idx, const int32_t *alive, int64_t i, int64_t n, int first,
                           int stride, int &err) {
    bool hit = false;
    for (int cc = col_ptr[i] + first; cc < col_ptr[i + 1]; cc += stride) {
        const int64_t j = col_idx[cc];
        if (j < 0 || j >= n) {
            err |= kErrIndex;
            continue;
        }
        hit |= j != i && alive[j] != 0;
    }
    return hit;
}

// One tile's step of a round of min-label propagation over the contact rows.  lab [n_tiles]: -1 for a dead tile, else the index
// of an alive tile of the same component.  Tile i takes the lowest live label of its contact row, follows the labels from there
// to the current root (pointer jumping: labels strictly decrease along the way), and stores the result when it is lower than
// its own; returns whether it stored.  Labels only ever decrease, so a label read while its owner lowers it is merely one step
// old.  An entry outside [0, n_tiles) sets kErrIndex and is passed over.
TGNN_TOPO_FN bool lower_label(const Tiles &g, volatile int32_t *lab, int64_t i, int &err) {
    const int32_t old = lab[i];
    if (old < 0) return false;
    int32_t best = old;
    for (int cc = g.touch_ptr[i]; cc < g.touch_ptr[i + 1]; ++cc) {
        const int64_t j = g.touch_idx[cc];
        if (j < 0 || j >= g.n_tiles) {
            err |= kErrIndex;
            continue;
        }
        const int32_t lj = lab[j];
        best = lj >= 0 && lj < best ? lj : best;
    }
    for (;;) {
        const int32_t up = lab[best];
        if (up >= best) break;
        best = up;
    }
    if (best < old) lab[i] = best;
    return best < old;
}

}  // namespace topo
}  // namespace tgnn
#endif
