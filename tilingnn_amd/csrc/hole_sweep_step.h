// The per-visit steps of csrc/hole_sweep.hip: the guarded acceptance sweep of util/algorithms.py (HostSweep.round with a
// HoleGuard: the reference's algorithms.py:41-54 with the hole veto of :150-152 before the draw) for ONE layout, one visited
// node at a time.  Plain C++ like union_hole_delta_point.h (no HIP header, no global state): the kernel shares every step among
// the threads of a block -- worker `part` of `parts` -- with a barrier between two steps; a host program calls the very same
// code with one worker (tests/host/hole_sweep_step_test.cpp, under AddressSanitizer and UBSan).
//
// The state of a layout: alive [n_tiles] (its selected tiles) and label [n_tiles], -1 for a dead tile, else the LOWEST alive tile
// of its component -- the convention of union_hole_delta_label_kernel, so topo::distinct_labels reads it unchanged.
//
// d holes of a visited tile t = (1 - distinct labels of the alive tiles of t's contact row) - d chi(t), the value
// tgnn_union_hole_delta gives for t on the same mask: 0 without further work when t touches nothing alive, has fewer than 3
// vertices (the map calls it blocked) or is alive already.  d chi is cut into items (slot, sub): slot 0 is t itself, slot s
// entry s - 1 of its contact row, and the kChiSub subs of a slot are every fourth vertex of that tile, with t counted or not
// (delta_chi_vertex).  Integer terms: any order of summation gives the same sum.
//
// d chi(t) reads nothing but which tiles of t's contact row are alive: every tile that touches a point of t's ring shares that
// point with t, so it is in the row (union_hole_delta_point.h).  chi_cache [n_tiles] keeps it from visit to visit and from round
// to round -- kChiUnknown, or d chi(t) under the present selection -- and accepting a tile forgets the entries of its own row
// (forget_chi; the relation is symmetric), the only ones its acceptance can change.  d components is counted afresh every time:
// the labels depend on far tiles.  Most visits of a solve are vetoes of the same tiles round after round, next to which nothing
// was accepted in between.
//
// Accepting t keeps the label convention in three steps, each a pass that reads only what the step before left:
//   begin_merge    alive[t] = 1, label[t] = marked(t);
//   mark_root      per entry of t's row: the root of an alive tile (its label; itself when it is a root) gets marked(root);
//                  the lowest of them and t is the merged component's label m (the caller folds the minimum);
//   join_member    per tile i: a tile whose label names a marked root takes m (only non-roots are written, only roots are read);
//   close_root     per tile i: a marked root takes m.
// marked(r) = -2 - r: neither dead (-1) nor a tile.  Every label of the merged component is m afterwards, the lowest alive
// tile of it, and no other label changed.
#ifndef TGNN_HOLE_SWEEP_STEP_H
#define TGNN_HOLE_SWEEP_STEP_H
#include "union_hole_delta_point.h"

namespace tgnn {
namespace sweep {

// the codes of a trace word, TGNN_SWEEP_* (include/tgnn.h)
constexpr int kNotReached = 0, kBreak = 1, kVetoed = 2, kRejected = 3, kAccepted = 4;
// the words of a layout's row of stats_out, TGNN_SWEEP_STAT_*
constexpr int kStatVisited = 0, kStatVetoes = 1, kStatDraws = 2, kStatAccepted = 3, kStatKilled = 4, kStatAllVetoed = 5, kStatWords = 8;
constexpr int kChiSub = 8;                   // items of one slot of d chi
constexpr int32_t kChiUnknown = -2147483647 - 1;    // a chi_cache entry that is not known

// Whether tile t can change the holes at all under `alive`: dead and of 3 vertices or more.  (Whether it touches an alive tile
// is what distinct_labels' n_alive says.)
TGNN_TOPO_FN bool may_change_holes(const topo::Tiles &g, const int32_t *alive, int64_t t) {
    return alive[t] == 0 && g.ring_ptr[t + 1] - g.ring_ptr[t] >= 3;
}

// Slots of d chi(t): t itself and every entry of its contact row.
TGNN_TOPO_FN int chi_slots(const topo::Tiles &g, int64_t t) { return g.touch_ptr[t + 1] - g.touch_ptr[t] + 1; }

// Whether slot `slot` of d chi(t) names a tile with a share (t itself; an alive tile of the row with 3 vertices or more).
TGNN_TOPO_FN bool chi_slot_has_share(const topo::Tiles &g, const int32_t *alive, int64_t t, int slot, int &err) {
    int64_t j;
    return slot == 0 || topo::delta_chi_row_tile(g, alive, t, g.touch_ptr[t] + slot - 1, j, err);
}

// Item (slot, sub) of d chi(t), slot one that has a share.
template <class Arcs>
TGNN_TOPO_FN int chi_item(const topo::Tiles &g, const int32_t *alive, int64_t t, int slot, int sub, Arcs &arcs, int &err) {
    const int64_t i = slot == 0 ? t : g.touch_idx[g.touch_ptr[t] + slot - 1];
    const int verts = g.ring_ptr[i + 1] - g.ring_ptr[i];
    int sum = 0;
    for (int v = sub >> 1; v < verts; v += kChiSub / 2) sum += topo::delta_chi_vertex(g, alive, t, i, v, (sub & 1) != 0, arcs, err);
    return sum;
}

// d chi(t), every item, by ONE worker (the host program; the kernel shares the items among its threads).
template <class Arcs>
TGNN_TOPO_FN int chi_sum(const topo::Tiles &g, const int32_t *alive, int64_t t, Arcs &arcs, int &err) {
    int dchi = 0;
    for (int slot = 0; slot < chi_slots(g, t); ++slot) {
        if (!chi_slot_has_share(g, alive, t, slot, err)) continue;
        for (int sub = 0; sub < kChiSub; ++sub) dchi += chi_item(g, alive, t, slot, sub, arcs, err);
    }
    return dchi;
}

// d holes of tile t by ONE worker, d chi from chi_cache when it is known there and stored there when it was computed.
template <class Arcs>
TGNN_TOPO_FN int hole_delta(const topo::Tiles &g, const int32_t *alive, const int32_t *label, int32_t *chi_cache, int64_t t,
                            Arcs &arcs, int &err) {
    if (!may_change_holes(g, alive, t)) return 0;
    int touching = 0;
    const int dcomp = topo::delta_components(g, label, t, touching, err);
    if (touching == 0) return 0;
    int dchi = chi_cache[t];
    if (dchi == kChiUnknown) {
        const int before = err;
        dchi = chi_sum(g, alive, t, arcs, err);
        if (err == before) chi_cache[t] = dchi;
    }
    return dcomp - dchi;
}

// Entry cc of the contact row of a tile that is being accepted: d chi of the tile it names is no longer known.
TGNN_TOPO_FN void forget_chi(const topo::Tiles &g, int32_t *chi_cache, int cc, int &err) {
    const int64_t j = g.touch_idx[cc];
    if (j < 0 || j >= g.n_tiles)
        err |= topo::kErrIndex;
    else
        chi_cache[j] = kChiUnknown;
}

TGNN_TOPO_FN int32_t marked(int64_t root) { return (int32_t)(-2 - root); }

// The first step of accepting t (ONE worker).  Returns the start value of the merged label's minimum.
TGNN_TOPO_FN int32_t begin_merge(int32_t *alive, int32_t *label, int64_t t) {
    alive[t] = 1;
    label[t] = marked(t);
    return (int32_t)t;
}

// Entry cc of t's contact row: marks the root of the tile it names, when that tile is alive, and returns the root; n_tiles (no
// root) otherwise.  Workers may run this for different entries at once: they only ever store marked(r) at root r.
TGNN_TOPO_FN int32_t mark_root(const topo::Tiles &g, int32_t *label, int64_t t, int cc, int &err) {
    const int64_t j = g.touch_idx[cc];
    if (j < 0 || j >= g.n_tiles) {
        err |= topo::kErrIndex;
        return (int32_t)g.n_tiles;
    }
    const int32_t lj = label[j];
    if (j == t || lj == -1) return (int32_t)g.n_tiles;
    if (lj >= g.n_tiles) {                                       // (a label array that is not one: reported, nothing touched)
        err |= topo::kErrIndex;
        return (int32_t)g.n_tiles;
    }
    const int32_t root = lj >= 0 ? lj : (int32_t)j;              // (lj <= -2: j is a root another entry has marked)
    label[root] = marked(root);
    return root;
}

TGNN_TOPO_FN void join_member(int32_t *label, int64_t n_tiles, int64_t i, int32_t m) {
    const int32_t li = label[i];
    if (li >= 0 && li < n_tiles && label[li] <= -2) label[i] = m;
}

TGNN_TOPO_FN void close_root(int32_t *label, int64_t i, int32_t m) {
    if (label[i] <= -2) label[i] = m;
}

// Entry cc of the collision row of an accepted node: the local node it labels -- in [0, n_nodes), still unlabelled, and named by
// no earlier entry of the row (rows are short: compare with the earlier ones) -- or -1.  unlabelled: the layout's own [n_nodes].
// The caller clears unlabelled[v] and appends v to the killed list, in entry order.
TGNN_TOPO_FN int32_t killed_by(const int32_t *nbr_idx, int64_t row0, int64_t cc, const int32_t *unlabelled, int64_t n_nodes, int &err) {
    const int32_t v = nbr_idx[cc];
    if (v < 0 || v >= n_nodes) {
        err |= topo::kErrIndex;
        return -1;
    }
    if (unlabelled[v] == 0) return -1;
    for (int64_t bb = row0; bb < cc; ++bb)
        if (nbr_idx[bb] == v) return -1;
    return v;
}

}  // namespace sweep
}  // namespace tgnn
#endif
