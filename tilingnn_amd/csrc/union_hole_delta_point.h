// The local terms of csrc/union_hole_delta.hip: what adding ONE tile t to a collision-free mask does to the components and to the
// Euler characteristic of the closed union -- holes = components - chi, so {d components, d holes} of every candidate follow
// without building a polygon.  Plain C++ like union_topology_point.h (no HIP header, no global state): the kernel calls these per
// candidate and per (candidate, affected tile); a host program calls the very same code
// (tests/host/union_hole_delta_test.cpp, under AddressSanitizer and UBSan).
//
// d components(t) = 1 - the number of distinct component labels among the alive tiles of t's contact row: t joins every
// component it touches into one, or is a new one.
//
// d chi(t): chi is a sum over the distinct vertex positions p of the alive tiles (union_topology_point.h).  Adding t changes the
// term of p only where t touches p, that is at the vertices of t and at the vertices of alive tiles that lie on t's closed ring.
// Every tile that touches such a p shares p with t, so it is in t's contact row: the sums below run over {t} and the alive tiles
// of that row only.
//   after  = sum over i in {t} + alive row, over the vertices v of i within tol of t's ring (all of them for i = t), of the point
//            term with t counted as alive (alive test AND owner rule: point_term_with<true>);
//   before = sum over i in alive row, over the same vertices, of today's point term.
// A tile that does not own the point returns 0, so each position counts once on each side.  A position only t has a vertex at
// is no vertex position before: it contributed 0 (inside a side of an alive tile there is one arc below it: 1 - 1).
// The owner of p before t was added has a vertex within tol of a vertex that is within tol of t's ring, 2 tol at the most:
// region.check_tolerance_gap, which every graph passes before its geometry is uploaded, guarantees that nothing lies between
// tol and the smallest real feature, so that vertex is within tol of the ring too, the contact row (built with tol) holds its
// tile and the ring test below finds it.  There is no second tolerance.
#ifndef TGNN_UNION_HOLE_DELTA_POINT_H
#define TGNN_UNION_HOLE_DELTA_POINT_H
#include "union_topology_point.h"

namespace tgnn {
namespace topo {

constexpr int kStateCandidate = 0, kStateAlive = 1, kStateBlocked = 2, kStateRefused = 3;    // TGNN_HOLE_STATE_* (include/tgnn.h)

// p within tol of a vertex of tile t or of the inside of one of its sides (the test of point_term, same arithmetic)
TGNN_TOPO_FN bool on_ring(const Tiles &g, int64_t t, Pt p) {
    const int w0 = g.ring_ptr[t], m = g.ring_ptr[t + 1] - w0;
    const Pt *r = g.ring_xy + w0;
    const double tol2 = g.tol * g.tol;
    bool on = false;
    Pt a = r[0];
    for (int w = 0; w < m; ++w) {
        const Pt b = r[w + 1 == m ? 0 : w + 1];
        const double rx = p.x - a.x, ry = p.y - a.y, ex = b.x - a.x, ey = b.y - a.y;
        const double ee = ex * ex + ey * ey, along = rx * ex + ry * ey, across = rx * ey - ry * ex;
        on |= rx * rx + ry * ry <= tol2 || (along > 0.0 && along < ee && across * across <= tol2 * ee);
        a = b;
    }
    return on;
}

// The distinct labels among the alive tiles of t's contact row whose FIRST entry in the row is one of the entries part,
// part + parts, ... (the kernel shares a row among `parts` lanes and adds their counts; the whole row: part 0 of 1).
// label [n_tiles]: -1 for a dead tile, else the lowest alive tile of its component.  n_alive: the alive tiles among these entries.
TGNN_TOPO_FN int distinct_labels(const Tiles &g, const int32_t *label, int64_t t, int part, int parts, int &n_alive, int &err) {
    const int c0 = g.touch_ptr[t], c1 = g.touch_ptr[t + 1];
    int distinct = 0;
    n_alive = 0;
    for (int cc = c0 + part; cc < c1; cc += parts) {
        const int64_t j = g.touch_idx[cc];
        if (j < 0 || j >= g.n_tiles) {
            err |= kErrIndex;
            continue;
        }
        const int32_t lj = label[j];
        if (j == t || lj < 0) continue;
        ++n_alive;
        bool seen = false;                                   // rows are short (58 at the most on ring 9): compare with the earlier ones
        for (int bb = c0; bb < cc; ++bb) {
            const int64_t u = g.touch_idx[bb];
            seen |= u >= 0 && u < g.n_tiles && u != t && label[u] == lj;
        }
        distinct += seen ? 0 : 1;
    }
    return distinct;
}

// d components(t) = 1 - the distinct labels among the alive tiles of t's contact row: t joins the components it touches into
// one, or is a new one.  n_alive: the alive tiles of the row (0: t touches nothing, the answer is {+1, 0} without more work).
TGNN_TOPO_FN int delta_components(const Tiles &g, const int32_t *label, int64_t t, int &n_alive, int &err) {
    return 1 - distinct_labels(g, label, t, 0, 1, n_alive, err);
}

// One term of d chi(t): vertex v of tile i (t itself, or an alive tile of t's contact row with 3 vertices or more), `before`
// the term it had without t (negative; nothing for i = t), else the term it has with t counted.  0 when v is not on t's ring.
template <class Arcs>
TGNN_TOPO_FN int delta_chi_vertex(const Tiles &g, const int32_t *alive, int64_t t, int64_t i, int v, bool before, Arcs &arcs,
                                  int &err) {
    if (i != t && !on_ring(g, t, g.ring_xy[g.ring_ptr[i] + v])) return 0;
    if (before) return i != t ? -point_term(g, alive, i, v, arcs, err) : 0;
    return point_term_with<true>(g, alive, t, i, v, arcs, err);
}

// The share of tile i in d chi(t): after - before over the vertices of i on t's ring.
template <class Arcs>
TGNN_TOPO_FN int delta_chi_tile(const Tiles &g, const int32_t *alive, int64_t t, int64_t i, Arcs &arcs, int &err) {
    const int n = g.ring_ptr[i + 1] - g.ring_ptr[i];
    int sum = 0;
    for (int v = 0; v < n; ++v)
        sum += delta_chi_vertex(g, alive, t, i, v, false, arcs, err) + delta_chi_vertex(g, alive, t, i, v, true, arcs, err);
    return sum;
}

// Whether entry cc of t's contact row names a tile with a share in d chi(t); j gets the tile.
TGNN_TOPO_FN bool delta_chi_row_tile(const Tiles &g, const int32_t *alive, int64_t t, int cc, int64_t &j, int &err) {
    j = g.touch_idx[cc];
    if (j < 0 || j >= g.n_tiles) {
        err |= kErrIndex;
        return false;
    }
    return j != t && alive[j] != 0 && g.ring_ptr[j + 1] - g.ring_ptr[j] >= 3;
}

// chi(mask + t) - chi(mask) for a dead tile t of 3 vertices or more that collides with no alive tile.
template <class Arcs>
TGNN_TOPO_FN int delta_chi(const Tiles &g, const int32_t *alive, int64_t t, Arcs &arcs, int &err) {
    int sum = delta_chi_tile(g, alive, t, t, arcs, err);
    for (int cc = g.touch_ptr[t]; cc < g.touch_ptr[t + 1]; ++cc) {
        int64_t j;
        if (delta_chi_row_tile(g, alive, t, cc, j, err)) sum += delta_chi_tile(g, alive, t, j, arcs, err);
    }
    return sum;
}

}  // namespace topo
}  // namespace tgnn
#endif
