// The per-piece code of csrc/union_contour.hip: the boundary of the closed union of a mask's tiles (tiles that do not overlap) as
// directed pieces and their successors.  Plain C++ on purpose (no HIP header, no global state): the kernels call it per tile and
// per piece, and a host program runs the very same code (tests/host/union_contour_piece_test.cpp, under AddressSanitizer and
// UBSan).
//
//   * side_splits: the vertices of other alive tiles on the open interior of one side, within tol, in order along the side;
//     vertices within tol of each other are one split and the lowest vertex index names it.
//   * piece_has_twin: a piece is inside the union when an alive tile of the contact row has a side running the opposite way over
//     it (the pieces are split at every vertex, so a side covers a piece wholly or not at all: the midpoint decides).
//   * tile_pieces: the kept (boundary) pieces of one tile in piece order (side, position along the side), handed to a sink.
//   * link_piece: the successor of a boundary piece among the pieces that leave its end point: the first one counter-clockwise
//     from its own reversed direction (the turn through the outside).
//
// A point is named by its CANONICAL VERTEX: the lowest index into ring_xy of a vertex of an alive tile within tol of it (ring_ptr
// ascends, so that is the lowest-numbered tile, lowest vertex on a tie).  Two pieces meet when the names agree; no coordinate is
// ever computed.  Lists are fixed-size in storage the caller provides; an overflow sets an error bit, never a guess.
#ifndef TGNN_UNION_CONTOUR_PIECE_H
#define TGNN_UNION_CONTOUR_PIECE_H
#include "union_topology_point.h"

namespace tgnn {
namespace contour {

using topo::Pt;
using topo::Tiles;

constexpr int kMaxSplits = 8;                // distinct foreign vertex positions inside one side (region.CONTOUR_MAX_SPLITS)
constexpr int kMaxLeaving = topo::kMaxWedges; // boundary pieces that may leave one point
// TGNN_CONTOUR_ERR_* (include/tgnn.h)
constexpr int kErrIndex = 1, kErrWedges = 2, kErrSplits = 4, kErrCapacity = 8, kErrTrace = 16;

struct Splits {
    double along[kMaxSplits];                // (p - a) . (b - a), ascending
    int32_t src[kMaxSplits];                 // the canonical vertex of the split
    int n;
};

struct Leaving {
    int32_t piece[kMaxLeaving];
    double dx[kMaxLeaving], dy[kMaxLeaving];
    int n;
};

// The pieces of one mask (caller's storage, `cap` entries each).
struct Pieces {
    int32_t *tile;                           // the tile the piece belongs to
    int32_t *side;                           // index into ring_xy of the side's first vertex
    int32_t *src;                            // canonical vertex of the start point
    int32_t *end;                            // canonical vertex of the end point
};

// One entry of tile i's contact row; false (and kErrIndex) when it is out of range, false for i itself and for a dead tile.
TGNN_TOPO_FN bool row_tile(const Tiles &g, const int32_t *alive, int64_t i, int cc, int64_t &j, int &err) {
    j = g.touch_idx[cc];
    if (j < 0 || j >= g.n_tiles) {
        err |= kErrIndex;
        return false;
    }
    return j != i && alive[j] != 0 && g.ring_ptr[j + 1] - g.ring_ptr[j] >= 3;
}

// The canonical vertex of p, a point of tile i's ring: among i and the alive tiles of its contact row.
TGNN_TOPO_FN int32_t canonical_vertex(const Tiles &g, const int32_t *alive, int64_t i, Pt p, int &err) {
    const double tol2 = g.tol * g.tol;
    int32_t best = 0x7fffffff;
    for (int cc = g.touch_ptr[i] - 1; cc < g.touch_ptr[i + 1]; ++cc) {
        int64_t j = i;                                       // (the first round is tile i itself)
        if (cc >= g.touch_ptr[i] && !row_tile(g, alive, i, cc, j, err)) continue;
        for (int32_t w = g.ring_ptr[j]; w < g.ring_ptr[j + 1]; ++w) {
            const double rx = g.ring_xy[w].x - p.x, ry = g.ring_xy[w].y - p.y;
            if (rx * rx + ry * ry <= tol2 && w < best) best = w;
        }
    }
    return best;
}

// The splits of the side a -> b of tile i.
TGNN_TOPO_FN void side_splits(const Tiles &g, const int32_t *alive, int64_t i, Pt a, Pt b, Splits &out, int &err) {
    const double tol2 = g.tol * g.tol, ex = b.x - a.x, ey = b.y - a.y, ee = ex * ex + ey * ey;
    out.n = 0;
    for (int cc = g.touch_ptr[i]; cc < g.touch_ptr[i + 1]; ++cc) {
        int64_t j;
        if (!row_tile(g, alive, i, cc, j, err)) continue;
        for (int32_t w = g.ring_ptr[j]; w < g.ring_ptr[j + 1]; ++w) {
            const Pt p = g.ring_xy[w];
            const double rx = p.x - a.x, ry = p.y - a.y, sx = p.x - b.x, sy = p.y - b.y;
            const double along = rx * ex + ry * ey, across = rx * ey - ry * ex;
            if (!(along > 0.0 && along < ee && across * across <= tol2 * ee)) continue;
            if (rx * rx + ry * ry <= tol2 || sx * sx + sy * sy <= tol2) continue;       // at an end of the side: no split
            int q = 0;
            bool known = false;
            for (; q < out.n; ++q) {
                const double d = along - out.along[q];
                if (d * d <= tol2 * ee) {                    // the same position: the lowest vertex names it
                    if (w < out.src[q]) out.src[q] = w;
                    known = true;
                    break;
                }
                if (d < 0.0) break;
            }
            if (known) continue;
            if (out.n == kMaxSplits) {
                err |= kErrSplits;
                continue;
            }
            for (int r = out.n; r > q; --r) {
                out.along[r] = out.along[r - 1];
                out.src[r] = out.src[r - 1];
            }
            out.along[q] = along;
            out.src[q] = w;
            ++out.n;
        }
    }
}

// Directions d and f agree (sign > 0) or oppose (sign < 0) within kAngTol.
TGNN_TOPO_FN bool parallel(double dx, double dy, double fx, double fy, double sign) {
    const double cross = dx * fy - dy * fx, dot = dx * fx + dy * fy;
    return sign * dot > 0.0 && cross * cross <= topo::kAngTol * topo::kAngTol * (dx * dx + dy * dy) * (fx * fx + fy * fy);
}

TGNN_TOPO_FN bool piece_has_twin(const Tiles &g, const int32_t *alive, int64_t i, Pt a, Pt b, int &err) {
    const double tol2 = g.tol * g.tol, dx = b.x - a.x, dy = b.y - a.y, mx = 0.5 * (a.x + b.x), my = 0.5 * (a.y + b.y);
    for (int cc = g.touch_ptr[i]; cc < g.touch_ptr[i + 1]; ++cc) {
        int64_t j;
        if (!row_tile(g, alive, i, cc, j, err)) continue;
        const int32_t w0 = g.ring_ptr[j], w1 = g.ring_ptr[j + 1];
        Pt c = g.ring_xy[w1 - 1];
        for (int32_t w = w0; w < w1; ++w) {                  // the side c -> d that ends in vertex w
            const Pt d = g.ring_xy[w];
            const double fx = d.x - c.x, fy = d.y - c.y, ff = fx * fx + fy * fy, rx = mx - c.x, ry = my - c.y;
            const double along = rx * fx + ry * fy, across = rx * fy - ry * fx;
            if (along > 0.0 && along < ff && across * across <= tol2 * ff && parallel(dx, dy, fx, fy, -1.0)) return true;
            c = d;
        }
    }
    return false;
}

// The boundary pieces of alive tile i in piece order: sink(side, src, end) per kept piece.  `sp` is scratch.
template <class Sink>
TGNN_TOPO_FN void tile_pieces(const Tiles &g, const int32_t *alive, int64_t i, Splits &sp, int &err, Sink &sink) {
    const int32_t v0 = g.ring_ptr[i], n = g.ring_ptr[i + 1] - v0;
    if (n < 3) return;
    const int32_t first = canonical_vertex(g, alive, i, g.ring_xy[v0], err);
    int32_t at = first;
    for (int32_t s = 0; s < n; ++s) {
        const Pt a = g.ring_xy[v0 + s], b = g.ring_xy[s + 1 == n ? v0 : v0 + s + 1];
        const int32_t to = s + 1 == n ? first : canonical_vertex(g, alive, i, b, err);
        side_splits(g, alive, i, a, b, sp, err);
        Pt from = a;
        int32_t from_src = at;
        for (int q = 0; q <= sp.n; ++q) {
            const Pt end = q < sp.n ? g.ring_xy[sp.src[q]] : b;
            const int32_t end_src = q < sp.n ? sp.src[q] : to;
            if (!piece_has_twin(g, alive, i, from, end, err)) sink(v0 + s, from_src, end_src);
            from = end;
            from_src = end_src;
        }
        at = to;
    }
}

// The direction of the side of `tile` that starts in vertex v (an index into ring_xy).
TGNN_TOPO_FN void side_direction(const Tiles &g, int64_t tile, int32_t v, double &dx, double &dy) {
    const int32_t v0 = g.ring_ptr[tile], v1 = g.ring_ptr[tile + 1], w = v + 1 == v1 ? v0 : v + 1;
    dx = g.ring_xy[w].x - g.ring_xy[v].x;
    dy = g.ring_xy[w].y - g.ring_xy[v].y;
}

TGNN_TOPO_FN void add_leaving(Leaving &l, int32_t piece, double dx, double dy, int &err) {
    if (l.n == kMaxLeaving) {
        err |= kErrWedges;
        return;
    }
    l.piece[l.n] = piece;
    l.dx[l.n] = dx;
    l.dy[l.n] = dy;
    ++l.n;
}

// Among the pieces that leave a point, the first counter-clockwise from (bx, by), the reversed direction of the piece that
// arrives: the turn lies in (0, 2 pi].  -1 for an empty list.
TGNN_TOPO_FN int32_t choose_successor(const Leaving &l, double bx, double by) {
    int32_t best = -1;
    double best_turn = 0.0;
    for (int q = 0; q < l.n; ++q) {
        double turn = atan2(bx * l.dy[q] - by * l.dx[q], bx * l.dx[q] + by * l.dy[q]);
        if (turn <= 1e-9) turn += 2.0 * topo::kPi;
        if (best < 0 || turn < best_turn) {
            best = l.piece[q];
            best_turn = turn;
        }
    }
    return best;
}

// The successor of piece e of a mask: first[t] .. first[t + 1] are the pieces of tile t in `pc` (indices within the mask).
// `lv` is scratch.  -1 when no piece leaves e's end point.
TGNN_TOPO_FN int32_t link_piece(const Tiles &g, const int32_t *alive, const int32_t *first, const Pieces &pc, int32_t e,
                                Leaving &lv, int &err) {
    const int64_t i = pc.tile[e];
    const int32_t p = pc.end[e];
    lv.n = 0;
    for (int cc = g.touch_ptr[i] - 1; cc < g.touch_ptr[i + 1]; ++cc) {
        int64_t j = i;
        if (cc >= g.touch_ptr[i] && !row_tile(g, alive, i, cc, j, err)) continue;
        for (int32_t f = first[j]; f < first[j + 1]; ++f) {
            if (pc.src[f] != p) continue;
            double dx, dy;
            side_direction(g, j, pc.side[f], dx, dy);
            add_leaving(lv, f, dx, dy, err);
        }
    }
    double dx, dy;
    side_direction(g, i, pc.side[e], dx, dy);
    return choose_successor(lv, -dx, -dy);
}

// The point between piece e and its successor f is a corner (kept) unless the two run the same way.
TGNN_TOPO_FN bool is_corner(const Tiles &g, const Pieces &pc, int32_t e, int32_t f) {
    double dx, dy, fx, fy;
    side_direction(g, pc.tile[e], pc.side[e], dx, dy);
    side_direction(g, pc.tile[f], pc.side[f], fx, fy);
    return !parallel(dx, dy, fx, fy, 1.0);
}

}  // namespace contour
}  // namespace tgnn
#endif
