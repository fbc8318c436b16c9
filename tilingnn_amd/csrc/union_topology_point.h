// The local term of csrc/union_topology.hip: what one vertex of one alive tile adds to the Euler characteristic of the closed
// union of a mask's tiles.  Plain C++ on purpose (no HIP header, no global state): the kernel calls it per (mask, tile, vertex),
// and a host program calls the very same code (tests/host/union_topology_point_test.cpp, under AddressSanitizer and UBSan).
//
// chi = sum over the distinct vertex positions p of (1 - m(p)), m(p) = the number of arcs in which a small circle around p meets
// the union strictly BELOW p (discrete Morse theory; height = the coordinate across the level lines of direction theta).  Every
// tile that touches p adds a wedge of directions: at its vertex from the outgoing side counter-clockwise to the reversed incoming
// side, inside one of its sides the half-plane to the side's left.  No side lies along a level line (the host picks theta so), so
// a wedge meets the open lower half-circle in at most two arcs with ends well inside it.  Arcs of different tiles that meet within
// kAngTol are one arc (two tiles sharing a side); tiles that do not overlap never do more than meet.
#ifndef TGNN_UNION_TOPOLOGY_POINT_H
#define TGNN_UNION_TOPOLOGY_POINT_H
#include <math.h>
#include <stdint.h>

#if defined(__HIPCC__)
#define TGNN_TOPO_FN __host__ __device__ __forceinline__
#else
#define TGNN_TOPO_FN inline
#endif

namespace tgnn {
namespace topo {

constexpr int kMaxWedges = 16;               // tiles that may meet in one point, and arcs kept below it; more: error, not a guess
constexpr double kAngTol = 1e-5;             // arcs whose ends meet within this are one (tilingnn_amd.tiling.region.SWEEP_ANGLE_TOL)
constexpr double kPi = 3.14159265358979323846;
constexpr int kErrIndex = 1, kErrWedges = 2; // TGNN_TOPO_ERR_INDEX, TGNN_TOPO_ERR_WEDGES (include/tgnn.h)

struct Pt {
    double x, y;
};

struct Tiles {
    const Pt *ring_xy;                       // [n_pts]
    const int32_t *ring_ptr;                 // [n_tiles + 1]
    int64_t n_tiles;
    const int32_t *touch_ptr;                // [n_tiles + 1]
    const int32_t *touch_idx;
    double tol, dir_x, dir_y;                // (dir_x, dir_y) = (cos theta, sin theta)
};

// The direction (dx, dy) as an angle in [0, 2 pi) counted counter-clockwise from theta + pi: the lower half-circle is (0, pi).
TGNN_TOPO_FN double lower_angle(const Tiles &g, double dx, double dy) {
    const double a = atan2(g.dir_x * dy - g.dir_y * dx, g.dir_x * dx + g.dir_y * dy) + kPi;
    return a >= 2.0 * kPi ? a - 2.0 * kPi : a;
}

// Arcs: lo(q), hi(q) give references to slot q of the caller's storage (LDS in the kernel), kMaxWedges slots.
template <class Arcs>
TGNN_TOPO_FN void add_wedge(Arcs &arcs, int &cnt, int &err, double from, double to) {
    double span = to - from;
    if (span <= 0.0) span += 2.0 * kPi;
    const double end = from + span;
    if (from < kPi) {
        if (cnt == kMaxWedges) {
            err |= kErrWedges;
        } else {
            arcs.lo(cnt) = from;
            arcs.hi(cnt) = end < kPi ? end : kPi;
            ++cnt;
        }
    }
    if (end > 2.0 * kPi) {                   // a wedge that comes round again
        if (cnt == kMaxWedges) {
            err |= kErrWedges;
        } else {
            arcs.lo(cnt) = 0.0;
            arcs.hi(cnt) = end - 2.0 * kPi < kPi ? end - 2.0 * kPi : kPi;
            ++cnt;
        }
    }
}

// The wedge of ring r[0 .. m) at its vertex w.
template <class Arcs>
TGNN_TOPO_FN void add_vertex_wedge(const Tiles &g, Arcs &arcs, int &cnt, int &err, const Pt *r, int m, int w) {
    const Pt p = r[w], nx = r[w + 1 == m ? 0 : w + 1], pv = r[w == 0 ? m - 1 : w - 1];
    add_wedge(arcs, cnt, err, lower_angle(g, nx.x - p.x, nx.y - p.y), lower_angle(g, pv.x - p.x, pv.y - p.y));
}

// 1 - m(p) for vertex v of alive tile i of the mask `alive` [n_tiles]; 0 when another tile owns the point (the lowest-numbered
// alive tile with a vertex within tol of it does).  err gets kErr* bits OR-ed in.  kExtra: tile `extra` counts as alive too,
// for the alive test and for the owner rule alike (union_hole_delta_point.h: the mask with one candidate added); without it
// `extra` is not looked at and the code is the one point_term always was.
template <bool kExtra, class Arcs>
TGNN_TOPO_FN int point_term_with(const Tiles &g, const int32_t *alive, int64_t extra, int64_t i, int v, Arcs &arcs, int &err) {
    const int v0 = g.ring_ptr[i], n = g.ring_ptr[i + 1] - v0;
    const Pt p = g.ring_xy[v0 + v];
    const double tol2 = g.tol * g.tol;
    int cnt = 0, wedges = 1;
    add_vertex_wedge(g, arcs, cnt, err, g.ring_xy + v0, n, v);
    for (int cc = g.touch_ptr[i]; cc < g.touch_ptr[i + 1]; ++cc) {
        const int64_t j = g.touch_idx[cc];
        if (j < 0 || j >= g.n_tiles) {
            err |= kErrIndex;
            continue;
        }
        if (j == i || (alive[j] == 0 && !(kExtra && j == extra))) continue;
        const int w0 = g.ring_ptr[j], m = g.ring_ptr[j + 1] - w0;
        if (m < 3) continue;
        const Pt *r = g.ring_xy + w0;
        int at_vertex = -1, on_side = -1;
        // within tol of a vertex of j, or of the inside of a side (no division: |cross| <= tol |side|, foot between the ends;
        // near an end the vertex test decides)
        Pt a = r[0];
        for (int w = 0; w < m; ++w) {
            const Pt b = r[w + 1 == m ? 0 : w + 1];
            const double rx = p.x - a.x, ry = p.y - a.y, ex = b.x - a.x, ey = b.y - a.y;
            const double ee = ex * ex + ey * ey, along = rx * ex + ry * ey, across = rx * ey - ry * ex;
            if (rx * rx + ry * ry <= tol2 && at_vertex < 0) at_vertex = w;
            if (on_side < 0 && along > 0.0 && along < ee && across * across <= tol2 * ee) on_side = w;
            a = b;
        }
        if (at_vertex < 0 && on_side < 0) continue;          // j touches i elsewhere
        if (at_vertex >= 0 && j < i) return 0;               // j counts this point
        if (++wedges > kMaxWedges) {
            err |= kErrWedges;
            continue;
        }
        if (at_vertex >= 0) {
            add_vertex_wedge(g, arcs, cnt, err, r, m, at_vertex);
        } else {
            const Pt s0 = r[on_side], s1 = r[on_side + 1 == m ? 0 : on_side + 1];
            add_wedge(arcs, cnt, err, lower_angle(g, s1.x - s0.x, s1.y - s0.y), lower_angle(g, s0.x - s1.x, s0.y - s1.y));
        }
    }
    // arcs after merging = arcs whose start no earlier arc reaches
    int merged = 0;
    for (int q = 0; q < cnt; ++q) {
        const double lq = arcs.lo(q);
        bool reached = false;
        for (int r = 0; r < cnt; ++r) {
            const double lr = arcs.lo(r);
            if (r != q && (lr < lq || (lr == lq && r < q)) && arcs.hi(r) >= lq - kAngTol) reached = true;
        }
        merged += reached ? 0 : 1;
    }
    return 1 - merged;
}

template <class Arcs>
TGNN_TOPO_FN int point_term(const Tiles &g, const int32_t *alive, int64_t i, int v, Arcs &arcs, int &err) {
    return point_term_with<false>(g, alive, -1, i, v, arcs, err);
}

}  // namespace topo
}  // namespace tgnn
#endif
