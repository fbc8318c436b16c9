// Which tiles of the complete graph lie inside a target region: the reference's `contain` predicate
// (util/algo_util.py:143-144, evaluated per tile by tile_factory.get_all_placement_in_polygon, tile_factory.py:39)
//     abs(region.intersection(tile).area - tile.area) < 1e-6
// for K regions x all tiles in one launch, in fp64.
//
// Inputs (built by tilingnn_amd/tiling/region.py and util/data_util.py: CompleteGraphOnDevice):
//   tiles    every tile's ring ear-clipped into counter-clockwise triangles, a tile -> triangle range, the tile's bounding
//            box, a point strictly inside it and area(T) as GEOS computes it (tile_graph.ring_area, bit for bit what the
//            reference compares against);
//   regions  rings (not closed), exterior counter-clockwise, holes clockwise, a region -> ring range and the region's box.
//
// Per (region, tile) pair:
//   (0) tile box disjoint from the region box: outside, area 0.
//   (a) no region edge's box meets the tile's box: the tile is entirely inside or entirely outside; the winding number of its
//       inside point decides, no area is computed (area = area(T) or 0).
//   (b) otherwise area(R n T) = sum over tile triangles t, over region edges (p, q) of  sigma * area(tri(O, p, q) n t),
//       sigma = the orientation of (O, p, q): the fan of signed triangles from any point O integrates the winding number.
//       Each term is a convex-convex clip done in registers (t clipped by the three edges of the fan triangle,
//       Sutherland-Hodgman, then the shoelace) and is bounded by area(t), so the rounding of the sum stays near
//       n_terms * area(t) * 1e-16, far below the 1e-6 threshold.  Near-coincident edges (the complete graphs place shared
//       vertices ~1e-12 apart) cost a sliver of their offset, not more: every clipped vertex stays on t's boundary.  O sits at the tile's height, beyond the region's box on the
//       nearer side: a fan triangle meets the tile only when its edge crosses the horizontal band of the tile between O and
//       the tile, so most terms are culled by a separating-axis test against the tile's box.  Coordinates are taken relative
//       to the tile's centre.
// G lanes work on one pair: they stride over the region's edges and reduce in a fixed butterfly, so the result has the same
// bits from run to run.  G = 8 for regions of a few dozen edges (random stars), 64 (one wave per pair) for silhouettes.
#include "tgnn_common.h"

// No fused multiply-add contraction here: a region edge that IS a tile edge must give exactly 0 in the side tests of the clip,
// and a*b - c*d contracted into fma(a, b, -c*d) leaves the rounding error of c*d where the two products are equal.
#pragma clang fp contract(off)

namespace tgnn {

constexpr int kRgThreads = 256;
constexpr double kContainEps = 1e-6;         // util/algo_util.py:144, strict `<`

struct RegionArgs {
    const double2 *tri;                      // [n_tri][3] counter-clockwise
    const int32_t *tile_tri_ptr;             // [n_tiles + 1]
    const double4 *tile_bbox;                // [n_tiles] xmin ymin xmax ymax
    const double *tile_area;                 // [n_tiles]
    const double2 *tile_point;               // [n_tiles]
    int64_t n_tiles;
    const double2 *ring_xy;                  // [n_pts]
    const int32_t *ring_ptr;                 // [n_rings + 1]
    const int32_t *region_ring_ptr;          // [K + 1]
    const double4 *region_bbox;              // [K]
    int32_t *alive;                          // [K][n_tiles]
    double *area;                            // [K][n_tiles] or NULL
};

__device__ __forceinline__ double cross2(double ax, double ay, double bx, double by) { return ax * by - ay * bx; }

// v[m] = (x, y) for a run-time m, without run-time indexing (which would put the arrays in scratch)
template <int N>
__device__ __forceinline__ void put(double (&vx)[N], double (&vy)[N], int m, double x, double y) {
#pragma unroll
    for (int j = 0; j < N; ++j) {
        vx[j] = j == m ? x : vx[j];
        vy[j] = j == m ? y : vy[j];
    }
}

// Sutherland-Hodgman: the n-gon (ix, iy) clipped to the left of the line u -> u + e; returns the new vertex count (<= n + 1).
// A vertex ON the line counts as inside.  Each output vertex lies on the input polygon's boundary, so a sign that rounding
// gets wrong for a vertex within rounding of the line moves the result by a sliver of that width, never more.
template <int NI, int NO>
__device__ __forceinline__ int clip_half_plane(const double (&ix)[NI], const double (&iy)[NI], int n, double (&ox)[NO],
                                               double (&oy)[NO], double ux, double uy, double ex, double ey) {
    double px = ix[0], py = iy[0];
#pragma unroll
    for (int j = 1; j < NI; ++j) {
        px = j == n - 1 ? ix[j] : px;
        py = j == n - 1 ? iy[j] : py;
    }
    double fp = cross2(ex, ey, px - ux, py - uy);
    int m = 0;
#pragma unroll
    for (int i = 0; i < NI; ++i) {
        if (i < n) {
            const double cx = ix[i], cy = iy[i];
            const double fc = cross2(ex, ey, cx - ux, cy - uy);
            if ((fp >= 0.0) != (fc >= 0.0)) {
                const double s = fp / (fp - fc);
                put(ox, oy, m, px + s * (cx - px), py + s * (cy - py));
                ++m;
            }
            if (fc >= 0.0) {
                put(ox, oy, m, cx, cy);
                ++m;
            }
            px = cx;
            py = cy;
            fp = fc;
        }
    }
    return m;
}

// area(t n T) of two counter-clockwise triangles: t clipped by T's three edges (3 -> 4 -> 5 -> 6 vertices at most), shoelace
__device__ __forceinline__ double tri_tri_area(const double (&t)[6], const double (&T)[6]) {
    double ax[3] = {t[0], t[2], t[4]}, ay[3] = {t[1], t[3], t[5]};
    double bx[4] = {}, by[4] = {}, cx[5] = {}, cy[5] = {}, dx[6] = {}, dy[6] = {};
    int n = clip_half_plane(ax, ay, 3, bx, by, T[0], T[1], T[2] - T[0], T[3] - T[1]);
    if (n < 3) return 0.0;
    n = clip_half_plane(bx, by, n, cx, cy, T[2], T[3], T[4] - T[2], T[5] - T[3]);
    if (n < 3) return 0.0;
    n = clip_half_plane(cx, cy, n, dx, dy, T[4], T[5], T[0] - T[4], T[1] - T[5]);
    if (n < 3) return 0.0;
    double s = 0.0, lx = dx[0], ly = dy[0];
#pragma unroll
    for (int i = 0; i < 5; ++i) {
        if (i + 1 < n) s += cross2(dx[i], dy[i], dx[i + 1], dy[i + 1]);
        lx = i + 1 == n - 1 ? dx[i + 1] : lx;
        ly = i + 1 == n - 1 ? dy[i + 1] : ly;
    }
    s += cross2(lx, ly, dx[0], dy[0]);
    return 0.5 * s;
}

// false when the counter-clockwise triangle T is separated from the box [x0, x1] x [y0, y1]
__device__ __forceinline__ bool tri_meets_box(const double (&T)[6], double x0, double y0, double x1, double y1) {
    if (fmax(T[0], fmax(T[2], T[4])) < x0 || fmin(T[0], fmin(T[2], T[4])) > x1 ||
        fmax(T[1], fmax(T[3], T[5])) < y0 || fmin(T[1], fmin(T[3], T[5])) > y1) return false;
#pragma unroll
    for (int i = 0; i < 3; ++i) {
        const double ux = T[2 * i], uy = T[2 * i + 1];
        const double ex = T[(2 * i + 2) % 6] - ux, ey = T[(2 * i + 3) % 6] - uy;
        // the box corner furthest on the inner (left) side of edge e
        const double cx = ey > 0.0 ? x0 : x1, cy = ex > 0.0 ? y1 : y0;
        if (cross2(ex, ey, cx - ux, cy - uy) < 0.0) return false;
    }
    return true;
}

template <int G, typename T>
__device__ __forceinline__ T group_sum(T v) {
#pragma unroll
    for (int d = G / 2; d >= 1; d >>= 1) v += __shfl_xor(v, d, G);
    return v;
}

template <int G>
__global__ __launch_bounds__(kRgThreads) void tiles_in_region_kernel(RegionArgs a, int64_t region0) {
    constexpr int kPairs = kRgThreads / G;
    const int lane = threadIdx.x % G;
    const int64_t tile = (int64_t)blockIdx.x * kPairs + threadIdx.x / G;
    const int64_t k = region0 + blockIdx.y;
    if (tile >= a.n_tiles) return;           // the whole group leaves together
    const double4 tb = a.tile_bbox[tile];
    const double4 rb = a.region_bbox[k];
    const double t_area = a.tile_area[tile];
    double area = 0.0;
    if (!(tb.x > rb.z || tb.z < rb.x || tb.y > rb.w || tb.w < rb.y)) {
        const double cx = 0.5 * (tb.x + tb.z), cy = 0.5 * (tb.y + tb.w);
        // tile box relative to the centre, widened so that (a) never decides a tile that an edge comes within rounding of
        const double tol = 1e-9 * (1.0 + fmax(fmax(fabs(tb.x), fabs(tb.z)), fmax(fabs(tb.y), fabs(tb.w))));
        const double bx0 = tb.x - cx, by0 = tb.y - cy, bx1 = tb.z - cx, by1 = tb.w - cy;
        const double2 pt = a.tile_point[tile];
        const double px = pt.x - cx, py = pt.y - cy;
        const int r0 = a.region_ring_ptr[k], r1 = a.region_ring_ptr[k + 1];
        int touch = 0, wn = 0;
        for (int r = r0; r < r1; ++r) {
            const int v0 = a.ring_ptr[r], n = a.ring_ptr[r + 1] - v0;
            for (int e = lane; e < n; e += G) {
                const double2 P = a.ring_xy[v0 + e], Q = a.ring_xy[v0 + (e + 1 == n ? 0 : e + 1)];
                const double ax = P.x - cx, ay = P.y - cy, qx = Q.x - cx, qy = Q.y - cy;
                if (!(fmax(ax, qx) < bx0 - tol || fmin(ax, qx) > bx1 + tol || fmax(ay, qy) < by0 - tol || fmin(ay, qy) > by1 + tol))
                    touch = 1;
                const double side = cross2(qx - ax, qy - ay, px - ax, py - ay);
                if (ay <= py) {
                    if (qy > py && side > 0.0) ++wn;
                } else if (qy <= py && side < 0.0) {
                    --wn;
                }
            }
        }
        touch = group_sum<G>(touch);
        if (!touch) {
            area = group_sum<G>(wn) != 0 ? t_area : 0.0;
        } else {
            // O: beyond the region's box on the side nearer to the tile, at the tile's height
            const double span = (rb.z - rb.x) + (rb.w - rb.y) + 1.0;
            const double ox = (cx - rb.x <= rb.z - cx) ? (rb.x - span) - cx : (rb.z + span) - cx, oy = 0.0;
            const int t0 = a.tile_tri_ptr[tile], t1 = a.tile_tri_ptr[tile + 1];
            double acc = 0.0;
            for (int r = r0; r < r1; ++r) {
                const int v0 = a.ring_ptr[r], n = a.ring_ptr[r + 1] - v0;
                for (int e = lane; e < n; e += G) {
                    const double2 P = a.ring_xy[v0 + e], Q = a.ring_xy[v0 + (e + 1 == n ? 0 : e + 1)];
                    const double ax = P.x - cx, ay = P.y - cy, qx = Q.x - cx, qy = Q.y - cy;
                    const double orient = cross2(ax - ox, ay - oy, qx - ox, qy - oy);
                    if (orient == 0.0) continue;
                    double T[6] = {ox, oy, ax, ay, qx, qy};
                    if (orient < 0.0) {
                        T[2] = qx; T[3] = qy; T[4] = ax; T[5] = ay;
                    }
                    if (!tri_meets_box(T, bx0, by0, bx1, by1)) continue;
                    double term = 0.0;
                    for (int j = t0; j < t1; ++j) {
                        const double2 u0 = a.tri[3 * j], u1 = a.tri[3 * j + 1], u2 = a.tri[3 * j + 2];
                        const double t[6] = {u0.x - cx, u0.y - cy, u1.x - cx, u1.y - cy, u2.x - cx, u2.y - cy};
                        term += tri_tri_area(t, T);
                    }
                    acc += orient > 0.0 ? term : -term;
                }
            }
            area = group_sum<G>(acc);
        }
    }
    if (lane == 0) {
        const int64_t o = k * a.n_tiles + tile;
        a.alive[o] = fabs(area - t_area) < kContainEps ? 1 : 0;
        if (a.area) a.area[o] = area;
    }
}

// counts[k] = {collision edges, adjacency edges} with both ends alive in region k
__global__ __launch_bounds__(kRgThreads) void region_edge_count_kernel(const int32_t *__restrict__ alive, int64_t n_tiles,
                                                                       const int64_t *__restrict__ col, int64_t n_col,
                                                                       const int64_t *__restrict__ adj, int64_t n_adj,
                                                                       int64_t region0, unsigned long long *__restrict__ counts,
                                                                       int32_t *__restrict__ err_flag) {
    __shared__ unsigned long long part[kRgThreads / kWave][2];
    const int64_t k = region0 + blockIdx.y;
    const int32_t *al = alive + k * n_tiles;
    unsigned long long c[2] = {0ull, 0ull};
    for (int set = 0; set < 2; ++set) {
        const int64_t *ei = set == 0 ? col : adj;
        const int64_t ne = set == 0 ? n_col : n_adj;
        for (int64_t i = (int64_t)blockIdx.x * kRgThreads + threadIdx.x; i < ne; i += (int64_t)gridDim.x * kRgThreads) {
            const int64_t u = ei[i], v = ei[ne + i];
            if (u < 0 || u >= n_tiles || v < 0 || v >= n_tiles) {
                if (err_flag) *err_flag = 1;
                continue;
            }
            c[set] += (al[u] != 0 && al[v] != 0) ? 1ull : 0ull;
        }
    }
    for (int set = 0; set < 2; ++set) {
        unsigned long long v = c[set];
        for (int d = kWave / 2; d >= 1; d >>= 1) v += __shfl_xor(v, d);
        if (threadIdx.x % kWave == 0) part[threadIdx.x / kWave][set] = v;
    }
    __syncthreads();
    if (threadIdx.x < 2) {
        unsigned long long v = 0;
        for (int w = 0; w < kRgThreads / kWave; ++w) v += part[w][threadIdx.x];
        if (v) atomicAdd(counts + 2 * k + threadIdx.x, v);
    }
}

}  // namespace tgnn

using namespace tgnn;

static constexpr int64_t kMaxGridY = 65535;

extern "C" int tgnn_tiles_in_region(const double *tri_xy, const int32_t *tile_tri_ptr, const double *tile_bbox,
                                    const double *tile_area, const double *tile_point, int64_t n_tiles, const double *ring_xy,
                                    const int32_t *ring_ptr, const int32_t *region_ring_ptr, const double *region_bbox,
                                    int64_t n_regions, int32_t max_region_edges, int32_t *alive_out, double *area_out,
                                    tgnn_stream_t stream) {
    DeviceGuard guard__(stream);
    TGNN_CHECK_ARG(n_tiles >= 0 && n_tiles < (1ll << 31) - 1 && n_regions >= 0, "shape");
    TGNN_CHECK_ARG(max_region_edges >= 0, "max_region_edges");
    if (n_tiles == 0 || n_regions == 0) return TGNN_OK;
    TGNN_CHECK_ARG(n_regions * n_tiles < (1ll << 62), "K * n_tiles overflows");
    TGNN_CHECK_ARG(tri_xy && tile_tri_ptr && tile_bbox && tile_area && tile_point, "null tile array");
    TGNN_CHECK_ARG(ring_xy && ring_ptr && region_ring_ptr && region_bbox && alive_out, "null region array");
    hipStream_t s = static_cast<hipStream_t>(stream);
    RegionArgs a{reinterpret_cast<const double2 *>(tri_xy), tile_tri_ptr, reinterpret_cast<const double4 *>(tile_bbox),
                 tile_area, reinterpret_cast<const double2 *>(tile_point), n_tiles,
                 reinterpret_cast<const double2 *>(ring_xy), ring_ptr, region_ring_ptr,
                 reinterpret_cast<const double4 *>(region_bbox), alive_out, area_out};
    const bool wide = max_region_edges > 48;
    const int pairs = kRgThreads / (wide ? kWave : 8);
    const unsigned gx = (unsigned)((n_tiles + pairs - 1) / pairs);
    for (int64_t k0 = 0; k0 < n_regions; k0 += kMaxGridY) {
        const unsigned gy = (unsigned)(n_regions - k0 < kMaxGridY ? n_regions - k0 : kMaxGridY);
        if (wide)
            tiles_in_region_kernel<kWave><<<dim3(gx, gy), kRgThreads, 0, s>>>(a, k0);
        else
            tiles_in_region_kernel<8><<<dim3(gx, gy), kRgThreads, 0, s>>>(a, k0);
    }
    TGNN_CHECK_LAUNCH();
    return TGNN_OK;
}

extern "C" int tgnn_region_edge_counts(const int32_t *alive, int64_t n_regions, int64_t n_tiles, const int64_t *col_edge_index,
                                       int64_t n_col_edges, const int64_t *adj_edge_index, int64_t n_adj_edges,
                                       int64_t *counts_out, int32_t *err_flag, tgnn_stream_t stream) {
    DeviceGuard guard__(stream);
    TGNN_CHECK_ARG(n_regions >= 0 && n_tiles >= 0 && n_col_edges >= 0 && n_adj_edges >= 0, "shape");
    if (n_regions == 0) return TGNN_OK;
    TGNN_CHECK_ARG(counts_out, "null counts_out");
    TGNN_CHECK_ARG(n_tiles == 0 || alive, "null alive");
    TGNN_CHECK_ARG(n_col_edges == 0 || col_edge_index, "null collision edges");
    TGNN_CHECK_ARG(n_adj_edges == 0 || adj_edge_index, "null adjacency edges");
    hipStream_t s = static_cast<hipStream_t>(stream);
    TGNN_CHECK_HIP(hipMemsetAsync(counts_out, 0, sizeof(int64_t) * 2 * n_regions, s));
    const int64_t m = n_col_edges > n_adj_edges ? n_col_edges : n_adj_edges;
    if (n_tiles == 0 || m == 0) return TGNN_OK;
    int64_t gx = (m + kRgThreads - 1) / kRgThreads;
    gx = gx > 16 ? 16 : gx;
    for (int64_t k0 = 0; k0 < n_regions; k0 += kMaxGridY) {
        const unsigned gy = (unsigned)(n_regions - k0 < kMaxGridY ? n_regions - k0 : kMaxGridY);
        region_edge_count_kernel<<<dim3((unsigned)gx, gy), kRgThreads, 0, s>>>(
            alive, n_tiles, col_edge_index, n_col_edges, adj_edge_index, n_adj_edges, k0,
            reinterpret_cast<unsigned long long *>(counts_out), err_flag);
    }
    TGNN_CHECK_LAUNCH();
    return TGNN_OK;
}
