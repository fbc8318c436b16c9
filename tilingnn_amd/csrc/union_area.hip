// Area of the union of a set of overlapping tiles -- the reference's `BrickLayout.get_super_contour_poly().area`
// (tiling/brick_layout.py:180-188, a shapely unary_union) -- for K tile masks of the complete graph in one call, in fp64.
//
// Inputs (built by tilingnn_amd/tiling/region.py: union_geometry, uploaded by util/data_util.py: CompleteGraphOnDevice):
//   tiles     every tile's ring, open and counter-clockwise, and a tile -> vertex range;
//   collide   the complete graph's collision edges as CSR (row i = the tiles that collide with tile i);
//   alive     [K][n_tiles] int32, != 0 = the tile belongs to mask k (what tgnn_tiles_in_region writes; any 0/1 mask).
//
// Formulation: a boundary integral.  By Green's theorem the union's area is the sum over every edge a -> b of every alive
// tile of 1/2 cross(a, b) x (the share of the edge that lies on the union's boundary).  A point of edge e of tile i is NOT on
// that boundary when it is strictly inside another alive tile j, or when it lies on a side of an alive j < i that runs in the
// SAME direction (two overlapping tiles sharing a side: the lower number keeps it).  On a side of j that runs the OPPOSITE way
// (two tiles touching from either side) both keep their piece and the two terms cancel.  Only collision neighbours can cover
// anything -- overlapping in area, or sharing a side from the same side, is colliding -- so j runs over row i of the CSR.
//
// Per (i, e, j) everything happens in the frame of the edge: t along it (0 .. L), s the signed distance to its line, with
// |s| <= tol SNAPPED to 0 (tol: the radius the reference buffers every tile by, brick_layout.py:185; it separates the
// lattice's noise, ~1e-8, from the smallest real feature, 0.25).  The edge is cut at every snapped vertex of j and wherever a
// side of j crosses s = 0; the midpoint of every piece is classified -- on a collinear side of j (then by that side's
// direction), else by the parity of j's sides above it -- and covered pieces go into a list of disjoint intervals that all
// the j of this edge share.  Nothing of j is stored: its vertices are transformed again in every pass (they sit in L1; a
// ring of m vertices costs O(pieces x m) transforms), so there is no bound on a ring's vertex count or on a tile's degree.
// The interval list is the one bounded thing: kMaxIntervals disjoint covered intervals per edge, in LDS; an edge that needs
// more sets *err_flag (TGNN_UNION_ERR_INTERVALS) and the binding raises -- never a silently wrong area.
//
// Origin.  A gap g between where one tile's piece ends and the next tile's begins (vertices that should coincide and do not)
// costs 1/2 |X| |g| of area, X = the place relative to the integral's origin.  So the origin is taken per MASK, at the first
// vertex of its first alive tile: every tile leaves its integral about its OWN first vertex c_i plus the vector sum V_i of its
// kept pieces, and the fold forms  sum_i A_i + 1/2 cross(c_i - o, V_i)  -- the same integral about o.
//
// Launch shape.  union_area_tiles_kernel: ONE THREAD per (mask, tile), grid (ceil(n_tiles / 256), K).  The work of a mask is
// small (n_tiles x edges x alive neighbours segment clips) and K is large (thousands of crops or candidate selections), so
// the parallelism comes from K x n_tiles threads; a dead tile costs one coalesced 4-byte load and leaves; no cross-lane step,
// so the per-tile sum has one fixed order.  256 threads x kMaxIntervals x 16 B = 32 KB of LDS per block, laid out
// [slot][thread] (conflict free), 5 blocks per CU.  union_area_fold_kernel: one block per mask adds the alive tiles' three
// partials in a fixed order (thread t takes tiles t, t + 256, ...; then a fixed LDS tree): the same bits on every run, no
// floating-point atomics.  The two kernels follow each other on the stream; nothing returns to the host.
#include "union_masks.h"

namespace tgnn {

constexpr int kUaThreads = 256;
constexpr int kMaxIntervals = 8;             // disjoint covered intervals one tile edge can hold (LDS); more: error, not a guess

struct UnionArgs {
    const double2 *ring_xy;                  // [n_pts]
    const int32_t *ring_ptr;                 // [n_tiles + 1]
    int64_t n_tiles;
    const int32_t *col_ptr;                  // [n_tiles + 1]
    const int32_t *col_idx;                  // [col_ptr[n_tiles]]
    const int32_t *alive;                    // [K][n_tiles]
    int64_t n_masks;
    double tol;
    double *part;                            // [3][K][n_tiles]: A_i, V_i.x, V_i.y (alive tiles only)
    double *area_out;                        // [K]
    int32_t *err_flag;
};

struct EdgeFrame {
    double ax, ay, dx, dy, len, tol;         // a, the unit direction, the length
    // (t, s) of the point p: along the edge, and the signed distance to its line (left of a -> b positive), snapped
    __device__ __forceinline__ void loc(const double2 p, double &t, double &s) const {
        const double rx = p.x - ax, ry = p.y - ay;
        t = rx * dx + ry * dy;
        s = dx * ry - dy * rx;
        s = fabs(s) <= tol ? 0.0 : s;
    }
};

// The smallest cut of the edge by ring j[0 .. m) that is > lo (and < len); len when there is none.
__device__ __forceinline__ double next_cut(const EdgeFrame &f, const double2 *__restrict__ j, int m, double lo) {
    double hi = f.len, pt, ps;
    f.loc(j[m - 1], pt, ps);
    for (int v = 0; v < m; ++v) {
        double qt, qs;
        f.loc(j[v], qt, qs);
        if (qs == 0.0 && qt > lo && qt < hi) hi = qt;
        if ((ps < 0.0 && qs > 0.0) || (ps > 0.0 && qs < 0.0)) {
            const double c = pt + (qt - pt) * (ps / (ps - qs));
            if (c > lo && c < hi) hi = c;
        }
        pt = qt;
        ps = qs;
    }
    return hi;
}

// Is the point (tm, 0) of the edge covered by ring j?  lower = j's number is below the edge's tile's.
__device__ __forceinline__ bool covered_at(const EdgeFrame &f, const double2 *__restrict__ j, int m, double tm, bool lower) {
    double pt, ps;
    f.loc(j[m - 1], pt, ps);
    bool on = false, same = false;
    int above = 0;
    for (int v = 0; v < m; ++v) {
        double qt, qs;
        f.loc(j[v], qt, qs);
        if (ps == 0.0 && qs == 0.0) {
            if (pt != qt && fmin(pt, qt) <= tm && tm <= fmax(pt, qt) && !on) {
                on = true;
                same = qt > pt;
            }
        } else if ((pt <= tm) != (qt <= tm)) {
            const double sc = ps + (qs - ps) * ((tm - pt) / (qt - pt));
            above ^= sc > 0.0 ? 1 : 0;
        }
        pt = qt;
        ps = qs;
    }
    return on ? (same && lower) : above != 0;
}

__global__ __launch_bounds__(kUaThreads) void union_area_tiles_kernel(UnionArgs a, int64_t mask0) {
    __shared__ double iv_lo[kMaxIntervals][kUaThreads], iv_hi[kMaxIntervals][kUaThreads];
    const int tid = threadIdx.x;
    const int64_t i = (int64_t)blockIdx.x * kUaThreads + tid;
    const int64_t k = mask0 + blockIdx.y;
    if (i >= a.n_tiles) return;
    const int32_t *al = a.alive + k * a.n_tiles;
    if (al[i] == 0) return;
    const int v0 = a.ring_ptr[i], n = a.ring_ptr[i + 1] - v0;
    const int c0 = a.col_ptr[i], c1 = a.col_ptr[i + 1];
    double acc = 0.0, vx = 0.0, vy = 0.0;
    if (n >= 3) {
        const double2 c = a.ring_xy[v0];
        for (int e = 0; e < n; ++e) {
            const double2 A = a.ring_xy[v0 + e], B = a.ring_xy[v0 + (e + 1 == n ? 0 : e + 1)];
            const double ex = B.x - A.x, ey = B.y - A.y;
            const double len = sqrt(ex * ex + ey * ey);
            if (!(len > 0.0)) continue;
            const EdgeFrame f{A.x, A.y, ex / len, ey / len, len, a.tol};
            int cnt = 0;
            for (int cc = c0; cc < c1; ++cc) {
                const int jn = a.col_idx[cc];
                if (jn < 0 || jn >= a.n_tiles) {
                    atomicOr(a.err_flag, TGNN_UNION_ERR_INDEX);
                    continue;
                }
                if (jn == i || al[jn] == 0) continue;
                const int w0 = a.ring_ptr[jn], m = a.ring_ptr[jn + 1] - w0;
                if (m < 3) continue;
                const double2 *jr = a.ring_xy + w0;
                // j entirely on one side of the line, or beyond the edge's ends: nothing to cover
                double tmin = INFINITY, tmax = -INFINITY, smin = INFINITY, smax = -INFINITY;
                for (int v = 0; v < m; ++v) {
                    double t, s;
                    f.loc(jr[v], t, s);
                    tmin = fmin(tmin, t);
                    tmax = fmax(tmax, t);
                    smin = fmin(smin, s);
                    smax = fmax(smax, s);
                }
                if (smin > 0.0 || smax < 0.0 || tmax <= 0.0 || tmin >= len) continue;
                double lo = 0.0;
                for (int piece = 0; piece <= 2 * m + 1 && lo < len; ++piece) {     // at most 2 m cuts
                    const double hi = next_cut(f, jr, m, lo);
                    if (covered_at(f, jr, m, 0.5 * (lo + hi), jn < i)) {
                        // into the disjoint list: absorb what [lo, hi] touches, then append
                        double nl = lo, nh = hi;
                        for (int q = 0; q < cnt;) {
                            const double ql = iv_lo[q][tid], qh = iv_hi[q][tid];
                            if (ql <= nh && qh >= nl) {
                                nl = fmin(nl, ql);
                                nh = fmax(nh, qh);
                                --cnt;
                                iv_lo[q][tid] = iv_lo[cnt][tid];
                                iv_hi[q][tid] = iv_hi[cnt][tid];
                            } else {
                                ++q;
                            }
                        }
                        if (cnt == kMaxIntervals) {
                            atomicOr(a.err_flag, TGNN_UNION_ERR_INTERVALS);
                        } else {
                            iv_lo[cnt][tid] = nl;
                            iv_hi[cnt][tid] = nh;
                            ++cnt;
                        }
                    }
                    lo = hi;
                }
            }
            double cov = 0.0;
            for (int q = 0; q < cnt; ++q) cov += iv_hi[q][tid] - iv_lo[q][tid];
            const double kept = fmax(len - cov, 0.0);
            acc += 0.5 * ((A.x - c.x) * f.dy - (A.y - c.y) * f.dx) * kept;
            vx += f.dx * kept;
            vy += f.dy * kept;
        }
    }
    const int64_t plane = a.n_masks * a.n_tiles, o = k * a.n_tiles + i;
    a.part[o] = acc;
    a.part[plane + o] = vx;
    a.part[2 * plane + o] = vy;
}

__global__ __launch_bounds__(kUaThreads) void union_area_fold_kernel(UnionArgs a, int64_t mask0) {
    __shared__ double red[kUaThreads];
    __shared__ int first[kUaThreads];
    const int tid = threadIdx.x;
    const int64_t k = mask0 + blockIdx.x;
    const int32_t *al = a.alive + k * a.n_tiles;
    const int n = (int)a.n_tiles;
    int mine = n;
    for (int i = tid; i < n; i += kUaThreads)
        if (al[i] != 0 && a.ring_ptr[i + 1] - a.ring_ptr[i] >= 3) {
            mine = i;
            break;
        }
    first[tid] = mine;
    __syncthreads();
    for (int d = kUaThreads / 2; d >= 1; d >>= 1) {
        if (tid < d) first[tid] = min(first[tid], first[tid + d]);
        __syncthreads();
    }
    const int i0 = first[0];
    if (i0 >= n) {                           // (uniform) an empty mask
        if (tid == 0) a.area_out[k] = 0.0;
        return;
    }
    const double2 org = a.ring_xy[a.ring_ptr[i0]];
    const int64_t plane = a.n_masks * a.n_tiles;
    const double *p0 = a.part + k * a.n_tiles, *p1 = p0 + plane, *p2 = p1 + plane;
    double acc = 0.0;
    for (int i = tid; i < n; i += kUaThreads) {
        if (al[i] == 0) continue;
        const int v0 = a.ring_ptr[i];
        if (a.ring_ptr[i + 1] - v0 < 3) continue;
        const double2 c = a.ring_xy[v0];
        acc += p0[i] + 0.5 * ((c.x - org.x) * p2[i] - (c.y - org.y) * p1[i]);
    }
    red[tid] = acc;
    __syncthreads();
    for (int d = kUaThreads / 2; d >= 1; d >>= 1) {
        if (tid < d) red[tid] += red[tid + d];
        __syncthreads();
    }
    if (tid == 0) a.area_out[k] = red[0];
}

}  // namespace tgnn

using namespace tgnn;

extern "C" size_t tgnn_union_area_workspace_bytes(int64_t n_masks, int64_t n_tiles) {
    if (n_masks <= 0 || n_tiles <= 0 || n_masks > (1ll << 58) / n_tiles) return 0;
    return (size_t)3 * (size_t)n_masks * (size_t)n_tiles * sizeof(double);
}

extern "C" int tgnn_union_area(const double *ring_xy, const int32_t *ring_ptr, int64_t n_tiles, const int32_t *col_ptr,
                               const int32_t *col_idx, const int32_t *alive, int64_t n_masks, double tol, double *area_out,
                               int32_t *err_flag, void *ws, size_t ws_bytes, tgnn_stream_t stream) {
    DeviceGuard guard__(stream);
    if (int rc = check_mask_shape(__func__, n_tiles, n_masks, tol, 1.0, 0.0)) return rc;
    if (n_masks == 0) return TGNN_OK;
    TGNN_CHECK_ARG(area_out && err_flag, "null area_out / err_flag");
    hipStream_t s = static_cast<hipStream_t>(stream);
    if (n_tiles == 0) {
        TGNN_CHECK_HIP(hipMemsetAsync(area_out, 0, sizeof(double) * n_masks, s));
        return TGNN_OK;
    }
    if (int rc = check_mask_arrays(__func__, n_masks, (1ll << 58) / n_tiles, ring_xy && ring_ptr && col_ptr && alive, ws, ws_bytes,
                                   tgnn_union_area_workspace_bytes(n_masks, n_tiles), sizeof(double)))
        return rc;
    UnionArgs a{reinterpret_cast<const double2 *>(ring_xy), ring_ptr, n_tiles, col_ptr, col_idx, alive, n_masks, tol,
                static_cast<double *>(ws), area_out, err_flag};
    const unsigned gx = (unsigned)((n_tiles + kUaThreads - 1) / kUaThreads);
    for_mask_chunks(n_masks, kMaskGridY, [&](int64_t k0, unsigned gy) {
        union_area_tiles_kernel<<<dim3(gx, gy), kUaThreads, 0, s>>>(a, k0);
    });
    for_mask_chunks(n_masks, kMaskGridX, [&](int64_t k0, unsigned g) { union_area_fold_kernel<<<g, kUaThreads, 0, s>>>(a, k0); });
    TGNN_CHECK_LAUNCH();
    return TGNN_OK;
}
