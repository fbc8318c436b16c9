// The outline of the union of a set of tiles that do not overlap -- what the reference's
// `BrickLayout.get_selected_tiles_union_polygon` (tiling/brick_layout.py:223-227) returns for a solved layout -- for K tile masks
// of the complete graph in one call: per mask the boundary rings of the CLOSED union of the alive tiles, one counter-clockwise
// ring per connected component (tiles sharing any point, a single corner included, are connected) and one clockwise ring per
// bounded component of the complement.  Inputs are those of csrc/union_topology.hip; the semantics (pieces, successor, leaders,
// dropped straight-through points, canonical vertices) are DESIGN section 38 and union_contour_piece.h.
//
// Launches, all on the caller's stream, nothing returns to the host:
//   union_contour_prep_kernel     one block per mask.  One thread per alive tile (listed in LDS first, a chunk of tiles at a
//                                 time): the collision row (status 1 when two alive tiles collide), the number of boundary
//                                 pieces of the tile (union_contour_piece.h: tile_pieces); an exclusive block scan in tile
//                                 order gives every tile its first piece, so piece indices do not depend on scheduling; the
//                                 component labels by label_components of union_masks.h, in the workspace.
//   union_contour_offsets_kernel  one block: exclusive scan of the K piece counts (int64), where each mask's pieces live.
//   union_contour_trace_kernel    one block per mask.  Fill (a thread per tile writes its pieces), link (a thread per piece
//                                 writes its successor), a check that the successor relation is a permutation (in-degrees, integer
//                                 atomics), every cycle's leader by min-propagation with pointer doubling, ceil(log2 pieces) + 1
//                                 rounds, the corner flags, corners per ring (integer atomics on the leader's word) and two block
//                                 scans in piece order: the ring table of the mask in ascending leader order.  The four working
//                                 arrays live in LDS for masks of up to kLdsPieces pieces (48 KB) and in the workspace beyond.
//   union_contour_finish_kernel   one block: exclusive scans of the K ring and point counts, mask_out, total_out, CAPACITY.
//   union_contour_emit_kernel     one block per mask, one thread per ring: walks the ring from its leader (at most `pieces`
//                                 steps), writes the surviving points, and sums the fp64 shoelace about the ring's first point in
//                                 listed order: no floating-point atomics anywhere, the same bits on every call.
#include "union_masks.h"
#include "union_contour_piece.h"

namespace tgnn {

constexpr int kUcThreads = 256;
constexpr int kLdsPieces = 3072;             // 4 arrays x 4 B x 3 072 = 48 KB of LDS
constexpr int kListTiles = 2048;             // tiles per chunk of the alive-tile lists (8 KB of LDS)
constexpr int kPieceWords = 13;              // int32 words of workspace per piece

struct ContourArgs : MaskSet {
    int64_t cap_pieces, cap_rings, cap_points;
    // workspace
    int64_t *piece_off, *ring_off, *point_off;               // [K]
    int32_t *status, *m_pieces, *m_rings, *m_points;         // [K]
    int32_t *first;                                          // [K][n_tiles + 1]
    int32_t *label;                                          // [K][n_tiles]
    int32_t *p_tile, *p_side, *p_src, *p_end, *p_next, *p_keep, *r_lead, *r_cnt, *r_first, *work;     // [cap_pieces] (work: 4 x)
    // outputs
    int32_t *mask_out, *ring_out;
    double *ring_area, *pts_xy;
    int32_t *pts_src;
    int64_t *total_out;
};
static_assert(contour::kErrIndex == topo::kErrIndex, "topo::collides reports into the contour error word");

// Exclusive scan of a[0 .. n) in place, in index order, by the whole block; returns the total (uniform).  tmp: kUcThreads words.
template <class T>
__device__ T block_scan_exclusive(T *a, int64_t n, T *tmp) {
    const int tid = threadIdx.x;
    T carry = 0;
    for (int64_t base = 0; base < n; base += kUcThreads) {
        const T v = base + tid < n ? a[base + tid] : 0;
        tmp[tid] = v;
        __syncthreads();
        for (int d = 1; d < kUcThreads; d <<= 1) {
            const T add = tid >= d ? tmp[tid - d] : 0;
            __syncthreads();
            tmp[tid] += add;
            __syncthreads();
        }
        if (base + tid < n) a[base + tid] = carry + tmp[tid] - v;
        carry += tmp[kUcThreads - 1];
        __syncthreads();
    }
    return carry;
}

struct CountSink {
    int n;
    __device__ void operator()(int32_t, int32_t, int32_t) { ++n; }
};

struct FillSink {
    contour::Pieces pc;
    int32_t at, limit, tile;                 // never past the pieces the count gave the tile
    __device__ void operator()(int32_t side, int32_t src, int32_t end) {
        if (at < limit) {
            pc.tile[at] = tile;
            pc.side[at] = side;
            pc.src[at] = src;
            pc.end[at] = end;
        }
        ++at;
    }
};

__global__ __launch_bounds__(kUcThreads) void union_contour_prep_kernel(ContourArgs a) {
    __shared__ int32_t tmp[kUcThreads], list[kListTiles];
    __shared__ int collide, changed, n_list;
    const int tid = threadIdx.x;
    const int64_t k = blockIdx.x, n = a.g.n_tiles;
    const int32_t *al = a.alive + k * n;
    int32_t *first = a.first + k * (n + 1);
    volatile int32_t *lab = a.label + k * n;
    if (tid == 0) collide = 0;
    __syncthreads();
    int err = 0;
    contour::Splits sp;
    // the alive tiles are few (a fifth of a solution's candidates): a chunk's alive tiles go into a list first, so that the
    // pieces, not the tiles, fill the lanes (in any order: every tile writes its own word)
    for (int64_t c0 = 0; c0 < n; c0 += kListTiles) {
        const int64_t c1 = c0 + kListTiles < n ? c0 + kListTiles : n;
        if (tid == 0) n_list = 0;
        __syncthreads();
        for (int64_t i = c0 + tid; i < c1; i += kUcThreads) {
            const bool alive = al[i] != 0;
            lab[i] = alive ? (int32_t)i : -1;
            first[i] = 0;
            if (alive) list[atomicAdd(&n_list, 1)] = (int32_t)(i - c0);
        }
        __syncthreads();
        for (int w = tid; w < n_list; w += kUcThreads) {
            const int64_t i = c0 + list[w];
            CountSink sink{0};
            if (topo::collides(a.col_ptr, a.col_idx, al, i, n, 0, 1, err)) collide = 1;
            else contour::tile_pieces(a.g, al, i, sp, err, sink);
            first[i] = sink.n;
        }
        __syncthreads();
    }
    if (tid == 0) first[n] = 0;
    __syncthreads();
    const bool bad = collide != 0;
    const int32_t pieces = block_scan_exclusive(first, n + 1, tmp);
    if (tid == 0) {
        a.status[k] = bad ? 1 : 0;
        a.m_pieces[k] = bad ? 0 : pieces;
    }
    // component labels, in the workspace (there is no LDS to spare for them here)
    int ignored = 0;                                         // (a bad contact index is tile_pieces' to report, not the labelling's)
    label_components<kUcThreads, false>(a.g, lab, nullptr, nullptr, &changed, ignored);
    if (err != 0) atomicOr(a.err_flag, err);
}

__global__ __launch_bounds__(kUcThreads) void union_contour_offsets_kernel(ContourArgs a) {
    __shared__ int64_t tmp[kUcThreads];
    for (int64_t k = threadIdx.x; k < a.n_masks; k += kUcThreads) a.piece_off[k] = a.m_pieces[k];
    __syncthreads();
    block_scan_exclusive(a.piece_off, a.n_masks, tmp);
}

__global__ __launch_bounds__(kUcThreads) void union_contour_trace_kernel(ContourArgs a) {
    __shared__ int32_t lds_work[4 * kLdsPieces];
    __shared__ int32_t tmp[kUcThreads];
    __shared__ int broken, n_list;
    static_assert(kListTiles <= kLdsPieces, "the list of tiles borrows a working array");
    int32_t *list = lds_work + 3 * kLdsPieces;               // (free until the leaders' ping-pong, long after the fill)
    const int tid = threadIdx.x;
    const int64_t k = blockIdx.x, nt = a.g.n_tiles;
    const int32_t n = a.m_pieces[k];
    const int64_t off = a.piece_off[k];
    if (n == 0 || off + n > a.cap_pieces) {                  // empty, colliding, or a workspace sized for fewer pieces
        if (tid == 0) {
            a.m_rings[k] = a.m_points[k] = 0;
            if (n != 0) {
                a.m_pieces[k] = 0;
                atomicOr(a.err_flag, contour::kErrCapacity);
            }
        }
        return;
    }
    const int32_t *al = a.alive + k * nt, *first = a.first + k * (nt + 1);
    const contour::Pieces pc{a.p_tile + off, a.p_side + off, a.p_src + off, a.p_end + off};
    int32_t *next = a.p_next + off, *keep = a.p_keep + off;
    int32_t *w[4];
    for (int q = 0; q < 4; ++q) w[q] = n <= kLdsPieces ? lds_work + q * kLdsPieces : a.work + q * a.cap_pieces + off;
    if (tid == 0) broken = 0;
    __syncthreads();
    int err = 0;
    // fill: a thread per tile; a tile that does not give the pieces it was counted with ends the mask (TRACE) before any
    // piece is read
    contour::Splits sp;
    for (int64_t c0 = 0; c0 < nt; c0 += kListTiles) {         // (the tiles with pieces into a list first, as in the prep kernel)
        const int64_t c1 = c0 + kListTiles < nt ? c0 + kListTiles : nt;
        if (tid == 0) n_list = 0;
        __syncthreads();
        for (int64_t i = c0 + tid; i < c1; i += kUcThreads)
            if (first[i + 1] != first[i]) list[atomicAdd(&n_list, 1)] = (int32_t)(i - c0);
        __syncthreads();
        for (int w = tid; w < n_list; w += kUcThreads) {
            const int64_t i = c0 + list[w];
            FillSink sink{pc, first[i], first[i + 1], (int32_t)i};
            contour::tile_pieces(a.g, al, i, sp, err, sink);
            if (sink.at != first[i + 1]) broken = 1;
        }
        __syncthreads();
    }
    for (int32_t e = tid; e < n; e += kUcThreads) w[0][e] = 0;
    __syncthreads();
    if (broken != 0) {                                       // (uniform)
        if (tid == 0) {
            a.m_rings[k] = a.m_points[k] = 0;
            a.m_pieces[k] = 0;
            atomicOr(a.err_flag, contour::kErrTrace);
        }
        if (err != 0) atomicOr(a.err_flag, err);
        return;
    }
    // link: a thread per piece; w[0] counts how many pieces continue into each
    contour::Leaving lv;
    bool lost = false;
    for (int32_t e = tid; e < n; e += kUcThreads) {
        const int32_t f = contour::link_piece(a.g, al, first, pc, e, lv, err);
        next[e] = f;
        if (f < 0) lost = true;
        else atomicAdd(&w[0][f], 1);
    }
    __syncthreads();
    for (int32_t e = tid; e < n; e += kUcThreads) lost |= w[0][e] != 1;
    if (lost) broken = 1;
    __syncthreads();
    if (broken != 0) {                                       // (uniform) not a permutation: nothing is emitted, nothing spins
        if (tid == 0) {
            a.m_rings[k] = a.m_points[k] = 0;
            a.m_pieces[k] = 0;
            atomicOr(a.err_flag, contour::kErrTrace);
        }
        if (err != 0) atomicOr(a.err_flag, err);
        return;
    }
    // leaders: min-propagation with pointer doubling, ping-pong between (w0, w1) and (w2, w3)
    int32_t *lead = w[0], *jump = w[1], *lead2 = w[2], *jump2 = w[3];
    for (int32_t e = tid; e < n; e += kUcThreads) {
        lead[e] = e;
        jump[e] = next[e];
    }
    int rounds = 1;
    while ((1ll << (rounds - 1)) < n) ++rounds;              // ceil(log2 n) + 1
    for (int r = 0; r < rounds; ++r) {
        __syncthreads();
        for (int32_t e = tid; e < n; e += kUcThreads) {
            const int32_t j = jump[e], mine = lead[e], theirs = lead[j];
            lead2[e] = theirs < mine ? theirs : mine;
            jump2[e] = jump[j];
        }
        int32_t *t = lead;
        lead = lead2;
        lead2 = t;
        t = jump;
        jump = jump2;
        jump2 = t;
    }
    // corner flags; corners per ring on the leader's word (jump is free now)
    int32_t *cnt = jump, *flag = lead2;
    for (int32_t e = tid; e < n; e += kUcThreads) {
        const int32_t f = next[e];
        keep[f] = contour::is_corner(a.g, pc, e, f) ? 1 : 0;
        cnt[e] = 0;
    }
    __syncthreads();
    for (int32_t e = tid; e < n; e += kUcThreads) {
        if (keep[e] != 0) atomicAdd(&cnt[lead[e]], 1);
        flag[e] = lead[e] == e ? 1 : 0;
    }
    __syncthreads();
    const int32_t rings = block_scan_exclusive(flag, (int64_t)n, tmp);
    int32_t *r_lead = a.r_lead + off, *r_cnt = a.r_cnt + off, *r_first = a.r_first + off;
    for (int32_t e = tid; e < n; e += kUcThreads) {
        if (lead[e] != e) continue;
        r_lead[flag[e]] = e;
        r_cnt[flag[e]] = cnt[e];
    }
    __syncthreads();
    const int32_t points = block_scan_exclusive(cnt, (int64_t)n, tmp);
    for (int32_t e = tid; e < n; e += kUcThreads)
        if (lead[e] == e) r_first[flag[e]] = cnt[e];
    if (tid == 0) {
        a.m_rings[k] = rings;
        a.m_points[k] = points;
    }
    if (err != 0) atomicOr(a.err_flag, err);
}

__global__ __launch_bounds__(kUcThreads) void union_contour_finish_kernel(ContourArgs a) {
    __shared__ int64_t tmp[kUcThreads];
    for (int64_t k = threadIdx.x; k < a.n_masks; k += kUcThreads) {
        a.ring_off[k] = a.m_rings[k];
        a.point_off[k] = a.m_points[k];
    }
    __syncthreads();
    const int64_t rings = block_scan_exclusive(a.ring_off, a.n_masks, tmp);
    const int64_t points = block_scan_exclusive(a.point_off, a.n_masks, tmp);
    const int64_t top = 0x7fffffff;
    for (int64_t k = threadIdx.x; k < a.n_masks; k += kUcThreads) {
        a.mask_out[4 * k + 0] = a.m_rings[k];
        a.mask_out[4 * k + 1] = (int32_t)(a.ring_off[k] < top ? a.ring_off[k] : top);
        a.mask_out[4 * k + 2] = a.m_points[k];
        a.mask_out[4 * k + 3] = a.status[k];
    }
    if (threadIdx.x == 0) {
        a.total_out[0] = rings;
        a.total_out[1] = points;
        if (rings > a.cap_rings || points > a.cap_points) atomicOr(a.err_flag, contour::kErrCapacity);
    }
}

__global__ __launch_bounds__(kUcThreads) void union_contour_emit_kernel(ContourArgs a) {
    const int64_t k = blockIdx.x, off = a.piece_off[k];
    const int32_t rings = a.m_rings[k], n = a.m_pieces[k];
    const int32_t *next = a.p_next + off, *keep = a.p_keep + off, *src = a.p_src + off;
    const int32_t *label = a.label + k * a.g.n_tiles;
    for (int32_t r = threadIdx.x; r < rings; r += kUcThreads) {
        const int32_t e0 = a.r_lead[off + r];
        const int64_t p0 = a.point_off[k] + a.r_first[off + r], ring = a.ring_off[k] + r;
        topo::Pt base{0.0, 0.0}, prev{0.0, 0.0};
        double twice = 0.0;
        int32_t e = e0, listed = 0;
        for (int32_t step = 0; step < n; ++step) {           // (a ring has at most n pieces)
            if (keep[e] != 0) {
                const int32_t v = src[e];
                const topo::Pt p = a.g.ring_xy[v];
                if (listed == 0) base = p;
                else twice += (prev.x - base.x) * (p.y - base.y) - (prev.y - base.y) * (p.x - base.x);
                prev = p;
                if (p0 + listed < a.cap_points) {
                    a.pts_xy[2 * (p0 + listed) + 0] = p.x;
                    a.pts_xy[2 * (p0 + listed) + 1] = p.y;
                    a.pts_src[p0 + listed] = v;
                }
                ++listed;
            }
            e = next[e];
            if (e == e0) break;
        }
        if (ring < a.cap_rings) {
            a.ring_out[4 * ring + 0] = (int32_t)p0;
            a.ring_out[4 * ring + 1] = listed;
            a.ring_out[4 * ring + 2] = label[a.p_tile[off + e0]];
            a.ring_out[4 * ring + 3] = twice > 0.0 ? 1 : -1;
            a.ring_area[ring] = 0.5 * twice;
        }
    }
}

}  // namespace tgnn

using namespace tgnn;

static size_t contour_fixed_bytes(int64_t n_masks, int64_t n_tiles) {
    return (size_t)n_masks * (3 * sizeof(int64_t) + 4 * sizeof(int32_t) + (2 * (size_t)n_tiles + 1) * sizeof(int32_t));
}

extern "C" size_t tgnn_union_contour_workspace_bytes(int64_t n_masks, int64_t n_tiles, int64_t max_pieces) {
    if (n_masks <= 0 || n_tiles <= 0 || max_pieces < 0 || n_masks > (1ll << 56) / (n_tiles + 4) || max_pieces > (1ll << 56)) return 0;
    return align_up(contour_fixed_bytes(n_masks, n_tiles), 8) + (size_t)max_pieces * kPieceWords * sizeof(int32_t);
}

extern "C" int tgnn_union_contour(const double *ring_xy, const int32_t *ring_ptr, int64_t n_tiles, const int32_t *col_ptr,
                                  const int32_t *col_idx, const int32_t *touch_ptr, const int32_t *touch_idx,
                                  const int32_t *alive, int64_t n_masks, double tol, int64_t cap_rings, int64_t cap_points,
                                  int32_t *mask_out, int32_t *ring_out, double *ring_area, double *pts_xy, int32_t *pts_src,
                                  int64_t *total_out, int32_t *err_flag, void *ws, size_t ws_bytes, tgnn_stream_t stream) {
    DeviceGuard guard__(stream);
    TGNN_CHECK_ARG(n_masks < (1ll << 31) - 1, "shape");      // (a block per mask, no chunks)
    if (int rc = check_mask_shape(__func__, n_tiles, n_masks, tol, 1.0, 0.0)) return rc;
    TGNN_CHECK_ARG(cap_rings >= 0 && cap_points >= 0 && cap_rings < (1ll << 31) && cap_points < (1ll << 31), "capacity");
    hipStream_t s = static_cast<hipStream_t>(stream);
    if (n_masks == 0 || n_tiles == 0) {
        if (total_out) TGNN_CHECK_HIP(hipMemsetAsync(total_out, 0, 2 * sizeof(int64_t), s));
        if (n_masks != 0) {
            TGNN_CHECK_ARG(mask_out, "null mask_out");
            TGNN_CHECK_HIP(hipMemsetAsync(mask_out, 0, sizeof(int32_t) * 4 * n_masks, s));
        }
        return TGNN_OK;
    }
    TGNN_CHECK_ARG(mask_out && total_out && err_flag, "null mask_out / total_out / err_flag");
    TGNN_CHECK_ARG((ring_out && ring_area) || cap_rings == 0, "null ring_out / ring_area");
    TGNN_CHECK_ARG((pts_xy && pts_src) || cap_points == 0, "null pts_xy / pts_src");
    const size_t fixed = align_up(contour_fixed_bytes(n_masks, n_tiles), 8);     // (any value when K * n_tiles overflows: not used then)
    if (int rc = check_mask_arrays(__func__, n_masks, (1ll << 56) / (n_tiles + 4), ring_xy && ring_ptr && col_ptr && touch_ptr && alive,
                                   ws, ws_bytes, fixed, sizeof(int64_t)))
        return rc;
    ContourArgs a{};
    a.g = {reinterpret_cast<const topo::Pt *>(ring_xy), ring_ptr, n_tiles, touch_ptr, touch_idx, tol, 1.0, 0.0};
    a.col_ptr = col_ptr;
    a.col_idx = col_idx;
    a.alive = alive;
    a.n_masks = n_masks;
    a.cap_pieces = (int64_t)((ws_bytes - fixed) / (kPieceWords * sizeof(int32_t)));
    a.cap_rings = cap_rings;
    a.cap_points = cap_points;
    int64_t *longs = static_cast<int64_t *>(ws);
    a.piece_off = longs;
    a.ring_off = longs + n_masks;
    a.point_off = longs + 2 * n_masks;
    int32_t *words = reinterpret_cast<int32_t *>(longs + 3 * n_masks);
    a.status = words;
    a.m_pieces = words + n_masks;
    a.m_rings = words + 2 * n_masks;
    a.m_points = words + 3 * n_masks;
    a.first = words + 4 * n_masks;
    a.label = a.first + n_masks * (n_tiles + 1);
    int32_t *pieces = reinterpret_cast<int32_t *>(static_cast<char *>(ws) + fixed);
    int32_t **slots[] = {&a.p_tile, &a.p_side, &a.p_src, &a.p_end, &a.p_next, &a.p_keep, &a.r_lead, &a.r_cnt, &a.r_first, &a.work};
    for (int q = 0; q < 10; ++q) *slots[q] = pieces + q * a.cap_pieces;
    a.mask_out = mask_out;
    a.ring_out = ring_out;
    a.ring_area = ring_area;
    a.pts_xy = pts_xy;
    a.pts_src = pts_src;
    a.total_out = total_out;
    a.err_flag = err_flag;
    const unsigned grid = (unsigned)n_masks;
    union_contour_prep_kernel<<<grid, kUcThreads, 0, s>>>(a);
    union_contour_offsets_kernel<<<1, kUcThreads, 0, s>>>(a);
    union_contour_trace_kernel<<<grid, kUcThreads, 0, s>>>(a);
    union_contour_finish_kernel<<<1, kUcThreads, 0, s>>>(a);
    union_contour_emit_kernel<<<grid, kUcThreads, 0, s>>>(a);
    TGNN_CHECK_LAUNCH();
    return TGNN_OK;
}
