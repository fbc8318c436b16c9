// The adjoint of NNConv(aggr="mean") on edge groups, widths 32 and 64, behind tgnn_set_nnconv_bwd_eg.
//
// Reference semantics: the backward of GraphConv.forward (graph_networks/layers/edge_conv.py:24-27 of the reference) as autograd
// derives it from PyG 1.3.2 NNConv.  With g = dz / max(deg_in, 1):
//     dh[v]  = sum_{e: src_e = v} g[dst_e] . W_{type_e}^T  +  dz[v] . root^T
//     dW_t   = sum_{e: type_e = t} h[src_e]^T (x) g[dst_e]           d root = h^T . dz
// The chain (train.hip, train.nnconv_backward) goes through S' [N][(T+1) C], the per-node type sums of g over the transposed graph:
// written once, read twice, 358 MB per layer at 100 000 nodes / T = 13 / width 64.  Here nothing of that size exists:
//   dh   the forward op itself over the TRANSPOSED graph's edge groups with the transposed table, in the kernels' SUM form
//        (nnconv_eg.hip / nnconv64_eg.hip: no mean, no bias, no activation; the root group reads dz, S = I);
//   dW   nnconv_bwd_eg_dw_kernel: per group of the FORWARD structure (16 edges of one type into one 16-row tile) the outer product
//        H^T [C x 16] . G [16 x C] on v_mfma_f32_16x16x4_f32 (exact fp32: no operand bounds), accumulated per type in registers;
//        the root groups are type T with H = the tile's rows of h and G = its rows of dz.  A block walks a contiguous share of the
//        type-major group list, stores one partial tile per type it meets, and nnconv_bwd_eg_fold_kernel adds the partials of a
//        type in block order straight into dwcat [T+1][C][C] -- no atomics, the same bits on every call at a given grid.
#include <atomic>

#include "nnconv64_eg.h"
#include "nnconv_bwd_eg_plan.h"
#include "tgnn_common.h"

namespace tgnn {

static std::atomic<int> g_nnconv_bwd_eg{0};                // tgnn_set_nnconv_bwd_eg
static_assert(kBwdEgImageFloats32 == kWtTypeF16, "the width-32 image of nnconv_eg.hip");
static_assert(kBwdEgMaxTypes32 + 2 <= 32 && 32 + kBwdEgMaxTypes32 + 1 <= kBwdEgListHeader, "the list header holds offsets and counts");

using f32x4 = __attribute__((ext_vector_type(4))) float;

#define TGNN_TRY_EG(expr)                \
    do {                                 \
        const int rc__ = (expr);         \
        if (rc__ != TGNN_OK) return rc__; \
    } while (0)

// wt [t][a][b] = W_t[b][a] for the T table entries, entry T = root^T: what the forward's image kernels take as (wtab, root)
__global__ __launch_bounds__(256) void nnconv_bwd_eg_transpose_kernel(const float *__restrict__ wtab, const float *__restrict__ root,
                                                                      int n_types, int c, float *__restrict__ wt) {
    const int t = blockIdx.x;
    const float *src = t < n_types ? wtab + (int64_t)t * c * c : root;
    float *dst = wt + (int64_t)t * c * c;
    for (int r = threadIdx.x; r < c * c; r += 256) dst[r] = src[(r % c) * c + r / c];
}

// ---- the type-major list: [0 .. T + 1] offsets of the types (root groups = type T), [32 .. 32 + T] their counts, then from
// kBwdEgListHeader on the (group, tile) pairs sorted by type, groups of a type in ascending order: a stable counting sort without
// atomics.  Block t walks every tile; FILL = false counts, FILL = true (a second launch) places.
template <bool FILL>
__global__ __launch_bounds__(256) void nnconv_bwd_eg_list_kernel(const int *__restrict__ tile_grp_ptr, const int2 *__restrict__ grp,
                                                                 int64_t n_tiles, int n_types, int *__restrict__ list) {
    __shared__ int scan[256];
    __shared__ int run_s;
    const int t = blockIdx.x, tid = threadIdx.x;
    int base = 0;
    if (FILL) {
        for (int u = 0; u < t; ++u) base += list[32 + u];
        if (t == 0 && tid == 0) {
            int acc = 0;
            for (int u = 0; u <= n_types; ++u) {
                list[u] = acc;
                acc += list[32 + u];
            }
            list[n_types + 1] = acc;
        }
    }
    if (tid == 0) run_s = 0;
    __syncthreads();
    for (int64_t tile0 = 0; tile0 < n_tiles; tile0 += 256) {
        const int64_t tile = tile0 + tid;
        int cnt = 0, first = 0;
        if (tile < n_tiles) {
            const int g0 = tile_grp_ptr[tile], g1 = tile_grp_ptr[tile + 1];
            for (int g = g0; g < g1; ++g)
                if (((grp[(int64_t)g * 16].y >> 16) & 0xff) == t) {     // (the groups of a type are contiguous in a tile)
                    if (cnt == 0) first = g;
                    ++cnt;
                }
        }
        scan[tid] = cnt;
        __syncthreads();
        for (int d = 1; d < 256; d <<= 1) {                  // inclusive scan
            const int v = tid >= d ? scan[tid - d] : 0;
            __syncthreads();
            scan[tid] += v;
            __syncthreads();
        }
        const int run = run_s;
        if (FILL) {
            int2 *pairs = reinterpret_cast<int2 *>(list + kBwdEgListHeader);
            const int64_t at = (int64_t)base + run + scan[tid] - cnt;
            for (int j = 0; j < cnt; ++j) pairs[at + j] = make_int2(first + j, (int)tile);
        }
        __syncthreads();
        if (tid == 255) run_s = run + scan[255];
        __syncthreads();
    }
    if (!FILL && tid == 0) list[32 + t] = run_s;
}

// ---- dW.  grid = the plan's blocks, 4 waves; every wave holds a whole C x C tile (acc[ib][ob][r]: input channel 16 ib + 4 q + r,
// output channel 16 ob + i for lane (i, q)) and takes every 4th group of the block's share of a type.
template <int C>
__global__ __launch_bounds__(kBwdEgDwThreads, 2) void nnconv_bwd_eg_dw_kernel(
    const float *__restrict__ h, const float *__restrict__ g, const float *__restrict__ dz, uint32_t row_bytes, const int2 *__restrict__ grp,
    const int *__restrict__ list, int n_types, int64_t n, float *__restrict__ slots) {
    constexpr int NB = C / 16;
    constexpr uint32_t kOob = 0x80000000u;                   // beyond every buffer (rows lie within 2 GB): the load returns zeros
    __shared__ float red[C * C];
    __shared__ int off_s[32];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, li = lane & 15, lq = lane >> 4;
    if (tid < n_types + 2) off_s[tid] = list[tid];
    __syncthreads();
    const BwdEgShare share = nnconv_bwd_eg_dw_share(off_s[n_types + 1], (int)gridDim.x, (int)blockIdx.x);
    const int2 *pairs = reinterpret_cast<const int2 *>(list + kBwdEgListHeader);
    const __amdgpu_buffer_rsrc_t h_rsrc = __builtin_amdgcn_make_buffer_rsrc(const_cast<float *>(h), 0, (int)row_bytes, 0x00020000);
    const __amdgpu_buffer_rsrc_t g_rsrc = __builtin_amdgcn_make_buffer_rsrc(const_cast<float *>(g), 0, (int)row_bytes, 0x00020000);
    const __amdgpu_buffer_rsrc_t z_rsrc = __builtin_amdgcn_make_buffer_rsrc(const_cast<float *>(dz), 0, (int)row_bytes, 0x00020000);

    for (int t = 0; t <= n_types; ++t) {                     // (block-uniform)
        const int64_t lo = share.begin > off_s[t] ? share.begin : off_s[t];
        const int64_t hi = share.end < off_s[t + 1] ? share.end : off_s[t + 1];
        if (lo >= hi) continue;
        const bool root = t == n_types;
        f32x4 acc[NB][NB];
#pragma unroll
        for (int ib = 0; ib < NB; ++ib)
#pragma unroll
            for (int ob = 0; ob < NB; ++ob) acc[ib][ob] = f32x4{0.f, 0.f, 0.f, 0.f};

        // group p of the list: a[kk][ib] = h[source of edge 4 kk + q][16 ib + i], b[kk][ob] = g[its destination row][16 ob + i]
        // Its index words are two dependent loads -- the (group, tile) pair, then lane i's (source, mask) word --: they are fetched
        // three and two groups ahead of the products, the operands one group ahead, so that no wave waits for a load it has just
        // issued (entries past the share: the share's last one, loaded and not used)
        auto load_pair = [&](int64_t p) { return pairs[p < hi ? p : hi - 1]; };
        auto load_word = [&](int2 pr) { return grp[(int64_t)__builtin_amdgcn_readfirstlane(pr.x) * 16 + li]; };
        auto fetch = [&](int2 pr, int2 w, float (&a)[4][NB], float (&b)[4][NB]) {   // w: lane i = slot i's source, row i's mask
            const int tile = __builtin_amdgcn_readfirstlane(pr.y);
            int src, dst;
            if (root) {                                      // the tile's own rows: w.x = float bits of max(deg, 1), -1 beyond n
                src = w.x >= 0 ? tile * 16 + li : -1;
                dst = w.x >= 0 ? li : -1;
            } else {
                src = w.x;
                dst = -1;
#pragma unroll
                for (int j = 0; j < 16; ++j) {
                    const int mj = __builtin_amdgcn_readlane(w.y, j);
                    if ((mj >> li) & 1) dst = j;
                }
                if (src < 0) dst = -1;
            }
#pragma unroll
            for (int kk = 0; kk < 4; ++kk) {
                const int se = __shfl(src, 4 * kk + lq, 64), de = __shfl(dst, 4 * kk + lq, 64);
                const int64_t drow = (int64_t)tile * 16 + de;
                const uint32_t ao = se >= 0 && se < n ? (uint32_t)se * (uint32_t)(C * 4) + (uint32_t)li * 4u : kOob;
                const uint32_t bo = de >= 0 && drow < n ? (uint32_t)drow * (uint32_t)(C * 4) + (uint32_t)li * 4u : kOob;
#pragma unroll
                for (int ib = 0; ib < NB; ++ib)
                    a[kk][ib] = __builtin_bit_cast(float, __builtin_amdgcn_raw_buffer_load_b32(h_rsrc, ao + 64u * ib, 0, 0));
                if (root) {
#pragma unroll
                    for (int ob = 0; ob < NB; ++ob)
                        b[kk][ob] = __builtin_bit_cast(float, __builtin_amdgcn_raw_buffer_load_b32(z_rsrc, bo + 64u * ob, 0, 0));
                } else {
#pragma unroll
                    for (int ob = 0; ob < NB; ++ob)
                        b[kk][ob] = __builtin_bit_cast(float, __builtin_amdgcn_raw_buffer_load_b32(g_rsrc, bo + 64u * ob, 0, 0));
                }
            }
        };
        auto mma = [&](const float (&a)[4][NB], const float (&b)[4][NB]) {
#pragma unroll
            for (int kk = 0; kk < 4; ++kk)
#pragma unroll
                for (int ib = 0; ib < NB; ++ib)
#pragma unroll
                    for (int ob = 0; ob < NB; ++ob)
                        acc[ib][ob] = __builtin_amdgcn_mfma_f32_16x16x4f32(a[kk][ib], b[kk][ob], acc[ib][ob], 0, 0, 0);
        };
        float a0[4][NB], b0[4][NB], a1[4][NB], b1[4][NB];
        constexpr int S = kBwdEgDwWaves;
        int64_t p = lo + wave;                               // (wave-uniform from here on)
        if (p < hi) {
            int2 pr1 = load_pair(p + S), pr2 = load_pair(p + 2 * S);
            {
                const int2 pr0 = load_pair(p);
                fetch(pr0, load_word(pr0), a0, b0);
            }
            int2 w1 = load_word(pr1);
            // entering a round: (a0, b0) = group p's operands in flight, (pr1, w1) = the words of p + S, pr2 = the pair of p + 2 S
            for (; p < hi; p += 2 * S) {
                const int2 pr3 = load_pair(p + 3 * S), w2 = load_word(pr2);
                const bool more = p + S < hi;
                if (more) fetch(pr1, w1, a1, b1);
                mma(a0, b0);
                if (more) {
                    const int2 pr4 = load_pair(p + 4 * S), w3 = load_word(pr3);
                    if (p + 2 * S < hi) fetch(pr2, w2, a0, b0);
                    mma(a1, b1);
                    pr1 = pr3;
                    w1 = w3;
                    pr2 = pr4;
                }
            }
        }
        // the four waves' tiles, added in wave order; then the block's partial of type t
        for (int w = 0; w < kBwdEgDwWaves; ++w) {
            if (wave == w) {
#pragma unroll
                for (int ib = 0; ib < NB; ++ib)
#pragma unroll
                    for (int ob = 0; ob < NB; ++ob)
#pragma unroll
                        for (int r = 0; r < 4; ++r) {
                            const int at = (16 * ib + 4 * lq + r) * C + 16 * ob + li;
                            red[at] = w == 0 ? acc[ib][ob][r] : red[at] + acc[ib][ob][r];
                        }
            }
            __syncthreads();
        }
        float *slot = slots + (int64_t)nnconv_bwd_eg_dw_slot((int)blockIdx.x, t) * (C * C);
        for (int i = tid; i < C * C; i += kBwdEgDwThreads) slot[i] = red[i];
        __syncthreads();
    }
}

// dwcat [t][in][out] = the partial tiles of type t, added in block order.  grid = (C C / 256, T + 1)
__global__ __launch_bounds__(256) void nnconv_bwd_eg_fold_kernel(const float *__restrict__ slots, const int *__restrict__ list, int n_types,
                                                                 int nblk, int cc, float *__restrict__ dwcat) {
    __shared__ int range_s[2];                              // first and last block whose share meets type t (a contiguous run)
    const int t = blockIdx.y, e = blockIdx.x * 256 + threadIdx.x;
    if (threadIdx.x == 0) {
        range_s[0] = nblk;
        range_s[1] = -1;
    }
    __syncthreads();
    {
        const int64_t o0 = list[t], o1 = list[t + 1], n_list = list[n_types + 1];
        for (int b = threadIdx.x; b < nblk; b += 256) {      // (integer min / max: the same answer in any order)
            const BwdEgShare sh = nnconv_bwd_eg_dw_share(n_list, nblk, b);
            const int64_t lo = sh.begin > o0 ? sh.begin : o0, hi = sh.end < o1 ? sh.end : o1;
            if (lo < hi) {
                atomicMin(&range_s[0], b);
                atomicMax(&range_s[1], b);
            }
        }
    }
    __syncthreads();
    const int b_lo = range_s[0], b_hi = range_s[1];
    float sum = 0.f;
    for (int b = b_lo; b <= b_hi; b += 8) {                  // eight loads in flight, added in block order
        float v[8];
#pragma unroll
        for (int u = 0; u < 8; ++u) v[u] = b + u <= b_hi ? slots[(int64_t)nnconv_bwd_eg_dw_slot(b + u, t) * cc + e] : 0.f;
#pragma unroll
        for (int u = 0; u < 8; ++u)
            if (b + u <= b_hi) sum += v[u];
    }
    dwcat[(int64_t)t * cc + e] = sum;
}

}  // namespace tgnn

using namespace tgnn;

extern "C" int32_t tgnn_set_nnconv_bwd_eg(int32_t on) {
    const int prev = g_nnconv_bwd_eg.load();
    if (on == 0 || on == 1) g_nnconv_bwd_eg.store(on);
    return prev;
}

extern "C" int32_t tgnn_nnconv_bwd_eg_ok(int32_t c, int64_t n_nodes, int32_t n_types, int32_t max_in_degree, int32_t max_out_degree,
                                         int32_t has_fwd_groups, int32_t has_bwd_groups) {
    return nnconv_bwd_eg_ok(c, n_nodes, n_types, max_in_degree, max_out_degree, has_fwd_groups != 0, has_bwd_groups != 0) ? 1 : 0;
}

extern "C" size_t tgnn_nnconv_bwd_eg_workspace_bytes(int64_t n_nodes, int64_t n_groups_cap, int32_t n_types, int32_t c) {
    return nnconv_bwd_eg_workspace_bytes(n_nodes, n_groups_cap, n_types, c);
}

extern "C" int32_t tgnn_nnconv_bwd_eg_dw_blocks(int64_t n_list) { return nnconv_bwd_eg_dw_blocks(n_list); }

extern "C" size_t tgnn_nnconv_bwd_eg_list_ints(int64_t n_groups_cap) { return nnconv_bwd_eg_list_ints(n_groups_cap); }

extern "C" int tgnn_nnconv_bwd_eg_build(const int32_t *tile_grp_ptr, const int32_t *grp, int64_t n_nodes, int32_t n_types,
                                        int32_t *type_major, tgnn_stream_t stream) {
    DeviceGuard guard__(stream);
    TGNN_CHECK_ARG(tile_grp_ptr && grp && type_major && ((uintptr_t)grp % 8) == 0 && ((uintptr_t)type_major % 8) == 0,
                   "null / misaligned pointer");
    TGNN_CHECK_ARG(n_nodes >= 1 && n_types >= 0 && n_types <= kBwdEgMaxTypes32, "shape");
    hipStream_t s = static_cast<hipStream_t>(stream);
    const int64_t n_tiles = (n_nodes + 15) / 16;
    nnconv_bwd_eg_list_kernel<false><<<n_types + 1, 256, 0, s>>>(tile_grp_ptr, reinterpret_cast<const int2 *>(grp), n_tiles, n_types,
                                                                  type_major);
    nnconv_bwd_eg_list_kernel<true><<<n_types + 1, 256, 0, s>>>(tile_grp_ptr, reinterpret_cast<const int2 *>(grp), n_tiles, n_types,
                                                                 type_major);
    TGNN_CHECK_LAUNCH();
    return TGNN_OK;
}

extern "C" int tgnn_nnconv_bwd_eg(const float *h, int64_t ld, const float *dz, const float *g, const int32_t *fwd_tile_grp_ptr,
                                  const int32_t *fwd_grp, const int32_t *bwd_tile_grp_ptr, const int32_t *bwd_grp,
                                  const int32_t *type_major, int64_t n_list, const float *wtab, const float *root, int64_t n_nodes,
                                  int32_t n_types, int32_t c, int32_t max_in_degree, int32_t max_out_degree, float *dh, float *dwcat,
                                  void *ws, size_t ws_bytes, tgnn_stream_t stream) {
    DeviceGuard guard__(stream);
    const bool has_fwd = fwd_tile_grp_ptr && fwd_grp && type_major, has_bwd = bwd_tile_grp_ptr && bwd_grp;
    if (const char *why = nnconv_bwd_eg_why_not(c, n_nodes, n_types, max_in_degree, max_out_degree, has_fwd, has_bwd)) {
        set_error("tgnn_nnconv_bwd_eg: %s (width %d, %lld rows, %d edge types, in-degree %d, out-degree %d)", why, c, (long long)n_nodes,
                  n_types, max_in_degree, max_out_degree);
        return TGNN_ERR_UNSUPPORTED;
    }
    TGNN_CHECK_ARG(h && dz && g && wtab && root && dh && dwcat, "null pointer");
    TGNN_CHECK_ARG(ld == c, "packed rows: the row stride of h, dz, g and dh is the width");
    TGNN_CHECK_ARG(((uintptr_t)h % 16) == 0 && ((uintptr_t)dz % 16) == 0 && ((uintptr_t)g % 16) == 0 && ((uintptr_t)dh % 16) == 0 &&
                       ((uintptr_t)dwcat % 16) == 0 && ((uintptr_t)wtab % 16) == 0 && ((uintptr_t)root % 16) == 0 &&
                       ((uintptr_t)fwd_grp % 8) == 0 && ((uintptr_t)bwd_grp % 8) == 0 && ((uintptr_t)type_major % 8) == 0,
                   "alignment");
    TGNN_CHECK_ARG(n_list >= 0 && n_list < ((int64_t)1 << 27), "list length");
    const BwdEgWorkspace lay = nnconv_bwd_eg_workspace(n_types, c);
    if (!ws || ws_bytes < lay.total || ((uintptr_t)ws % 256) != 0) {
        set_error("tgnn_nnconv_bwd_eg: workspace too small or not 256-byte aligned (%zu < %zu)", ws_bytes, lay.total);
        return TGNN_ERR_WORKSPACE;
    }
    hipStream_t s = static_cast<hipStream_t>(stream);
    char *base = static_cast<char *>(ws);
    unsigned *bounds = reinterpret_cast<unsigned *>(base + lay.bounds);
    float *wt = reinterpret_cast<float *>(base + lay.wt), *wimg = reinterpret_cast<float *>(base + lay.wimg);
    float *slots = reinterpret_cast<float *>(base + lay.slots);
    const float *root_t = wt + (size_t)n_types * c * c;

    // ---- dh: the forward kernel's SUM form over the transposed groups.  Scales: the table entries are the forward's (sigmoid outputs
    // in (0, 1), the root by nnconv_weight_scale(max |root|): transposing changes neither), so the image scale stands.  The rows are
    // gradients, 1e-6 and smaller in training: bounds[0] = max |dz| >= max |g| (g = dz / max(deg, 1)) covers both arrays the kernel
    // gathers, and the kernel's power of two sx = pow2_scale_for(bound) lifts them to max |row| sx in [2^8, 2^9) (width 64) or
    // [2^9, 2^10) (width 32) whatever their magnitude -- an exponent shift, exact; the fp16 pair then keeps 22 bits of every element
    // down to 2^-3 and is off by at most 2^-25 (2^-34 of the bound) below.  The C products of a message stay below 2^15 as in the
    // forward; sums over up to 2 048 out-edges accumulate in fp32.
    nnconv_bwd_eg_transpose_kernel<<<n_types + 1, 256, 0, s>>>(wtab, root, n_types, c, wt);
    if (c == 32) {
        launch_forward_scales(bounds, 2, &root_t, 1, bounds + 1, nullptr, 0, nullptr, s);
        launch_absmax(dz, n_nodes * 32, bounds, s);
        launch_nnconv_weight_image(wt, &root_t, n_types, 1, wimg, s, bounds + 1, kEgImageScale);
        TGNN_TRY_EG(launch_nnconv_eg(g, bwd_tile_grp_ptr, bwd_grp, wimg, n_types, nullptr, n_nodes, TGNN_ACT_NONE, dh, nullptr, nullptr, s,
                                  bounds, bounds + 1, nullptr, nullptr, dz));
    } else {
        TGNN_CHECK_HIP(hipMemsetAsync(bounds, 0, 2 * sizeof(uint32_t), s));
        launch_absmax(dz, n_nodes * 64, bounds, s);
        launch_nnconv64_eg_images(wt, &root_t, n_types, 1, wimg, bounds + 1, s);
        TGNN_TRY_EG(launch_nnconv64_eg(g, n_nodes, bwd_tile_grp_ptr, bwd_grp, wimg, n_types, nullptr, n_nodes, TGNN_ACT_NONE, dh, nullptr,
                                    nullptr, s, bounds, bounds + 1, dz));
    }

    // ---- dW: partial tiles per (block, type), folded in block order into dwcat [T+1][C][C] (entry T: d root)
    int cap = kBwdEgDwMaxBlocks;
    if (const int dbg = g_debug_block_cap[0].load(); dbg > 0) cap = dbg;
    const int nblk = nnconv_bwd_eg_dw_blocks(n_list, cap);
    const uint32_t row_bytes = (uint32_t)(n_nodes * c * 4);
    if (c == 32)
        nnconv_bwd_eg_dw_kernel<32><<<nblk, kBwdEgDwThreads, 0, s>>>(h, g, dz, row_bytes, reinterpret_cast<const int2 *>(fwd_grp),
                                                                      type_major, n_types, n_nodes, slots);
    else
        nnconv_bwd_eg_dw_kernel<64><<<nblk, kBwdEgDwThreads, 0, s>>>(h, g, dz, row_bytes, reinterpret_cast<const int2 *>(fwd_grp),
                                                                      type_major, n_types, n_nodes, slots);
    nnconv_bwd_eg_fold_kernel<<<dim3(c * c / 256, n_types + 1), 256, 0, s>>>(slots, type_major, n_types, nblk, c * c, dwcat);
    TGNN_CHECK_LAUNCH();
    return TGNN_OK;
}
