// NNConv(aggr="mean"), network_width 32, "edge group" formulation for gfx950: full gathers instead of type columns.
//
// Reference semantics: GraphConv.forward (/root/reference/graph_networks/layers/edge_conv.py:24-27) over
// PyG 1.3.2 NNConv:   out[v] = mean_{e: dst_e = v} h[src_e] . W_{type_e}  +  h[v] . root + bias  (+ LeakyReLU)
//
// Why another formulation: the type-column kernel (nnconv_cols.hip) is bound by the CU's gather path
// and its columns -- one gather instruction per (type, k-th edge of a row) of a 16-row tile -- are 29 % full at 10 edges
// over 13 types: 70 gather instructions per tile.  Here a gather instruction fetches the sources of 16 EDGES of one type,
// whatever rows of the tile they end in (graph_prep.hip: nnconv_eg_kernel): ~15 groups + the root group per tile, 70-77 %
// full, 31 instructions.  Two chained matrix products per group, both on the matrix pipe, no LDS between them:
//     M [16 edges x 32]  = G [16 edges x 32] . W_t        (fp16-pair split, 3 terms: v_mfma_f32_16x16x32_f16 x 6)
//     out[16 rows x 32] += S [16 rows x 16 edges] . M     (S: 0 / 1 selection of the group, exact; M split into an fp16 pair:
//                                                          v_mfma_f32_16x16x16_f16 x 4)
// The accumulator layout of the first product (lane (j, q): edges 4 q + r, channel j) IS the B-operand layout of the second.
// The root group (the rows themselves, W = root) takes the same path with S = diag(max(deg, 1)): one 1 / deg at the end of the
// tile turns the edge sum into the mean and leaves the root term as it is (in-degrees up to 2048: exact in fp16).  The
// BatchNorm partial sums need no transpose any more (a lane holds ONE channel of 4 rows).
#include <atomic>
#include <type_traits>

#include "tgnn_common.h"
#include "nnconv_eg_plan.h"
#include "split_pair_f16.h"

namespace tgnn {

using f32x4 = __attribute__((ext_vector_type(4))) float;
using f16x8 = tgnn_f16x8;
using f16x4 = __attribute__((ext_vector_type(4))) _Float16;

constexpr int kEgRootBit = 1 << 8;                        // meta = type | root << 8 (graph_prep.hip: kEgRoot)
constexpr int kEgExtraLog2 = 5;                             // h . sx < 2^10: 32 products with weights below 1 stay below 2^15

using u32x4 = __attribute__((ext_vector_type(4))) unsigned;
using u32x2 = __attribute__((ext_vector_type(2))) unsigned;

// [r6] SHARD: the sharded step's pack launch inside this kernel (forward.hip, split exchange: NNConv -> pack -> all-to-all -> ... is a
// serial chain of launches with a 4 - 12 us gap each).  The epilogue also stores a row into every message slot that carries it
// (send_row_ptr / send_row_slot: the inverse of the message's row list), and the LAST block to finish (two-level ticket fold of the
// partial rows, bn_finalize_kernel's tree: the same bits as shard_pack1_kernel's block 0) writes the shard's BatchNorm sums into
// `sums` and into the message's sums rows (msg_idx[r] = -1 - k: sums row k).
struct EgShard {
    const int *send_row_ptr, *send_row_slot;   // [n + 1], [n_send]: message rows that carry row v
    float *msg;                                // the message, 32 floats per row
    const int *msg_idx;                        // [n_msg]: >= 0 a row of this shard, -1 - k the sums row k
    int64_t n_msg;
    double *sums;                              // [64] this shard's sums (read by the unpack side for the own rank)
    unsigned *counter;                         // 17 zeroed words, left zeroed
    double *group_rows;                        // 16 x 64 doubles
};

// SUM (the adjoint's input gradient, nnconv_bwd_eg.hip: this op over the TRANSPOSED graph with the transposed table): the edge SUM
// instead of the mean, no bias, no activation, no BatchNorm partials; the root group's rows come from a second array, passed in
// `bias`'s place ([N][32] packed like h: dz where h is g = dz / deg), with S = I.  The other instantiations keep their code.
template <int WAVES, int OCC, int ACT, bool SHARD = false, bool SUM = false>
__global__ __launch_bounds__(WAVES * 64, OCC) void nnconv32_eg_kernel(
    const float *__restrict__ h, const int *__restrict__ tile_grp_ptr, const int2 *__restrict__ grp,
    const float *__restrict__ wimg, int n_types, const float *__restrict__ bias, int64_t n,
    int act, float *__restrict__ out, double *__restrict__ bn_partial, const unsigned *__restrict__ h_max,
    const unsigned *__restrict__ root_max, unsigned long long *__restrict__ stamp, EgShard sh = EgShard{}) {
    extern __shared__ __attribute__((aligned(16))) float lds[];
    if (stamp && threadIdx.x == 0) atomicMin(stamp, wall_clock64());
    constexpr int kTy = kWtTypeF16;                         // floats of one type's image
    float *wl = lds;                                        // [(T+1)][2 planes][2 N blocks][4][16] x 8 fp16
    f16x4 *lut = reinterpret_cast<f16x4 *>(lds + (n_types + 1) * kTy);   // [16]: 4 selection bits -> 4 fp16 of 0 / 1
    const unsigned hm_bits = *h_max, hm_exp = (hm_bits >> 23) & 0xffu;           // max |h| < 2^(hm_exp - 126)
#ifdef TGNN_ABL_EGNOUNIT
    const bool unit = hm_exp > 300;                         // (timing ablation: always scaled)
#else
    // no scale where the rows are in range as they are: 2^3 <= max |h| < 2^10 (elements down to 2^-3 keep a NORMAL fp16 low
    // half -- 22 bits --, smaller ones are off by at most 2^-25, 2^-28 of the largest; below 2^3 the scaled split is the exact one)
    const bool unit = hm_exp >= 130 && hm_exp <= 136;
#endif
    const float sx = unit ? 1.0f : pow2_scale_for(hm_bits, kEgExtraLog2);
    const float unscale = 1.0f / (sx * nnconv_weight_scale(*root_max) * kEgImageScale);   // (powers of two: exact)
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int fj = lane & 15, fq = lane >> 4;
    constexpr int kThreads = WAVES * 64;
    // ---- this wave's run of 16-row tiles (nnconv_eg_plan.h: shares follow the XCD, the block, the SIMD, then the waves of a SIMD)
    static_assert(WAVES % kEgSimds == 0, "whole SIMD quads");
    const EgTiles share = nnconv_eg_wave_share(nnconv_eg_n_tiles(n), gridDim.x, blockIdx.x, (uint32_t)wave, WAVES);
    const int64_t t0 = share.t0, t1 = share.t1;
    const int cbeg = __builtin_amdgcn_readfirstlane(tile_grp_ptr[t0]);
    const int cend = __builtin_amdgcn_readfirstlane(tile_grp_ptr[t1]);

    const float bias0 = SUM ? 0.f : bias[fj], bias1 = SUM ? 0.f : bias[16 + fj];
    // BN partial sums of this lane: channel 16 m + fj over the rows 4 fq .. 4 fq + 3 of every tile
    double bs[2] = {0, 0}, bq[2] = {0, 0};

    const __amdgpu_buffer_rsrc_t h_rsrc =
        __builtin_amdgcn_make_buffer_rsrc(const_cast<float *>(h), 0, (int)0x80000000u, 0x00020000);   // 2 GB window
    const __amdgpu_buffer_rsrc_t own_rsrc =
        SUM ? __builtin_amdgcn_make_buffer_rsrc(const_cast<float *>(bias), 0, (int)0x80000000u, 0x00020000) : h_rsrc;
    const uint32_t fq_bytes = (uint32_t)fq * 32u;
    auto load_four = [&](int p, int &s4, int &m4) {         // groups p .. p+3: lane (fj, fq) <- group p + fq, word fj
        const int pc = p < cend ? p : cbeg;                  // (reads past cend stay inside the slack)
        const int2 v = grp[(int64_t)pc * 16 + lane];        // one 8-byte load: (source, mask | meta << 16)
        s4 = v.x;
        m4 = v.y;
    };
    // group u of a four: s = source of slot fj, m = row fj's mask, meta (wave-uniform) = type | root << 8
    auto unpack = [&](auto steady, int p, int u, int s4, int m4, int &s, int &m, int &meta) {
        s = __shfl(s4, u * 16 + fj, 64);
        m = __shfl(m4, u * 16 + fj, 64);
        meta = __builtin_amdgcn_readlane(m4, u * 16) >> 16;
        if constexpr (!decltype(steady)::value)
            if (p + u >= cend) {                             // wave-uniform: past the share = an empty group of type 0
                s = -1;
                m = 0;
                meta = 0;
            }
    };
    int64_t gtile = t0;                                     // tile of the group the gather stage is at
    auto own_off_of = [&](int64_t tile) -> uint32_t {
        const int64_t r = tile * 16 + fj;
        return r < n ? (uint32_t)r * 128u + fq_bytes : 0x80000000u;
    };
    uint32_t own_off = own_off_of(gtile);
    auto issue_gather = [&](int s, int meta, float4 (&x)[2]) {
        const bool root = (meta & kEgRootBit) != 0;          // wave-uniform
#ifdef TGNN_ABL_EGNOGATHER
        const uint32_t off = 0x80000000u + (((uint32_t)s + own_off) & 0);   // (timing ablation: no row is fetched)
#else
        const uint32_t off = root ? own_off : ((uint32_t)s << 7) + fq_bytes;   // s = -1: beyond the window, loads zeros
#endif
        if (SUM && root) {                                   // (wave-uniform) the root rows of the sum form: the second array
            x[0] = __builtin_bit_cast(float4, __builtin_amdgcn_raw_buffer_load_b128(own_rsrc, off, 0, 0));
            x[1] = __builtin_bit_cast(float4, __builtin_amdgcn_raw_buffer_load_b128(own_rsrc, off + 16u, 0, 0));
        } else {
            x[0] = __builtin_bit_cast(float4, __builtin_amdgcn_raw_buffer_load_b128(h_rsrc, off, 0, 0));
            x[1] = __builtin_bit_cast(float4, __builtin_amdgcn_raw_buffer_load_b128(h_rsrc, off + 16u, 0, 0));
        }
        if (root) {
            ++gtile;
            own_off = own_off_of(gtile);
        }
    };

    f32x4 d0 = {0.f, 0.f, 0.f, 0.f}, d1 = d0;               // out tile: rows 4 fq + r, channel fj (d0) and 16 + fj (d1)
    int64_t ctile = t0;
    const f32x4 zero4 = {0.f, 0.f, 0.f, 0.f};
    // unit: the rows go into the fp16 pair as they are (no scale: 4 instructions less per row pair)
    struct Msg {                                            // a group's messages M = G . W_t as fp16 pairs + its selection operand
        u32x2 a0, b0, a1, b1;                               // hi / lo of channel fj (a0, b0) and 16 + fj (a1, b1), edges 4 fq + r
        f16x4 sel;                                          // S[row fj][edges 4 fq .. 4 fq + 3]
    };
    auto stage1 = [&](int s, int m, int meta, const float4 (&x)[2]) -> Msg {
        const int t = meta & 0xff;
        // the type's operand fragments and the selection operand first: their LDS round trip runs under the split's instructions
        constexpr int kPl = kWtPlane / 4;                    // 16-byte fragments per plane
        const f16x8 *wp = reinterpret_cast<const f16x8 *>(wl + t * kTy) + lane;      // lane order: conflict-free
        const f16x8 h0 = wp[0], h1 = wp[64], l0 = wp[kPl], l1 = wp[kPl + 64];
        f16x4 sel0 = lut[(m >> (4 * fq)) & 15];
#ifndef TGNN_ABL_EGLATE
        asm volatile("" : "+v"(sel0) :: "memory");            // (keeps the reads above the split)
#endif
        unsigned xh0, xh1, xh2, xh3, xl0, xl1, xl2, xl3;
#ifdef TGNN_ABL_EGNOSPLIT
        // (timing ablation, VERDICT r5 item 7: the gathered words used as if their producer had split them -- garbage values, the
        //  same instruction stream minus the row split's ~20 instructions per group)
        xh0 = __float_as_uint(x[0].x); xl0 = __float_as_uint(x[0].y); xh1 = __float_as_uint(x[0].z); xl1 = __float_as_uint(x[0].w);
        xh2 = __float_as_uint(x[1].x); xl2 = __float_as_uint(x[1].y); xh3 = __float_as_uint(x[1].z); xl3 = __float_as_uint(x[1].w);
        if (false) {
#else
        if (unit) {                                          // wave-uniform
#endif
            split_pair_f16(x[0].x, x[0].y, xh0, xl0);
            split_pair_f16(x[0].z, x[0].w, xh1, xl1);
            split_pair_f16(x[1].x, x[1].y, xh2, xl2);
            split_pair_f16(x[1].z, x[1].w, xh3, xl3);
        } else {
            split_pair_f16(x[0].x, x[0].y, sx, xh0, xl0);
            split_pair_f16(x[0].z, x[0].w, sx, xh1, xl1);
            split_pair_f16(x[1].x, x[1].y, sx, xh2, xl2);
            split_pair_f16(x[1].z, x[1].w, sx, xh3, xl3);
        }
        const f16x8 gh = __builtin_bit_cast(f16x8, u32x4{xh0, xh1, xh2, xh3}), gl = __builtin_bit_cast(f16x8, u32x4{xl0, xl1, xl2, xl3});
        f32x4 m0 = __builtin_amdgcn_mfma_f32_16x16x32_f16(gh, l0, zero4, 0, 0, 0);   // hi . lo
        f32x4 m1 = __builtin_amdgcn_mfma_f32_16x16x32_f16(gh, l1, zero4, 0, 0, 0);
        m0 = __builtin_amdgcn_mfma_f32_16x16x32_f16(gl, h0, m0, 0, 0, 0);           // lo . hi
        m1 = __builtin_amdgcn_mfma_f32_16x16x32_f16(gl, h1, m1, 0, 0, 0);
        m0 = __builtin_amdgcn_mfma_f32_16x16x32_f16(gh, h0, m0, 0, 0, 0);           // hi . hi
        m1 = __builtin_amdgcn_mfma_f32_16x16x32_f16(gh, h1, m1, 0, 0, 0);
        unsigned a00, a01, b00, b01, a10, a11, b10, b11;     // the messages as fp16 pairs (below 2^15 by the scales)
#ifdef TGNN_ABL_EGNOMSGSPLIT
        // (timing ablation: the message words taken as the pair halves -- garbage, minus the message split's 16 instructions per group)
        a00 = __float_as_uint(m0[0]); b00 = __float_as_uint(m0[1]); a01 = __float_as_uint(m0[2]); b01 = __float_as_uint(m0[3]);
        a10 = __float_as_uint(m1[0]); b10 = __float_as_uint(m1[1]); a11 = __float_as_uint(m1[2]); b11 = __float_as_uint(m1[3]);
#else
        split_pair_f16(m0[0], m0[1], a00, b00);
        split_pair_f16(m0[2], m0[3], a01, b01);
        split_pair_f16(m1[0], m1[1], a10, b10);
        split_pair_f16(m1[2], m1[3], a11, b11);
#endif
        Msg r;
        r.a0 = u32x2{a00, a01}; r.b0 = u32x2{b00, b01}; r.a1 = u32x2{a10, a11}; r.b1 = u32x2{b10, b11};
        r.sel = sel0;
        if (!SUM && (meta & kEgRootBit)) {                   // S = diag(max(deg, 1)): s = its float bits for row fj
            asm volatile("" ::: "memory");                   // (a real branch: one group in ~16 takes it)
            const _Float16 dg = (_Float16)__int_as_float(s);
            r.sel = r.sel * dg;
        }
        return r;
    };
    auto fold16 = [&](const Msg &g) {                        // out += S . M, one group: K = 16
        d0 = __builtin_amdgcn_mfma_f32_16x16x16f16(g.sel, __builtin_bit_cast(f16x4, g.b0), d0, 0, 0, 0);
        d1 = __builtin_amdgcn_mfma_f32_16x16x16f16(g.sel, __builtin_bit_cast(f16x4, g.b1), d1, 0, 0, 0);
        d0 = __builtin_amdgcn_mfma_f32_16x16x16f16(g.sel, __builtin_bit_cast(f16x4, g.a0), d0, 0, 0, 0);
        d1 = __builtin_amdgcn_mfma_f32_16x16x16f16(g.sel, __builtin_bit_cast(f16x4, g.a1), d1, 0, 0, 0);
    };
    auto fold32 = [&](const Msg &g, const Msg &k) {          // two groups of one tile: K = 32 (the K = 16 form costs the same 16 cycles)
        using f16x8v = f16x8;
        const f16x4 sg = g.sel, sk = k.sel;
        const f16x8v sel = {sg[0], sg[1], sg[2], sg[3], sk[0], sk[1], sk[2], sk[3]};
        auto cat = [](u32x2 p, u32x2 q) { return __builtin_bit_cast(f16x8v, u32x4{p[0], p[1], q[0], q[1]}); };
        d0 = __builtin_amdgcn_mfma_f32_16x16x32_f16(sel, cat(g.b0, k.b0), d0, 0, 0, 0);
        d1 = __builtin_amdgcn_mfma_f32_16x16x32_f16(sel, cat(g.b1, k.b1), d1, 0, 0, 0);
        d0 = __builtin_amdgcn_mfma_f32_16x16x32_f16(sel, cat(g.a0, k.a0), d0, 0, 0, 0);
        d1 = __builtin_amdgcn_mfma_f32_16x16x32_f16(sel, cat(g.a1, k.a1), d1, 0, 0, 0);
    };
    auto finish_tile = [&](int s) {                          // s: float bits of max(deg, 1) of row fj (-1: row >= n)
        double s0 = 0, s1 = 0, z0 = 0, z1 = 0;
#pragma unroll
        for (int r = 0; r < 4; ++r) {
            const int dg = __shfl(s, 4 * fq + r, 64);        // row 4 fq + r's word
            const bool valid = dg >= 0;
            const float inv = SUM ? unscale : unscale * __builtin_amdgcn_rcpf(__int_as_float(dg));
            float o0 = SUM ? d0[r] * inv : fmaf(d0[r], inv, bias0);
            float o1 = SUM ? d1[r] * inv : fmaf(d1[r], inv, bias1);
            if constexpr (ACT == TGNN_ACT_LEAKY_RELU) {
                o0 = leakyf_(o0);
                o1 = leakyf_(o1);
            }
            const int64_t v = ctile * 16 + 4 * fq + r;
            if (valid) {
                out[v * 32 + fj] = o0;
                out[v * 32 + 16 + fj] = o1;
                if constexpr (SHARD) {                       // the row's copies in the halo message (most rows: none)
                    const int p0 = sh.send_row_ptr[v], p1 = sh.send_row_ptr[v + 1];
                    for (int pp = p0; pp < p1; ++pp) {
                        float *dst = sh.msg + (int64_t)sh.send_row_slot[pp] * 32;
                        dst[fj] = o0;
                        dst[16 + fj] = o1;
                    }
                }
                s0 += (double)o0; z0 += (double)o0 * (double)o0;
                s1 += (double)o1; z1 += (double)o1 * (double)o1;
            }
        }
        bs[0] += s0; bq[0] += z0;
        bs[1] += s1; bq[1] += z1;
        d0 = zero4;
        d1 = zero4;
        ++ctile;
    };
    // two consecutive groups of the stream: one K = 32 fold unless the first one ends its tile
    auto consume_pair = [&](int sa, int ma, int ta, const float4 (&xa)[2], int sb, int mb, int tb, const float4 (&xb)[2]) {
        const Msg ga = stage1(sa, ma, ta, xa);
        const Msg gb = stage1(sb, mb, tb, xb);
#ifdef TGNN_ABL_EGSINGLE
        if (true) {                                          // (timing ablation: every group folded on its own)
#else
        if (ta & kEgRootBit) {                               // wave-uniform
#endif
            fold16(ga);
            finish_tile(sa);
            fold16(gb);
        } else {
            fold32(ga, gb);
        }
        if (tb & kEgRootBit) finish_tile(sb);
    };

    // ---- the group stream, four groups at a time: a four's index words are fetched two rounds ahead, its gathers one
    int s4n, m4n;
    int xs[4], xm[4], xt[4];
    float4 x[4][2];
    {
        int s4, m4;
        load_four(cbeg, s4, m4);
        load_four(cbeg + 4, s4n, m4n);
#pragma unroll
        for (int u = 0; u < 4; ++u) {
            unpack(std::false_type{}, cbeg, u, s4, m4, xs[u], xm[u], xt[u]);
            issue_gather(xs[u], xt[u], x[u]);
        }
    }
    // (the first gathers are in flight: the block's weight image lands behind them)
    {   // weight image: straight copy, all loads of a thread issued before the first LDS store
        const int n4 = (n_types + 1) * kTy / 4;
        for (int i = tid; i < n4; i += 4 * kThreads) {
            float4 v[4];
#pragma unroll
            for (int u = 0; u < 4; ++u) {
                const int ii = i + u * kThreads < n4 ? i + u * kThreads : n4 - 1;
                v[u] = reinterpret_cast<const float4 *>(wimg)[ii];
            }
#pragma unroll
            for (int u = 0; u < 4; ++u)
                if (i + u * kThreads < n4) reinterpret_cast<float4 *>(wl)[i + u * kThreads] = v[u];
        }
        if (tid < 16) {
            f16x4 e;
#pragma unroll
            for (int b = 0; b < 4; ++b) e[b] = (tid >> b & 1) ? (_Float16)1.0f : (_Float16)0.0f;
            lut[tid] = e;
        }
    }

    __syncthreads();
    int base = cbeg;
#ifdef TGNN_ABL_EGNOLOOP
    base = cend;                                             // (timing ablation: what a launch costs without its groups)
#endif
    for (; base + 8 <= cend; base += 4) {                    // steady state: the four gathered in this round lies before cend
        int s4c, m4c;
        load_four(base + 8, s4c, m4c);
#pragma unroll
        for (int u = 0; u < 4; u += 2) {
            consume_pair(xs[u], xm[u], xt[u], x[u], xs[u + 1], xm[u + 1], xt[u + 1], x[u + 1]);
#pragma unroll
            for (int v = u; v < u + 2; ++v) {
                unpack(std::true_type{}, base + 4, v, s4n, m4n, xs[v], xm[v], xt[v]);
                issue_gather(xs[v], xt[v], x[v]);
            }
        }
        s4n = s4c;
        m4n = m4c;
    }
    for (; base < cend; base += 4) {
        int s4c, m4c;
        load_four(base + 8, s4c, m4c);
#pragma unroll
        for (int u = 0; u < 4; u += 2) {
            consume_pair(xs[u], xm[u], xt[u], x[u], xs[u + 1], xm[u + 1], xt[u + 1], x[u + 1]);
#pragma unroll
            for (int v = u; v < u + 2; ++v) {
                unpack(std::false_type{}, base + 4, v, s4n, m4n, xs[v], xm[v], xt[v]);
                issue_gather(xs[v], xt[v], x[v]);
            }
        }
        s4n = s4c;
        m4n = m4c;
    }

    // ---- BN partials of the block: lanes (fj, fq) -> channel 16 m + fj; fold fq, then the waves, in fixed order
    if (bn_partial) {
        __syncthreads();                                     // everybody is done with the weight image
        double *red = reinterpret_cast<double *>(lds);       // [WAVES][64 lanes][4]
        double *mine = red + ((int64_t)wave * 64 + lane) * 4;
        mine[0] = bs[0]; mine[1] = bs[1]; mine[2] = bq[0]; mine[3] = bq[1];
        __syncthreads();
        if (tid < 64) {                                      // tid = which * 32 + channel
            const int which = tid >> 5, ch = tid & 31, m2 = ch >> 4, j = ch & 15;
            double acc = 0;
            for (int w = 0; w < WAVES; ++w)
#pragma unroll
                for (int q = 0; q < 4; ++q) acc += red[((int64_t)w * 64 + q * 16 + j) * 4 + which * 2 + m2];
            if constexpr (SHARD) st_partial_sc1(bn_partial, (int64_t)blockIdx.x * 64 + tid, acc);   // (another block reads the row)
            else bn_partial[(int64_t)blockIdx.x * 64 + tid] = acc;
        }
        if constexpr (SHARD) {
            // two-level fold of the partial rows to the shard's sums (the tree of bn_fold_two_level, which writes a record instead)
            using u32x2_ = __attribute__((ext_vector_type(2))) unsigned int;
            constexpr int kSc1 = 16;
            double *ftot = red + WAVES * 64 * 4;             // (behind the block's own reduction array: eg_lds_bytes)
            unsigned *ticket = reinterpret_cast<unsigned *>(ftot + 64);
            const int np = (int)gridDim.x, g = (int)(blockIdx.x & 15u);
            const __amdgpu_buffer_rsrc_t prs = __builtin_amdgcn_make_buffer_rsrc(bn_partial, 0, (int)0x80000000u, 0x00020000);
            const __amdgpu_buffer_rsrc_t grs = __builtin_amdgcn_make_buffer_rsrc(sh.group_rows, 0, (int)0x80000000u, 0x00020000);
            asm volatile("s_waitcnt vmcnt(0)" ::: "memory");    // the partial row AND the message rows of this block are out
            __syncthreads();
            if (tid == 0) *ticket = __hip_atomic_fetch_add(sh.counter + 1 + g, 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
            __syncthreads();
            if (*ticket == (unsigned)((np - g + 15) / 16) - 1u) {        // (uniform) last of its row group
                if (tid < 64) {
                    double acc = 0.0;
                    for (int u0 = 0; g + u0 * 16 < np; u0 += 16) {
                        u32x2_ v[16];
#pragma unroll
                        for (int u = 0; u < 16; ++u) {
                            const int pp = g + (u0 + u) * 16;
                            v[u] = __builtin_amdgcn_raw_buffer_load_b64(prs, pp < np ? ((uint32_t)pp * 64u + (uint32_t)tid) * 8u : 0x80000000u, 0, kSc1);
                        }
#pragma unroll
                        for (int u = 0; u < 16; ++u)
                            if (g + (u0 + u) * 16 < np) acc += __builtin_bit_cast(double, v[u]);
                    }
                    __builtin_amdgcn_raw_buffer_store_b64(__builtin_bit_cast(u32x2_, acc), grs, ((uint32_t)g * 64u + (uint32_t)tid) * 8u, 0, kSc1);
                }
                asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
                __syncthreads();
                if (tid == 0) {
                    __hip_atomic_store(sh.counter + 1 + g, 0u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
                    *ticket = __hip_atomic_fetch_add(sh.counter, 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
                }
                __syncthreads();
                const int n_groups = np < 16 ? np : 16;
                if (*ticket == (unsigned)n_groups - 1u) {    // (uniform) the last group-finisher: every block's rows are out
                    if (tid < 64) {
                        u32x2_ v[16];
#pragma unroll
                        for (int gg = 0; gg < 16; ++gg)
                            v[gg] = __builtin_amdgcn_raw_buffer_load_b64(grs, gg < n_groups ? ((uint32_t)gg * 64u + (uint32_t)tid) * 8u : 0x80000000u, 0, kSc1);
                        double t = 0.0;
#pragma unroll
                        for (int gg = 0; gg < 16; ++gg)
                            if (gg < n_groups) t += __builtin_bit_cast(double, v[gg]);
                        ftot[tid] = t;
                        sh.sums[tid] = t;
                    }
                    __syncthreads();
                    const float *tf = reinterpret_cast<const float *>(ftot);      // 64 doubles = 4 message rows of 32 floats
                    for (int64_t r = tid >> 5; r < sh.n_msg; r += kThreads / 32) {
                        const int id = sh.msg_idx[r];
                        if (id < 0) sh.msg[r * 32 + (tid & 31)] = tf[(-1 - id) * 32 + (tid & 31)];
                    }
                    if (tid == 0) __hip_atomic_store(sh.counter, 0u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
                }
            }
        }
    }
    if (stamp && tid == 0) atomicMax(stamp + 1, wall_clock64());
}

static size_t eg_lds_bytes(int n_types, int waves) {
    const size_t a = (size_t)(n_types + 1) * kWtTypeF16 * sizeof(float) + 16 * 8;
    const size_t b = (size_t)waves * 64 * 4 * sizeof(double) + 64 * sizeof(double) + 16;   // (+ the SHARD tail's sums and ticket)
    return a > b ? a : b;
}

constexpr size_t kEgMaxLds = 160 * 1024 - 256;

// Block shape (nnconv_eg_plan.h: kLayerFootprints).  Timing switches of the co-residency study (profiles/coresident_stage0.txt):
#if defined(TGNN_ABL_EGW8)                                  // two 8-wave blocks per CU instead of one 16-wave block
constexpr int kEgWaves = 8, kEgOcc = 4, kEgBlocksPerCu = 2;
#elif defined(TGNN_ABL_EGW12)                               // 3 waves per SIMD x 128 registers: 128 left to the other chain
constexpr int kEgWaves = 12, kEgOcc = 4, kEgBlocksPerCu = 1;
#elif defined(TGNN_ABL_EGW16C96)                            // 4 waves per SIMD capped at 96 registers (spills: 124 bytes of scratch)
constexpr int kEgWaves = 16, kEgOcc = 5, kEgBlocksPerCu = 1;
#else
constexpr int kEgWaves = kLayerFootprints[kLayerNnconvEg].waves_per_block, kEgOcc = kSimdVgprs / kLayerFootprints[kLayerNnconvEg].vgpr_cap;
constexpr int kEgBlocksPerCu = 1;
#endif

int nnconv_eg_func_attributes(hipFuncAttributes *attr, int *waves) {
    *waves = kEgWaves;
    return (int)hipFuncGetAttributes(attr, reinterpret_cast<const void *>(nnconv32_eg_kernel<kEgWaves, kEgOcc, TGNN_ACT_LEAKY_RELU>));
}

int launch_nnconv_eg(const float *h, const int32_t *tile_grp_ptr, const int32_t *grp, const float *wimg, int32_t n_types, const float *bias, int64_t n_nodes, int32_t act, float *out,
                     double *bn_partial, int32_t *n_partials_host, hipStream_t s, const unsigned *h_max, const unsigned *root_max,
                     unsigned long long *stamp, const EgShardPack *pack, const float *sum_root_rows) {
    constexpr int WAVES = kEgWaves, OCC = kEgOcc, kBlocksPerCu = kEgBlocksPerCu;
    const bool leaky = act == TGNN_ACT_LEAKY_RELU;
    const bool shard = pack && pack->counter && bn_partial && leaky;
    const bool sum = sum_root_rows != nullptr;               // (the adjoint's form: act, bias, bn_partial and pack are not read)
    auto kern = sum     ? nnconv32_eg_kernel<WAVES, OCC, TGNN_ACT_NONE, false, true>
                : shard ? nnconv32_eg_kernel<WAVES, OCC, TGNN_ACT_LEAKY_RELU, true>
                        : leaky ? nnconv32_eg_kernel<WAVES, OCC, TGNN_ACT_LEAKY_RELU> : nnconv32_eg_kernel<WAVES, OCC, TGNN_ACT_NONE>;
    static LdsOptIn site[4];
    TGNN_CHECK_HIP(opt_in_dynamic_lds(kern, (int)kEgMaxLds, site[sum ? 3 : shard ? 2 : leaky]));
    if (sum) {
        bias = sum_root_rows;
        bn_partial = nullptr;
    }
    EgShard sh{};
    if (shard) sh = EgShard{pack->send_row_ptr, pack->send_row_slot, pack->msg, pack->msg_idx, pack->n_msg, pack->sums, pack->counter, pack->group_rows};
#ifdef TGNN_ABL_EGRES0
    constexpr int reserve = 0;                               // (timing switch: every CU)
#else
    // (CUs left to the collision chain: nnconv_cols.hip.  Re-measured with 12-wave blocks, which leave the aggregate room on
    //  every CU: reserve 0 is still 2.7 % slower than reserve 32 in the step, profiles/coresident_stage0.txt)
    constexpr int reserve = 32;
#endif
    int64_t cap = (int64_t)cus_minus(reserve) * kBlocksPerCu;
    if (const int dbg = g_debug_block_cap[0].load(); dbg > 0) cap = dbg < device_cus() ? dbg : device_cus();
    const int blocks = nnconv_eg_blocks(n_nodes, cap);       // nnconv_eg_plan.h
    kern<<<(unsigned)blocks, WAVES * 64, eg_lds_bytes(n_types, WAVES), s>>>(h, tile_grp_ptr, reinterpret_cast<const int2 *>(grp), wimg,
                                                                            n_types, bias, n_nodes, act, out, bn_partial, h_max, root_max,
                                                                            stamp, sh);
    if (n_partials_host) *n_partials_host = (int32_t)blocks;
    TGNN_CHECK_LAUNCH();
    return TGNN_OK;
}

}  // namespace tgnn

using namespace tgnn;

extern "C" int tgnn_kernel_footprint(int32_t kernel, int32_t n_types, int32_t *out) {
    TGNN_CHECK_ARG(kernel >= 0 && kernel < kLayerKernels && out && n_types >= 0, "kernel index / null pointer");
    hipFuncAttributes attr{};
    int waves = 0, dyn_lds = 0, rc = 0;
    switch (kernel) {
    case kLayerNnconvEg:
        rc = nnconv_eg_func_attributes(&attr, &waves);
        dyn_lds = (int)eg_lds_bytes(n_types, waves);
        break;
    case kLayerMerge: rc = merge_wide_func_attributes(&attr, &waves); break;
    default: rc = gin32_func_attributes(kernel, &attr, &waves); break;
    }
    if (rc != 0) {
        set_error("tgnn_kernel_footprint: hipFuncGetAttributes failed (%d)", rc);
        return TGNN_ERR_LAUNCH;
    }
    out[0] = waves;                                          // waves of a block as the general schedule launches it
    out[1] = (waves + kEgSimds - 1) / kEgSimds;              // ... of them on one SIMD
    out[2] = kLayerFootprints[kernel].vgpr_cap;              // what __launch_bounds__ pins the kernel to (nnconv_eg_plan.h)
    out[3] = attr.numRegs;                                   // what the runtime reports for the code object that is loaded
    out[4] = (int32_t)attr.sharedSizeBytes + dyn_lds;        // LDS of a block, static + dynamic at n_types edge types
    out[5] = attr.maxThreadsPerBlock;
    return TGNN_OK;
}

extern "C" int tgnn_nnconv_mean_eg_fwd(const float *h, int64_t ldh, int64_t n_src_rows, const int32_t *tile_grp_ptr,
                                       const int32_t *grp, const float *wtab, int32_t n_types,
                                       const float *root, const float *bias, int64_t n_nodes, int32_t act, float *out,
                                       float *wimg_scratch, uint32_t *bounds_scratch, double *bn_partial,
                                       int32_t *n_partials_host, tgnn_stream_t stream) {
    DeviceGuard guard__(stream);
    TGNN_CHECK_ARG(n_nodes >= 1 && n_src_rows >= n_nodes, "shape");
    TGNN_CHECK_ARG(act == TGNN_ACT_NONE || act == TGNN_ACT_LEAKY_RELU, "activation");
    TGNN_CHECK_ARG(h && tile_grp_ptr && grp && root && bias && out && wimg_scratch && bounds_scratch, "null pointer");
    TGNN_CHECK_ARG(n_types == 0 || wtab, "null weight table");
    TGNN_CHECK_ARG(ldh == 32 && ((uintptr_t)h % 16) == 0 && ((uintptr_t)wimg_scratch % 16) == 0 && ((uintptr_t)root % 16) == 0,
                   "alignment / packed rows");
    TGNN_CHECK_ARG(n_src_rows * 128 < ((int64_t)1 << 31), "source rows must lie within 2 GB of h");
    if ((size_t)(n_types + 1) * kWtTypeF16 * sizeof(float) + 16 * 8 > kEgMaxLds) {
        set_error("tgnn_nnconv_mean_eg_fwd: %d edge types do not fit the LDS weight image", n_types);
        return TGNN_ERR_UNSUPPORTED;
    }
    hipStream_t s = static_cast<hipStream_t>(stream);
    // bounds: [0] = max |h| over every row that can be gathered, [1] = max |root|
    launch_forward_scales(bounds_scratch, 2, &root, 1, bounds_scratch + 1, nullptr, 0, nullptr, s);
    launch_absmax(h, n_src_rows * 32, bounds_scratch, s);
    launch_nnconv_weight_image(wtab, &root, n_types, 1, wimg_scratch, s, bounds_scratch + 1, kEgImageScale);
    return launch_nnconv_eg(h, tile_grp_ptr, grp, wimg_scratch, n_types, bias, n_nodes, act, out, bn_partial,
                            n_partials_host, s, bounds_scratch, bounds_scratch + 1, nullptr, nullptr, nullptr);
}
