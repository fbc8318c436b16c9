// NNConv(aggr="mean"), network_width 64, fp32 in and out, over the layout's edge groups on the matrix cores of gfx950.
//
// Reference semantics: GraphConv.forward (graph_networks/layers/edge_conv.py:24-27 of the reference) over PyG 1.3.2 NNConv:
//     out[v] = mean_{e: dst_e = v} h[src_e] . W_{type_e}  +  h[v] . root + bias  (+ LeakyReLU)
//
// The op of nnconv_eg.hip (width 32) at the width the generic kernel served so far (one thread per output, the [T][64][64] table
// read through L2: 4.5 ms per layer at 100 000 nodes), in the shape of its bf16-storage sibling (bf16_path.hip:
// nnconv64_bf16_eg_kernel) over the SAME structure (graph_prep.hip: nnconv_eg_kernel; tile_grp_ptr / grp unchanged):
//     M [16 edges x 32]   = G [16 edges x 64] . W_t[:, half]   fp16-pair split of rows and weights, 3 terms:
//                                                               v_mfma_f32_16x16x32_f16 x 12 (2 N blocks x 2 K chunks x 3)
//     out[16 rows x 32]  += S [16 rows x 16 edges] . M          S: the group's 0 / 1 selection matrix (exact in fp16); M kept as an
//                                                               fp16 PAIR (hi + lo: 2^-22, nothing of the split is lost):
//                                                               v_mfma_f32_16x16x16_f16 x 4
// The accumulator layout of the first product (lane (j, q): edges 4 q + r, channel j) is the B-operand layout of the second.
// The root group (the last of a tile; W = root, S = I): the edge sum is turned into the mean first (fp32 reciprocal of
// max(deg, 1): no in-degree limit in the kernel), then the root product joins.
//
// LDS is the design constraint: a type's 64 x 64 fp16-pair image is 16 KiB, and 160 KiB hold 9 of them -- not the 13 types + root
// of a complete tile graph.  A block therefore walks its tiles TWICE, once per half of the output columns, with the 8 KiB
// half-images of all entries resident (T <= 18: nnconv64_eg_plan.h); the second walk's gathers hit the rows the first one
// brought into the L2 of the same XCD.  8 waves per block (two per SIMD, 256 registers each: four groups' gathers -- 16 x 16-byte
// loads per lane -- stay in flight beside the operand fragments).
//
// Scales (powers of two, as nnconv_eg.hip): rows by sx with max |h| sx < 2^9, weights by nnconv_weight_scale(max |root|) 2^-15
// (every weight below 1), so that the 64 products of a message stay below 2^15; 2^3 <= max |h| < 2^9: rows go in unscaled.
#include <type_traits>

#include "nnconv64_eg.h"
#include "split_pair_f16.h"

namespace tgnn {

using f32x4 = __attribute__((ext_vector_type(4))) float;
using f16x8 = tgnn_f16x8;
using f16x4 = __attribute__((ext_vector_type(4))) _Float16;
using u32x4 = __attribute__((ext_vector_type(4))) unsigned;
using u32x2 = __attribute__((ext_vector_type(2))) unsigned;

constexpr int kEg64RootBit = 1 << 8;                        // meta = type | root << 8 (graph_prep.hip: kEgRoot)
constexpr int kEg64ExtraLog2 = 6;                           // h . sx < 2^9: 64 products with weights below 1 stay below 2^15
constexpr int kC64 = 64;

// wtab [T][64][64] (+ root [64][64] as entry T), element (k, o) = weight of input k for output o -> fp16-pair image
//   [entry][half o >> 5][plane (hi, lo)][N block (o >> 4) & 1][K chunk k >> 5][lane 16 ((k >> 3) & 3) + (o & 15)][k & 7]
// every weight multiplied by nnconv_weight_scale(max |root|) 2^-15 first.  grid = (T + 1, layers); every block takes the bound of
// its layer's root itself (16 KiB), block 0 of a layer leaves it in root_max[layer] for the kernel's unscale.
struct RootPtrs64Eg {
    const float *p[kMaxDepth];
};
__global__ __launch_bounds__(256) void nnconv64_eg_image_kernel(const float *__restrict__ wtab_all, RootPtrs64Eg roots, int n_types,
                                                                float *__restrict__ wimg_all, unsigned *__restrict__ root_max) {
    __shared__ float wave_max[4];
    const int t = blockIdx.x, layer = blockIdx.y, tid = threadIdx.x;
    const float *root = roots.p[layer];
    float m = 0.f;
#pragma unroll
    for (int u = 0; u < 4; ++u) {
        const float4 v = reinterpret_cast<const float4 *>(root)[tid + 256 * u];
        m = fmaxf(fmaxf(m, fmaxf(fabsf(v.x), fabsf(v.y))), fmaxf(fabsf(v.z), fabsf(v.w)));
    }
#pragma unroll
    for (int d = 32; d >= 1; d >>= 1) m = fmaxf(m, __shfl_xor(m, d, 64));
    if ((tid & 63) == 0) wave_max[tid >> 6] = m;
    __syncthreads();
    const unsigned rm_bits = __float_as_uint(fmaxf(fmaxf(wave_max[0], wave_max[1]), fmaxf(wave_max[2], wave_max[3])));
    if (t == 0 && tid == 0) root_max[layer] = rm_bits;
    const float wscale = nnconv_weight_scale(rm_bits) * kEgImageScale;
    const float *src = t < n_types ? wtab_all + ((int64_t)layer * n_types + t) * (kC64 * kC64) : root;
    _Float16 *dst = reinterpret_cast<_Float16 *>(wimg_all + ((int64_t)layer * (n_types + 1) + t) * kEg64TypeFloats);
    for (int r = tid; r < kC64 * kC64; r += 256) {
        const int k = r >> 6, o = r & 63;
        const float v = src[r] * wscale;                     // (a power of two: exact)
        const _Float16 hi = (_Float16)v;
        const _Float16 lo = (_Float16)(v - (float)hi);
        const int half = o >> 5, nb = (o >> 4) & 1, kc = k >> 5, lane = 16 * ((k >> 3) & 3) + (o & 15);
        const int at = ((((half * 2 + 0) * 2 + nb) * 2 + kc) * 64 + lane) * 8 + (k & 7);
        dst[at] = hi;
        dst[at + 2 * 2 * 64 * 8] = lo;                       // plane 1
    }
}

// SUM (the adjoint's input gradient, nnconv_bwd_eg.hip: this op over the TRANSPOSED graph with the transposed table): the edge SUM
// instead of the mean, no bias, no activation, no BatchNorm partials; the root group's rows come from a second array, passed in
// `bias`'s place ([n rows][64] packed like h: dz where h is g = dz / deg).  The other instantiations keep their code.
template <int WAVES, int ACT, bool SUM = false>
__global__ __launch_bounds__(WAVES * 64) void nnconv64_eg_kernel(
    const float *__restrict__ h, uint32_t h_bytes, const int *__restrict__ tile_grp_ptr, const int2 *__restrict__ grp,
    const float *__restrict__ wimg, int n_types, const float *__restrict__ bias, int64_t n, float *__restrict__ out,
    double *__restrict__ bn_partial, const unsigned *__restrict__ h_max, const unsigned *__restrict__ root_max) {
    extern __shared__ __attribute__((aligned(16))) float lds[];
    float *wl = lds;                                        // [(T+1)][2 planes][2 N blocks][2 K chunks][64 lanes] x 8 fp16
    f16x4 *lut = reinterpret_cast<f16x4 *>(lds + (n_types + 1) * kEg64HalfFloats);   // [16]: 4 selection bits -> 4 fp16 of 0 / 1
    const unsigned hm_bits = *h_max, hm_exp = (hm_bits >> 23) & 0xffu;               // max |h| < 2^(hm_exp - 126)
    // no scale where the rows are in range as they are: 2^3 <= max |h| < 2^9 (nnconv_eg.hip; one bit less for 64 products)
    const bool unit = hm_exp >= 130 && hm_exp <= 135;
    const float sx = unit ? 1.0f : pow2_scale_for(hm_bits, kEg64ExtraLog2);
    const float unscale = 1.0f / (sx * nnconv_weight_scale(*root_max) * kEgImageScale);   // (powers of two: exact)
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int fj = lane & 15, fq = lane >> 4;
    constexpr int kThreads = WAVES * 64;

    // ---- this wave's run of 16-row tiles
    const uint64_t n_tiles = (uint64_t)((n + 15) / 16);
    const uint64_t n_waves = (uint64_t)gridDim.x * WAVES, wg = (uint64_t)blockIdx.x * WAVES + wave;
    const int64_t t0 = (int64_t)(n_tiles * wg / n_waves), t1 = (int64_t)(n_tiles * (wg + 1) / n_waves);
    const int cbeg = __builtin_amdgcn_readfirstlane(tile_grp_ptr[t0]);
    const int cend = __builtin_amdgcn_readfirstlane(tile_grp_ptr[t1]);

    const __amdgpu_buffer_rsrc_t h_rsrc =
        __builtin_amdgcn_make_buffer_rsrc(const_cast<float *>(h), 0, (int)h_bytes, 0x00020000);   // beyond the rows: zeros
    const __amdgpu_buffer_rsrc_t own_rsrc =
        SUM ? __builtin_amdgcn_make_buffer_rsrc(const_cast<float *>(bias), 0, (int)h_bytes, 0x00020000) : h_rsrc;
    const uint32_t fq_bytes = (uint32_t)fq * 32u;
    auto load_four = [&](int p, int &s4, int &m4) {         // groups p .. p+3: lane (fj, fq) <- group p + fq, word fj
        const int pc = p < cend ? p : cbeg;                  // (never past the wave's share)
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
    const f32x4 zero4 = {0.f, 0.f, 0.f, 0.f};
    double bs[4] = {0, 0, 0, 0}, bq[4] = {0, 0, 0, 0};       // BN sums of channel 16 mb + fj over rows 4 fq .. 4 fq + 3

    // ---- one walk over the wave's groups for the output columns 32 half .. 32 half + 31
    auto walk = [&](auto half_c) {
        constexpr int half = decltype(half_c)::value;
        int64_t gtile = t0, ctile = t0;                      // tile of the group the gather stage / the fold is at
        auto own_off_of = [&](int64_t tile) -> uint32_t {
            const int64_t r = tile * 16 + fj;
            return r < n ? (uint32_t)r * 256u + fq_bytes : 0x80000000u;
        };
        uint32_t own_off = own_off_of(gtile);
        // lane (fj, fq) of the A operand: row fj, K chunk kc -> channels 32 kc + 8 fq .. + 7 (two 16-byte loads)
        auto issue_gather = [&](int s, int meta, float4 (&x)[4]) {
            const bool root = (meta & kEg64RootBit) != 0;    // wave-uniform
            const uint32_t off = root ? own_off : ((uint32_t)s << 8) + fq_bytes;   // s = -1: beyond the rows, loads zeros
            if (SUM && root) {                               // (wave-uniform) the root rows of the sum form: the second array
#pragma unroll
                for (int kc = 0; kc < 2; ++kc) {
                    x[2 * kc] = __builtin_bit_cast(float4, __builtin_amdgcn_raw_buffer_load_b128(own_rsrc, off + 128u * kc, 0, 0));
                    x[2 * kc + 1] = __builtin_bit_cast(float4, __builtin_amdgcn_raw_buffer_load_b128(own_rsrc, off + 128u * kc + 16u, 0, 0));
                }
            } else {
#pragma unroll
                for (int kc = 0; kc < 2; ++kc) {
                    x[2 * kc] = __builtin_bit_cast(float4, __builtin_amdgcn_raw_buffer_load_b128(h_rsrc, off + 128u * kc, 0, 0));
                    x[2 * kc + 1] = __builtin_bit_cast(float4, __builtin_amdgcn_raw_buffer_load_b128(h_rsrc, off + 128u * kc + 16u, 0, 0));
                }
            }
            if (root) {
                ++gtile;
                own_off = own_off_of(gtile);
            }
        };
        f32x4 d[2] = {zero4, zero4};                         // out tile: rows 4 fq + r, channel 32 half + 16 nb + fj
        const float bias_r[2] = {SUM ? 0.f : bias[32 * half + fj], SUM ? 0.f : bias[32 * half + 16 + fj]};

        // a group: its messages M = G . W_t[:, half] as fp16 pairs, folded into the tile by the selection operand
        auto consume = [&](int s, int m, int meta, const float4 (&x)[4]) {
            const int t = meta & 0xff;
            const bool root = (meta & kEg64RootBit) != 0;    // wave-uniform
            const f16x8 *wp = reinterpret_cast<const f16x8 *>(wl + t * kEg64HalfFloats) + lane;   // lane order: conflict-free
            f16x4 sel = lut[(m >> (4 * fq)) & 15];           // S[row fj][edges 4 fq .. 4 fq + 3]
            f16x8 gh[2], gl[2];
#pragma unroll
            for (int kc = 0; kc < 2; ++kc) {
                const float4 xa = x[2 * kc], xb = x[2 * kc + 1];
                unsigned h0, h1, h2, h3, l0, l1, l2, l3;
                if (unit) {                                  // wave-uniform
                    split_pair_f16(xa.x, xa.y, h0, l0);
                    split_pair_f16(xa.z, xa.w, h1, l1);
                    split_pair_f16(xb.x, xb.y, h2, l2);
                    split_pair_f16(xb.z, xb.w, h3, l3);
                } else {
                    split_pair_f16(xa.x, xa.y, sx, h0, l0);
                    split_pair_f16(xa.z, xa.w, sx, h1, l1);
                    split_pair_f16(xb.x, xb.y, sx, h2, l2);
                    split_pair_f16(xb.z, xb.w, sx, h3, l3);
                }
                gh[kc] = __builtin_bit_cast(f16x8, u32x4{h0, h1, h2, h3});
                gl[kc] = __builtin_bit_cast(f16x8, u32x4{l0, l1, l2, l3});
            }
            if (!SUM && root) {                              // the edge sum of rows 4 fq + r -> their mean; then S = I
#pragma unroll
                for (int r = 0; r < 4; ++r) {
                    const int dg = __shfl(s, 4 * fq + r, 64);    // float bits of max(deg, 1) of row 4 fq + r, -1 = row >= n
                    const float inv = dg >= 0 ? 1.0f / __int_as_float(dg) : 0.f;
                    d[0][r] *= inv;
                    d[1][r] *= inv;
                }
            }
#pragma unroll
            for (int nb = 0; nb < 2; ++nb) {
                // fragment (plane, nb, kc) at 64 x 16 B x ((plane * 2 + nb) * 2 + kc)
                const f16x8 wh0 = wp[(nb * 2 + 0) * 64], wh1 = wp[(nb * 2 + 1) * 64];
                const f16x8 wl0 = wp[((2 + nb) * 2 + 0) * 64], wl1 = wp[((2 + nb) * 2 + 1) * 64];
                f32x4 acc = __builtin_amdgcn_mfma_f32_16x16x32_f16(gh[0], wl0, zero4, 0, 0, 0);   // hi . lo
                acc = __builtin_amdgcn_mfma_f32_16x16x32_f16(gh[1], wl1, acc, 0, 0, 0);
                acc = __builtin_amdgcn_mfma_f32_16x16x32_f16(gl[0], wh0, acc, 0, 0, 0);           // lo . hi
                acc = __builtin_amdgcn_mfma_f32_16x16x32_f16(gl[1], wh1, acc, 0, 0, 0);
                acc = __builtin_amdgcn_mfma_f32_16x16x32_f16(gh[0], wh0, acc, 0, 0, 0);           // hi . hi
                acc = __builtin_amdgcn_mfma_f32_16x16x32_f16(gh[1], wh1, acc, 0, 0, 0);
                unsigned a0, a1, b0, b1;                     // the messages as an fp16 pair (below 2^15 by the scales)
                split_pair_f16(acc[0], acc[1], a0, b0);
                split_pair_f16(acc[2], acc[3], a1, b1);
                d[nb] = __builtin_amdgcn_mfma_f32_16x16x16f16(sel, __builtin_bit_cast(f16x4, u32x2{b0, b1}), d[nb], 0, 0, 0);
                d[nb] = __builtin_amdgcn_mfma_f32_16x16x16f16(sel, __builtin_bit_cast(f16x4, u32x2{a0, a1}), d[nb], 0, 0, 0);
            }
            if (root) {                                      // the tile is complete
#pragma unroll
                for (int nb = 0; nb < 2; ++nb) {
                    double sum = 0, sq = 0;
#pragma unroll
                    for (int r = 0; r < 4; ++r) {
                        const int dg = __shfl(s, 4 * fq + r, 64);
                        float o = SUM ? d[nb][r] * unscale : fmaf(d[nb][r], unscale, bias_r[nb]);
                        if constexpr (ACT == TGNN_ACT_LEAKY_RELU) o = leakyf_(o);
                        if (dg >= 0) {                       // row < n
                            const int64_t v = ctile * 16 + 4 * fq + r;
                            out[v * kC64 + 32 * half + 16 * nb + fj] = o;
                            sum += (double)o;
                            sq += (double)o * (double)o;
                        }
                    }
                    bs[2 * half + nb] += sum;
                    bq[2 * half + nb] += sq;
                    d[nb] = zero4;
                }
                ++ctile;
            }
        };

        // ---- the group stream, four groups at a time: a four's index words are fetched two rounds ahead, its gathers one
        int s4n, m4n;
        int xs[4], xm[4], xt[4];
        float4 x[4][4];
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
        // (the first gathers are in flight: this half's weight image lands behind them)
        if (half) __syncthreads();                           // every wave is done with the other half's image
        {
            const int n4 = (n_types + 1) * (kEg64HalfFloats / 4);
            const float4 *src = reinterpret_cast<const float4 *>(wimg);
            auto src_at = [&](int i) {                       // 16-byte word i of the half-images -> of the whole images
                constexpr int kH4 = kEg64HalfFloats / 4;
                return (i / kH4) * 2 * kH4 + half * kH4 + i % kH4;
            };
#pragma unroll 4
            for (int i = tid; i < n4; i += kThreads) reinterpret_cast<float4 *>(wl)[i] = src[src_at(i)];   // (n4 % kThreads == 0)
            if (tid < 16) {
                f16x4 e;
#pragma unroll
                for (int b = 0; b < 4; ++b) e[b] = (tid >> b & 1) ? (_Float16)1.0f : (_Float16)0.0f;
                lut[tid] = e;
            }
        }
        __syncthreads();
        int base = cbeg;
        for (; base + 8 <= cend; base += 4) {                // steady state: the four gathered in this round lies before cend
            int s4c, m4c;
            load_four(base + 8, s4c, m4c);
#pragma unroll
            for (int u = 0; u < 4; ++u) {
                consume(xs[u], xm[u], xt[u], x[u]);
                unpack(std::true_type{}, base + 4, u, s4n, m4n, xs[u], xm[u], xt[u]);
                issue_gather(xs[u], xt[u], x[u]);
            }
            s4n = s4c;
            m4n = m4c;
        }
        for (; base < cend; base += 4) {
            int s4c, m4c;
            load_four(base + 8, s4c, m4c);
#pragma unroll
            for (int u = 0; u < 4; ++u) {
                consume(xs[u], xm[u], xt[u], x[u]);
                unpack(std::false_type{}, base + 4, u, s4n, m4n, xs[u], xm[u], xt[u]);
                issue_gather(xs[u], xt[u], x[u]);
            }
            s4n = s4c;
            m4n = m4c;
        }
    };
    walk(std::integral_constant<int, 0>{});
    walk(std::integral_constant<int, 1>{});

    // ---- BN partials of the block, [2][64]: lanes (fj, fq) -> channel 16 mb + fj; fold fq, then the waves, in fixed order
    if (bn_partial) {
        __syncthreads();                                     // everybody is done with the weight image
        double *red = reinterpret_cast<double *>(lds);       // [WAVES][64 lanes][8]
        double *mine = red + ((int64_t)wave * 64 + lane) * 8;
#pragma unroll
        for (int mb = 0; mb < 4; ++mb) { mine[mb] = bs[mb]; mine[4 + mb] = bq[mb]; }
        __syncthreads();
        if (tid < 128) {                                     // tid = which * 64 + channel
            const int which = tid >> 6, ch = tid & 63, mb = ch >> 4, j = ch & 15;
            double acc = 0;
            for (int w = 0; w < WAVES; ++w)
#pragma unroll
                for (int q = 0; q < 4; ++q) acc += red[((int64_t)w * 64 + q * 16 + j) * 8 + which * 4 + mb];
            bn_partial[(int64_t)blockIdx.x * 128 + tid] = acc;
        }
    }
}

void launch_nnconv64_eg_images(const float *wtab_all, const float *const *roots, int n_types, int depth, float *wimg_all,
                               unsigned *root_max, hipStream_t s) {
    RootPtrs64Eg rp{};
    for (int i = 0; i < depth; ++i) rp.p[i] = roots[i];
    nnconv64_eg_image_kernel<<<dim3(n_types + 1, depth), 256, 0, s>>>(wtab_all, rp, n_types, wimg_all, root_max);
}

int launch_nnconv64_eg(const float *h, int64_t n_src_rows, const int32_t *tile_grp_ptr, const int32_t *grp, const float *wimg,
                       int32_t n_types, const float *bias, int64_t n_nodes, int32_t act, float *out, double *bn_partial,
                       int32_t *n_partials_host, hipStream_t s, const unsigned *h_max, const unsigned *root_max,
                       const float *sum_root_rows) {
    constexpr int WAVES = kEg64Waves;
    const bool leaky = act == TGNN_ACT_LEAKY_RELU;
    const bool sum = sum_root_rows != nullptr;               // (the adjoint's form: act, bias and bn_partial are not read)
    auto kern = sum ? nnconv64_eg_kernel<WAVES, TGNN_ACT_NONE, true>
                    : leaky ? nnconv64_eg_kernel<WAVES, TGNN_ACT_LEAKY_RELU> : nnconv64_eg_kernel<WAVES, TGNN_ACT_NONE>;
    static LdsOptIn site[3];
    TGNN_CHECK_HIP(opt_in_dynamic_lds(kern, (int)kEg64MaxLds, site[sum ? 2 : leaky]));
    if (sum) {
        bias = sum_root_rows;
        bn_partial = nullptr;
    }
    const int64_t n_tiles = (n_nodes + 15) / 16;
    int64_t blocks = (n_tiles + WAVES - 1) / WAVES;          // at least one tile per wave
    const int64_t cap = cus_minus(32);                       // (CUs left to the collision chain, as in the width-32 path)
    if (blocks > cap) blocks = cap;
    if (blocks < 1) blocks = 1;
    kern<<<(unsigned)blocks, WAVES * 64, nnconv64_eg_lds_bytes(n_types, WAVES), s>>>(
        h, (uint32_t)(n_src_rows * 256), tile_grp_ptr, reinterpret_cast<const int2 *>(grp), wimg, n_types, bias, n_nodes, out, bn_partial,
        h_max, root_max);
    if (n_partials_host) *n_partials_host = (int32_t)blocks;
    TGNN_CHECK_LAUNCH();
    return TGNN_OK;
}

}  // namespace tgnn

using namespace tgnn;

extern "C" int32_t tgnn_nnconv64_eg_max_types(void) { return nnconv64_eg_max_types(); }
extern "C" size_t tgnn_nnconv64_eg_image_floats(int32_t n_types) { return (size_t)(n_types < 0 ? 0 : n_types + 1) * kEg64TypeFloats; }

extern "C" int tgnn_nnconv64_mean_eg_fwd(const float *h, int64_t ldh, int64_t n_src_rows, const int32_t *tile_grp_ptr,
                                         const int32_t *grp, const float *wtab, int32_t n_types, const float *root,
                                         const float *bias, int64_t n_nodes, int32_t act, float *out, float *wimg_scratch,
                                         uint32_t *bounds_scratch, double *bn_partial, int32_t *n_partials_host,
                                         tgnn_stream_t stream) {
    DeviceGuard guard__(stream);
    TGNN_CHECK_ARG(n_nodes >= 1 && n_src_rows >= n_nodes, "shape");
    TGNN_CHECK_ARG(act == TGNN_ACT_NONE || act == TGNN_ACT_LEAKY_RELU, "activation");
    TGNN_CHECK_ARG(h && tile_grp_ptr && grp && root && bias && out && wimg_scratch && bounds_scratch, "null pointer");
    TGNN_CHECK_ARG(n_types >= 0 && (n_types == 0 || wtab), "null weight table");
    TGNN_CHECK_ARG(ldh == 64 && ((uintptr_t)h % 16) == 0 && ((uintptr_t)wimg_scratch % 16) == 0 && ((uintptr_t)root % 16) == 0,
                   "alignment / packed rows");
    TGNN_CHECK_ARG(n_src_rows * 256 < ((int64_t)1 << 31), "source rows must lie within 2 GB of h");
    if (n_types > nnconv64_eg_max_types()) {
        set_error("tgnn_nnconv64_mean_eg_fwd: %d edge types do not fit the LDS weight image (max %d)", n_types, nnconv64_eg_max_types());
        return TGNN_ERR_UNSUPPORTED;
    }
    hipStream_t s = static_cast<hipStream_t>(stream);
    // bounds: [0] = max |h| over every row that can be gathered, [1] = max |root| (left by the image kernel)
    TGNN_CHECK_HIP(hipMemsetAsync(bounds_scratch, 0, 2 * sizeof(uint32_t), s));
    launch_absmax(h, n_src_rows * 64, bounds_scratch, s);
    launch_nnconv64_eg_images(wtab, &root, n_types, 1, wimg_scratch, bounds_scratch + 1, s);
    return launch_nnconv64_eg(h, n_src_rows, tile_grp_ptr, grp, wimg_scratch, n_types, bias, n_nodes, act, out, bn_partial,
                              n_partials_host, s, bounds_scratch, bounds_scratch + 1, nullptr);
}
