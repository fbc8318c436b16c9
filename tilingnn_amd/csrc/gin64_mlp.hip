// GINConv's MLP at network_width 64, fp32 in and out, on the matrix cores of gfx950 (the width-64 sibling of gin.hip's
// gin32_mlp_kernel; reference: CollConv.forward, graph_networks/layers/coll_conv.py:24-27):
//   out[v] = act( sigmoid(W3 sigmoid(W2 sigmoid(W1 z[v] + b1) + b2) + b3) ),   W1 [32 x 64], W2 [64 x 32], W3 [64 x 64]
// on the aggregate z [N][64] that gin_aggregate_kernel<64> writes (the previous layer's BatchNorm folded in there).
//
// The shape is gin32_mlp_kernel's:
//   * the TRANSPOSED product H^T = W . Z^T on v_mfma_f32_16x16x32_bf16 (A = weights, B = activations): lane (n = lane & 15,
//     q = lane >> 4) holds features 16 mb + 4 q + r (r = 0 .. 3) of batch row n for M block mb, and two M blocks are the 8 values
//     per lane the B operand of the next layer takes when that layer's K order is kf(q, e) = 4 q + e (e < 4), 16 + 4 q + (e - 4)
//     (e >= 4), + 32 for the second K step -- the weight images are stored in that order, no LDS round trip for activations;
//   * every fp32 operand split exactly into three bf16 pieces, six cross terms, smallest first (forward_persist.h: small_mma6 =
//     gin.hip: gin_mma6; tgnn_common.h: split3_trunc);
//   * layer 1: 2 M blocks x 2 K steps in natural order (Z straight from memory, one tile ahead), layer 2: 4 M blocks, layer 3:
//     4 M blocks x 2 K steps: 24 + 24 + 48 = 96 matrix instructions per 16-row tile;
//   * the output sigmoid is sigmoid_out_f32 (the BatchNorm behind this kernel amplifies every ulp: see gin.hip);
//   * 8 waves, persistent, a contiguous run of tiles per wave (gin64_plan.h: gin64_tile_share, tested on the host).
// Where the 48 weight fragments live: in the LDS image, re-read every tile (48 ds_read_b128 per lane and tile).  With W1 / W2
// in registers and W3 from LDS (228 registers) the kernel measured 27.0 against 27.4 us at 100 000 nodes and the forward the same
// within its spread; all 48 in registers (192 beside 64 of BatchNorm sums) spill.  DESIGN.md section 28.
// Layer 1 -- the one layer whose operand has no bound -- adds the five small cross terms of BOTH K steps before the two hi . hi
// products, so that the small terms meet a small accumulator: a row with 500 in-edges behind a BatchNorm has sum |w z| ~ 650,
// and with the six terms of a step together it came out 1.4e-6 of the output's max-norm off the fp64 oracle (now 2.3e-7).
// BatchNorm sums: fp64 per lane, folded in a fixed order (lane butterfly, then the waves in ascending order): bit-reproducible.
#include "forward_persist.h"
#include "gin64_mlp.h"

namespace tgnn {

__device__ __forceinline__ int gin64_kf(int q, int e) { return e < 4 ? 4 * q + e : 16 + 4 * q + (e - 4); }

// acc += the five small cross terms of W . X over one K step of 32, smallest first (the sixth, hi . hi: gin64_mma_hh)
__device__ __forceinline__ f32x4 gin64_mma5(const bf16x8 *wpl, int plane_stride, const bf16x8 (&x)[3], f32x4 acc) {
    const bf16x8 w0 = wpl[0], w1 = wpl[plane_stride], w2 = wpl[2 * plane_stride];
    acc = __builtin_amdgcn_mfma_f32_16x16x32_bf16(w2, x[0], acc, 0, 0, 0);   // lo . hi
    acc = __builtin_amdgcn_mfma_f32_16x16x32_bf16(w0, x[2], acc, 0, 0, 0);   // hi . lo
    acc = __builtin_amdgcn_mfma_f32_16x16x32_bf16(w1, x[1], acc, 0, 0, 0);   // mid . mid
    acc = __builtin_amdgcn_mfma_f32_16x16x32_bf16(w1, x[0], acc, 0, 0, 0);   // mid . hi
    acc = __builtin_amdgcn_mfma_f32_16x16x32_bf16(w0, x[1], acc, 0, 0, 0);   // hi . mid
    return acc;
}
__device__ __forceinline__ f32x4 gin64_mma_hh(const bf16x8 *wpl, const bf16x8 (&x)[3], f32x4 acc) {
    return __builtin_amdgcn_mfma_f32_16x16x32_bf16(wpl[0], x[0], acc, 0, 0, 0);   // hi . hi
}

__global__ __launch_bounds__(kGin64Threads, 2) void gin64_mlp_kernel(
    const float *__restrict__ z, const float *__restrict__ w1, const float *__restrict__ b1, const float *__restrict__ w2,
    const float *__restrict__ b2, const float *__restrict__ w3, const float *__restrict__ b3, int64_t n, int act,
    float *__restrict__ out, double *__restrict__ bn_partial) {
    // weight images: the A fragment of lane (i, q) is one ds_read_b128
    __shared__ bf16x8 W1s[3 * 2 * 2 * 64];      // [plane][M block 2][K step 2][i 16][q 4], K = 64 in natural order 32 ks + 8 q + e
    __shared__ bf16x8 W2s[3 * 4 * 64];          // [plane][M block 4][..], K = 32 in kf order
    __shared__ bf16x8 W3s[3 * 4 * 2 * 64];      // [plane][M block 4][K step 2][..], K = 64 in kf order
    __shared__ __attribute__((aligned(16))) float Bs[160];   // b1 | b2 | b3
    __shared__ double red[kGin64Waves * 128];
    constexpr int kP1 = 2 * 2 * 64, kP2 = 4 * 64, kP3 = 4 * 2 * 64;   // plane strides
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int fn = lane & 15, fq = lane >> 4;

    const Gin64Tiles share = gin64_tile_share(n, (int)gridDim.x, (int)blockIdx.x, wave);
    const int64_t t0 = share.t0, t1 = share.t1;

    // Z rows of a tile: lane (n, q) reads floats 32 ks + 8 q .. + 7 of row n for the two K steps; one tile ahead
    auto load_z = [&](int64_t tile, float4 (&zin)[4]) {
        int64_t zr = tile * 16 + fn;                        // clamped, unconditional: rows >= n are masked at the store
        zr = zr < n ? zr : n - 1;
        const float4 *pz = reinterpret_cast<const float4 *>(z + zr * 64 + 8 * fq);
        zin[0] = pz[0];
        zin[1] = pz[1];
        zin[2] = pz[8];
        zin[3] = pz[9];
    };
    float4 zin[4];
    load_z(t0 < t1 ? t0 : 0, zin);                          // in flight while the weight images are built

    for (int i = tid; i < 2 * 2 * 64; i += kGin64Threads) { // item = (M block, K step, i, q): 8 weights
        const int mb = i >> 7, ks = (i >> 6) & 1, ii = (i >> 2) & 15, q = i & 3;
        float x[8];
#pragma unroll
        for (int e = 0; e < 8; ++e) x[e] = w1[(16 * mb + ii) * 64 + 32 * ks + 8 * q + e];
        const int o = (mb * 2 + ks) * 64 + ii * 4 + q;
        split3_trunc(x, W1s[o], W1s[kP1 + o], W1s[2 * kP1 + o]);
    }
    for (int i = tid; i < 4 * 64; i += kGin64Threads) {     // item = (M block, i, q)
        const int mb = i >> 6, ii = (i >> 2) & 15, q = i & 3;
        float x[8];
#pragma unroll
        for (int e = 0; e < 8; ++e) x[e] = w2[(16 * mb + ii) * 32 + gin64_kf(q, e)];
        const int o = mb * 64 + ii * 4 + q;
        split3_trunc(x, W2s[o], W2s[kP2 + o], W2s[2 * kP2 + o]);
    }
    for (int i = tid; i < 4 * 2 * 64; i += kGin64Threads) { // item = (M block, K step, i, q)
        const int mb = i >> 7, ks = (i >> 6) & 1, ii = (i >> 2) & 15, q = i & 3;
        float x[8];
#pragma unroll
        for (int e = 0; e < 8; ++e) x[e] = w3[(16 * mb + ii) * 64 + 32 * ks + gin64_kf(q, e)];
        const int o = (mb * 2 + ks) * 64 + ii * 4 + q;
        split3_trunc(x, W3s[o], W3s[kP3 + o], W3s[2 * kP3 + o]);
    }
    if (tid < 32) Bs[tid] = b1[tid];
    else if (tid < 96) Bs[tid] = b2[tid - 32];
    else if (tid < 160) Bs[tid] = b3[tid - 96];
    __syncthreads();

    // this lane's accumulator registers hold features 16 mb + 4 q + r: bias vectors in that order
    auto bias4 = [&](int base, int mb) {
        const float4 t = *reinterpret_cast<const float4 *>(Bs + base + 16 * mb + 4 * fq);
        return f32x4{t.x, t.y, t.z, t.w};
    };
    const unsigned frag = (unsigned)(fn * 4 + fq);
    double cs[16], cq[16];                                  // BatchNorm sums of this lane's 16 output features
#pragma unroll
    for (int e = 0; e < 16; ++e) cs[e] = cq[e] = 0.0;

    for (int64_t tile = t0; tile < t1; ++tile) {
        // the fragments are re-read every tile: an offset the compiler cannot see through, or it hoists the loop-invariant LDS
        // reads -- all 48 fragments, 192 registers -- out of the loop and spills them
        unsigned wo = frag;
        asm volatile("" : "+v"(wo));
        const bf16x8 *w1p = W1s + wo, *w2p = W2s + wo, *w3p = W3s + wo;
        bf16x8 xa[3], xb[3];
        // ---- layer 1: 2 M blocks x 2 K steps; the small terms of both steps first
        {
            const float x[8] = {zin[0].x, zin[0].y, zin[0].z, zin[0].w, zin[1].x, zin[1].y, zin[1].z, zin[1].w};
            split3_trunc(x, xa[0], xa[1], xa[2]);
        }
        {
            const float x[8] = {zin[2].x, zin[2].y, zin[2].z, zin[2].w, zin[3].x, zin[3].y, zin[3].z, zin[3].w};
            split3_trunc(x, xb[0], xb[1], xb[2]);
        }
        load_z(tile + 1 < t1 ? tile + 1 : tile, zin);
        f32x4 h1[2];
#pragma unroll
        for (int mb = 0; mb < 2; ++mb) {
            f32x4 acc = bias4(0, mb);
            acc = gin64_mma5(w1p + (mb * 2 + 0) * 64, kP1, xa, acc);
            acc = gin64_mma5(w1p + (mb * 2 + 1) * 64, kP1, xb, acc);
            acc = gin64_mma_hh(w1p + (mb * 2 + 0) * 64, xa, acc);
            h1[mb] = gin64_mma_hh(w1p + (mb * 2 + 1) * 64, xb, acc);
        }
        {
            const float x[8] = {sigmoidf_(h1[0][0]), sigmoidf_(h1[0][1]), sigmoidf_(h1[0][2]), sigmoidf_(h1[0][3]),
                                sigmoidf_(h1[1][0]), sigmoidf_(h1[1][1]), sigmoidf_(h1[1][2]), sigmoidf_(h1[1][3])};
            split3_trunc(x, xa[0], xa[1], xa[2]);
        }
        // ---- layer 2: 4 M blocks
        f32x4 h2[4];
#pragma unroll
        for (int mb = 0; mb < 4; ++mb) h2[mb] = small_mma6(w2p + mb * 64, kP2, xa, bias4(32, mb));
        // ---- layer 3: 4 M blocks x 2 K steps (operands in (0, 1): the six terms of a step together, as gin32_mlp_kernel)
        f32x4 o[4];
#pragma unroll
        for (int mb = 0; mb < 4; ++mb) o[mb] = bias4(96, mb);
#pragma unroll
        for (int ks = 0; ks < 2; ++ks) {
            const float x[8] = {sigmoidf_(h2[2 * ks][0]), sigmoidf_(h2[2 * ks][1]), sigmoidf_(h2[2 * ks][2]), sigmoidf_(h2[2 * ks][3]),
                                sigmoidf_(h2[2 * ks + 1][0]), sigmoidf_(h2[2 * ks + 1][1]), sigmoidf_(h2[2 * ks + 1][2]), sigmoidf_(h2[2 * ks + 1][3])};
            split3_trunc(x, xa[0], xa[1], xa[2]);
#pragma unroll
            for (int mb = 0; mb < 4; ++mb) o[mb] = small_mma6(w3p + (mb * 2 + ks) * 64, kP3, xa, o[mb]);
        }
        // ---- epilogue: row fn, features 16 mb + 4 q + r; the output sigmoid at full accuracy (see gin32_mlp_kernel)
        const int64_t row = tile * 16 + fn;
        const bool row_ok = row < n;
#pragma unroll
        for (int mb = 0; mb < 4; ++mb) {
            float4 r;
            r.x = sigmoid_out_f32(o[mb][0]); r.y = sigmoid_out_f32(o[mb][1]); r.z = sigmoid_out_f32(o[mb][2]); r.w = sigmoid_out_f32(o[mb][3]);
            if (act == TGNN_ACT_LEAKY_RELU) { r.x = leakyf_(r.x); r.y = leakyf_(r.y); r.z = leakyf_(r.z); r.w = leakyf_(r.w); }
            if (row_ok) {
                *reinterpret_cast<float4 *>(out + row * 64 + 16 * mb + 4 * fq) = r;
                const float v[4] = {r.x, r.y, r.z, r.w};
#pragma unroll
                for (int e = 0; e < 4; ++e) {
                    cs[4 * mb + e] += (double)v[e];
                    cq[4 * mb + e] += (double)v[e] * (double)v[e];
                }
            }
        }
    }
    if (bn_partial) {
        // lanes of one 16-lane row hold the same 16 features: fold the 16 batch rows (fixed butterfly), then the waves in order
#pragma unroll
        for (int e = 0; e < 16; ++e)
#pragma unroll
            for (int d = 1; d <= 8; d <<= 1) {
                cs[e] += __shfl_xor(cs[e], d, 64);
                cq[e] += __shfl_xor(cq[e], d, 64);
            }
        if (fn == 0) {
#pragma unroll
            for (int e = 0; e < 16; ++e) {
                const int feat = 16 * (e >> 2) + 4 * fq + (e & 3);
                red[wave * 128 + feat] = cs[e];
                red[wave * 128 + 64 + feat] = cq[e];
            }
        }
        __syncthreads();
        if (tid < 128) {                                      // the generic kernel's row: [sum 64 | sum of squares 64]
            double tot = 0.0;
            for (int w = 0; w < kGin64Waves; ++w) tot += red[w * 128 + tid];
            bn_partial[(int64_t)blockIdx.x * 128 + tid] = tot;
        }
    }
}

int gin64_fwd(const float *a, int64_t lda, const float *in_stat, const int32_t *rowptr, const int32_t *col_src, const float *eps,
              const float *w1, const float *b1, const float *w2, const float *b2, const float *w3, const float *b3, int64_t n_nodes,
              int32_t act, float *out, float *z, double *bn_partial, int32_t *n_partials_host, hipStream_t s) {
    if (!(n_nodes >= 1 && lda >= 64 && lda % 4 == 0 && ((uintptr_t)a % 16) == 0 && ((uintptr_t)out % 16) == 0 && z &&
          ((uintptr_t)z % 16) == 0)) {
        set_error("gin64_fwd: rows of at least 64 floats, lda a multiple of 4, a / out / z_scratch 16-byte aligned (lda %lld)",
                  (long long)lda);
        return TGNN_ERR_UNSUPPORTED;
    }
    if (const int rc = tgnn_gin_aggregate(a, lda, in_stat, rowptr, col_src, eps, n_nodes, 64, z, s); rc != TGNN_OK) return rc;
    // persistent 8-wave blocks, one per CU minus a few left to the other chain's kernels (as gin32_mlp_kernel's grid)
    int blocks = producer_blocks(n_nodes, kGin64BlockRows);
    constexpr int reserve = 32;
    if (blocks > cus_minus(reserve)) blocks = cus_minus(reserve);
    if (blocks >= 8) blocks &= ~7;
    gin64_mlp_kernel<<<blocks, kGin64Threads, 0, s>>>(z, w1, b1, w2, b2, w3, b3, n_nodes, act, out, bn_partial);
    if (n_partials_host) *n_partials_host = blocks;
    TGNN_CHECK_LAUNCH();
    return TGNN_OK;
}

}  // namespace tgnn

using namespace tgnn;

extern "C" int tgnn_gin64_fwd(const float *a, int64_t lda, const float *in_stat, const int32_t *rowptr, const int32_t *col_src,
                              const float *eps, const float *w1, const float *b1, const float *w2, const float *b2, const float *w3,
                              const float *b3, int64_t n_nodes, int32_t act, float *out, float *z_scratch, double *bn_partial,
                              int32_t *n_partials_host, tgnn_stream_t stream) {
    DeviceGuard guard__(stream);
    TGNN_CHECK_ARG(n_nodes >= 0, "shape");
    TGNN_CHECK_ARG(act == TGNN_ACT_NONE || act == TGNN_ACT_LEAKY_RELU, "activation");
    if (n_nodes == 0) {
        if (n_partials_host) *n_partials_host = 0;
        return TGNN_OK;
    }
    TGNN_CHECK_ARG(a && rowptr && eps && w1 && b1 && w2 && b2 && w3 && b3 && out && z_scratch, "null pointer");
    TGNN_CHECK_ARG(lda >= 64, "lda");
    return gin64_fwd(a, lda, in_stat, rowptr, col_src, eps, w1, b1, w2, b2, w3, b3, n_nodes, act, out, z_scratch, bn_partial,
                     n_partials_host, static_cast<hipStream_t>(stream));
}
