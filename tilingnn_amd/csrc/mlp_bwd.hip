// The adjoint of a 3-layer sigmoid MLP (Linear -> Sigmoid three times, no BatchNorm) as kernels of its own, behind an opt-in switch
// (tgnn_set_mlp_bwd_fused): what tgnn_sigmoid_mlp_bwd (backward.hip) sequences from a dozen generic launches -- a transpose, two
// dense forwards, then sigmoid_bwd / wgrad / dense per layer, every intermediate through HBM -- for the two shapes every layer of
// tgnn_backward calls it with.  mlp_bwd_plan.h decides the form, the grid and the workspace on the host.
//
// TALL (GINConv's MLP at width 32: 32 -> 32 -> 64 -> 32 over n rows): mlp_bwd_tall_kernel + mlp_bwd_fold_kernel.
//   * 8 waves, persistent, a contiguous run of 16-row tiles per wave (mlp_bwd_tile_share).  Every product runs on
//     v_mfma_f32_16x16x4_f32: exact fp32 products, fp32 accumulation -- the arithmetic of wgrad_kernel.
//   * A tile's activations live in registers in ONE lane map: lane l holds row l & 15, features 16 ft + 4 (l >> 4) + r (r = 0 .. 3)
//     of every 16-feature block ft.  That is the C/D map of D = W . act^T (features down the rows of D, the tile's rows across its
//     columns), and -- read with the K index permuted the same way on the A side -- it is a B operand as it stands: step (ft, r)
//     of a product takes k = 16 ft + 4 g + r from lane group g = l >> 4.  So the chain  x -> t1 -> t2  and back  dpre3 -> d_t2 ->
//     dpre2 -> d_t1 -> dpre1 -> dx  never leaves the registers; the A operands are the weights (or their transposes), read from an
//     LDS image with padded rows (strides 36 / 68 floats: both read patterns touch 64 distinct banks per 64 lanes).
//   * dW_k += dpre_k^T . in_k needs the other map (K = the tile's rows): both factors go through a wave-private LDS stage
//     ([16 rows][in 64 | dpre 64 | pad 16], stride 144 = 16 mod 64) and come back as  lane l: row 4 s + (l >> 4), feature
//     f0 + (l & 15).  The wave keeps dW1, dW2, dW3 (80 registers) and the three bias rows (32 registers, per lane = per tile row;
//     folded over the 16 rows by a butterfly at the very end) across all its tiles.
//   * Rows >= n: the row index is clamped on load, every dpre is forced to zero, the dx store is masked.
//   * End of block: the waves that had tiles add their accumulators into one LDS image in ascending wave order; the image is the
//     block's partial row.  The fold kernel sums the partial rows in fp64 over wgrad_final_kernel's fixed tree.  No atomics:
//     the same bits on every call.
//
// WIDE (GraphConv's edge MLP: fe -> 32 -> 64 -> C C over the T <= 63 distinct attribute rows, no input gradient):
//   mlp_bwd_wide_a_kernel, one block per 64 output columns of layer 3 (re-derives t1, t2; its rows of dW3 / db3 finished; its
//   partial d_t2 to the workspace), then mlp_bwd_wide_b_kernel, one block (partial d_t2 added in fp64 in ascending chunk order;
//   layers 2 and 1).  Plain fp32 FMAs in a fixed order.
//
// TALL at width 64 (GINConv's MLP at width 64: 64 -> 32 -> 64 -> 64): mlp_bwd_tall64_kernel + mlp_bwd_fold64_kernel, a form of its
//   own with its own entry (tgnn_sigmoid_mlp_bwd_tall64) and its own switch (tgnn_set_mlp_bwd_tall64); mlp_bwd64_plan.h plans it.
//   The tall scheme in 4-wave blocks, one wave per SIMD: see the kernel.
#include "mlp_bwd64_plan.h"
#include "mlp_bwd_plan.h"
#include "tgnn_common.h"

namespace tgnn {

static std::atomic<int> g_mlp_bwd_fused{0};                // tgnn_set_mlp_bwd_fused
static std::atomic<int> g_mlp_bwd_tall64{0};               // tgnn_set_mlp_bwd_tall64

typedef float mb_f32x4 __attribute__((ext_vector_type(4)));

constexpr int kMbS32 = 36, kMbS64 = 68;                    // LDS row strides of the weight images (W1, W2: 32 columns; W3: 64)
constexpr int kMbW1 = 0, kMbW2 = kMbW1 + 32 * kMbS32, kMbW3 = kMbW2 + 64 * kMbS32, kMbWFloats = kMbW3 + 32 * kMbS64;
constexpr int kMbStage = 144, kMbStageFloats = kMbStage * kMlpBwdTileRows;    // per wave
constexpr int kMbLdsFloats = kMbWFloats + kMlpBwdWaves * kMbStageFloats;
constexpr int kMbLdsBytes = kMbLdsFloats * 4;              // 96 256 B: one block per CU
static_assert(kMbLdsFloats >= kMlpBwdRowFloats, "the block's partial row is folded in the same LDS");

// the stage is written in one lane map and read in another: LDS operations of a wave execute in order, the compiler must keep them so
#define MB_WAVE_SYNC()                                         \
    do {                                                       \
        __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront"); \
        __builtin_amdgcn_wave_barrier();                       \
        __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront"); \
    } while (0)
#define MB_MFMA(a, b, c) __builtin_amdgcn_mfma_f32_16x16x4f32((a), (b), (c), 0, 0, 0)

// D[16 fo + 4 g + r][row] (+)= sum_k W[16 fo + i][k] in[row][k]: W row-major in LDS with row stride S, `in` in the lane map, KT
// 16-feature blocks of K.  wl = the lane's A base: &W[l & 15][4 g].
template <int KT, int S>
__device__ __forceinline__ mb_f32x4 mb_fwd(const float *wl, int fo, const float (*in)[4], mb_f32x4 acc) {
#pragma unroll
    for (int ft = 0; ft < KT; ++ft) {
        const float4 a = *reinterpret_cast<const float4 *>(wl + fo * 16 * S + 16 * ft);
        acc = MB_MFMA(a.x, in[ft][0], acc);
        acc = MB_MFMA(a.y, in[ft][1], acc);
        acc = MB_MFMA(a.z, in[ft][2], acc);
        acc = MB_MFMA(a.w, in[ft][3], acc);
    }
    return acc;
}
// D[16 fo + 4 g + r][row] = sum_j W[j][16 fo + i] dp[row][j]: the product on W^T, from the same image.  wl = &W[4 g][l & 15].
template <int JT, int S>
__device__ __forceinline__ mb_f32x4 mb_bwd(const float *wl, int fo, const float (*dp)[4]) {
    mb_f32x4 acc = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
    for (int ft = 0; ft < JT; ++ft)
#pragma unroll
        for (int r = 0; r < 4; ++r) acc = MB_MFMA(wl[(16 * ft + r) * S + 16 * fo], dp[ft][r], acc);
    return acc;
}

__global__ __launch_bounds__(kMlpBwdThreads) void mlp_bwd_tall_kernel(
    const float *__restrict__ x, const float *__restrict__ t3, const float *__restrict__ d_out, int64_t ld_dout,
    const float *__restrict__ w1, const float *__restrict__ b1, const float *__restrict__ w2, const float *__restrict__ b2,
    const float *__restrict__ w3, int64_t n, float *__restrict__ dx, float *__restrict__ partial) {
    extern __shared__ float mb_lds[];
    const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63, li = lane & 15, g = lane >> 4;
    for (int e = tid; e < 1024; e += kMlpBwdThreads) mb_lds[kMbW1 + (e >> 5) * kMbS32 + (e & 31)] = w1[e];
    for (int e = tid; e < 2048; e += kMlpBwdThreads) mb_lds[kMbW2 + (e >> 5) * kMbS32 + (e & 31)] = w2[e];
    for (int e = tid; e < 2048; e += kMlpBwdThreads) mb_lds[kMbW3 + (e >> 6) * kMbS64 + (e & 63)] = w3[e];
    __syncthreads();
    float *st = mb_lds + kMbWFloats + wave * kMbStageFloats;

    mb_f32x4 bias1[2], bias2[4];
#pragma unroll
    for (int ft = 0; ft < 2; ++ft)
#pragma unroll
        for (int r = 0; r < 4; ++r) bias1[ft][r] = b1[16 * ft + 4 * g + r];
#pragma unroll
    for (int ft = 0; ft < 4; ++ft)
#pragma unroll
        for (int r = 0; r < 4; ++r) bias2[ft][r] = b2[16 * ft + 4 * g + r];

    mb_f32x4 acc1[2][2], acc2[4][2], acc3[2][4];            // dW1 [32][32], dW2 [64][32], dW3 [32][64] as 16 x 16 tiles
    float sb1[2][4], sb2[4][4], sb3[2][4];                  // bias gradients of the lane's row
#pragma unroll
    for (int i = 0; i < 2; ++i)
#pragma unroll
        for (int j = 0; j < 2; ++j) acc1[i][j] = mb_f32x4{0.f, 0.f, 0.f, 0.f};
#pragma unroll
    for (int i = 0; i < 4; ++i)
#pragma unroll
        for (int j = 0; j < 2; ++j) acc2[i][j] = mb_f32x4{0.f, 0.f, 0.f, 0.f};
#pragma unroll
    for (int i = 0; i < 2; ++i)
#pragma unroll
        for (int j = 0; j < 4; ++j) acc3[i][j] = mb_f32x4{0.f, 0.f, 0.f, 0.f};
#pragma unroll
    for (int i = 0; i < 4; ++i)
#pragma unroll
        for (int r = 0; r < 4; ++r) {
            sb2[i][r] = 0.f;
            if (i < 2) sb1[i][r] = sb3[i][r] = 0.f;
        }

    const Gin64Tiles share = mlp_bwd_tile_share(n, (int)gridDim.x, (int)blockIdx.x, wave);
    for (int64_t tile = share.t0; tile < share.t1; ++tile) {
        // the weight fragments do not depend on the tile: an index the compiler cannot see through keeps it from hoisting all of
        // their LDS reads out of this loop into registers it does not have
        int opq = 0;
        asm volatile("" : "+v"(opq));
        const float *w1f = mb_lds + kMbW1 + opq + li * kMbS32 + 4 * g, *w1b = mb_lds + kMbW1 + opq + 4 * g * kMbS32 + li;
        const float *w2f = mb_lds + kMbW2 + opq + li * kMbS32 + 4 * g, *w2b = mb_lds + kMbW2 + opq + 4 * g * kMbS32 + li;
        const float *w3b = mb_lds + kMbW3 + opq + 4 * g * kMbS64 + li;

        const int64_t row_raw = tile * kMlpBwdTileRows + li;
        const bool valid = row_raw < n;
        const int64_t row = valid ? row_raw : n - 1;
        float xv[2][4], t1[2][4], t2[4][4], dp3[2][4], dp2[4][4], dp1[2][4];
#pragma unroll
        for (int ft = 0; ft < 2; ++ft) {
            const float4 xx = *reinterpret_cast<const float4 *>(x + row * 32 + 16 * ft + 4 * g);
            const float4 tt = *reinterpret_cast<const float4 *>(t3 + row * 32 + 16 * ft + 4 * g);
            const float4 dd = *reinterpret_cast<const float4 *>(d_out + row * ld_dout + 16 * ft + 4 * g);
            xv[ft][0] = xx.x; xv[ft][1] = xx.y; xv[ft][2] = xx.z; xv[ft][3] = xx.w;
            dp3[ft][0] = valid ? dd.x * tt.x * (1.0f - tt.x) : 0.f;
            dp3[ft][1] = valid ? dd.y * tt.y * (1.0f - tt.y) : 0.f;
            dp3[ft][2] = valid ? dd.z * tt.z * (1.0f - tt.z) : 0.f;
            dp3[ft][3] = valid ? dd.w * tt.w * (1.0f - tt.w) : 0.f;
        }
        // t1 = sigmoid(W1 x + b1), t2 = sigmoid(W2 t1 + b2)
#pragma unroll
        for (int fo = 0; fo < 2; ++fo) {
            const mb_f32x4 p = mb_fwd<2, kMbS32>(w1f, fo, xv, bias1[fo]);
#pragma unroll
            for (int r = 0; r < 4; ++r) t1[fo][r] = sigmoid_out_f32(p[r]);
        }
#pragma unroll
        for (int fo = 0; fo < 4; ++fo) {
            const mb_f32x4 p = mb_fwd<2, kMbS32>(w2f, fo, t1, bias2[fo]);
#pragma unroll
            for (int r = 0; r < 4; ++r) t2[fo][r] = sigmoid_out_f32(p[r]);
        }
        // ---- layer 3: dW3 += dpre3^T t2, db3 += dpre3, d_t2 = dpre3 W3
#pragma unroll
        for (int ft = 0; ft < 4; ++ft)
            *reinterpret_cast<float4 *>(st + li * kMbStage + 16 * ft + 4 * g) = make_float4(t2[ft][0], t2[ft][1], t2[ft][2], t2[ft][3]);
#pragma unroll
        for (int ft = 0; ft < 2; ++ft) {
            *reinterpret_cast<float4 *>(st + li * kMbStage + 64 + 16 * ft + 4 * g) =
                make_float4(dp3[ft][0], dp3[ft][1], dp3[ft][2], dp3[ft][3]);
#pragma unroll
            for (int r = 0; r < 4; ++r) sb3[ft][r] += dp3[ft][r];
        }
        MB_WAVE_SYNC();
#pragma unroll
        for (int s = 0; s < 4; ++s) {
            const float *sr = st + (4 * s + g) * kMbStage + li;
            float a[2], b[4];
#pragma unroll
            for (int i = 0; i < 2; ++i) a[i] = sr[64 + 16 * i];
#pragma unroll
            for (int j = 0; j < 4; ++j) b[j] = sr[16 * j];
#pragma unroll
            for (int i = 0; i < 2; ++i)
#pragma unroll
                for (int j = 0; j < 4; ++j) acc3[i][j] = MB_MFMA(a[i], b[j], acc3[i][j]);
        }
#pragma unroll
        for (int fo = 0; fo < 4; ++fo) {
            const mb_f32x4 d = mb_bwd<2, kMbS64>(w3b, fo, dp3);
#pragma unroll
            for (int r = 0; r < 4; ++r) dp2[fo][r] = valid ? d[r] * t2[fo][r] * (1.0f - t2[fo][r]) : 0.f;
        }
        // ---- layer 2: dW2 += dpre2^T t1, db2 += dpre2, d_t1 = dpre2 W2
        MB_WAVE_SYNC();
#pragma unroll
        for (int ft = 0; ft < 2; ++ft)
            *reinterpret_cast<float4 *>(st + li * kMbStage + 16 * ft + 4 * g) = make_float4(t1[ft][0], t1[ft][1], t1[ft][2], t1[ft][3]);
#pragma unroll
        for (int ft = 0; ft < 4; ++ft) {
            *reinterpret_cast<float4 *>(st + li * kMbStage + 64 + 16 * ft + 4 * g) =
                make_float4(dp2[ft][0], dp2[ft][1], dp2[ft][2], dp2[ft][3]);
#pragma unroll
            for (int r = 0; r < 4; ++r) sb2[ft][r] += dp2[ft][r];
        }
        MB_WAVE_SYNC();
#pragma unroll
        for (int s = 0; s < 4; ++s) {
            const float *sr = st + (4 * s + g) * kMbStage + li;
            float a[4], b[2];
#pragma unroll
            for (int i = 0; i < 4; ++i) a[i] = sr[64 + 16 * i];
#pragma unroll
            for (int j = 0; j < 2; ++j) b[j] = sr[16 * j];
#pragma unroll
            for (int i = 0; i < 4; ++i)
#pragma unroll
                for (int j = 0; j < 2; ++j) acc2[i][j] = MB_MFMA(a[i], b[j], acc2[i][j]);
        }
#pragma unroll
        for (int fo = 0; fo < 2; ++fo) {
            const mb_f32x4 d = mb_bwd<4, kMbS32>(w2b, fo, dp2);
#pragma unroll
            for (int r = 0; r < 4; ++r) dp1[fo][r] = valid ? d[r] * t1[fo][r] * (1.0f - t1[fo][r]) : 0.f;
        }
        // ---- layer 1: dW1 += dpre1^T x, db1 += dpre1, dx = dpre1 W1
        MB_WAVE_SYNC();
#pragma unroll
        for (int ft = 0; ft < 2; ++ft) {
            *reinterpret_cast<float4 *>(st + li * kMbStage + 16 * ft + 4 * g) = make_float4(xv[ft][0], xv[ft][1], xv[ft][2], xv[ft][3]);
            *reinterpret_cast<float4 *>(st + li * kMbStage + 64 + 16 * ft + 4 * g) =
                make_float4(dp1[ft][0], dp1[ft][1], dp1[ft][2], dp1[ft][3]);
#pragma unroll
            for (int r = 0; r < 4; ++r) sb1[ft][r] += dp1[ft][r];
        }
        MB_WAVE_SYNC();
#pragma unroll
        for (int s = 0; s < 4; ++s) {
            const float *sr = st + (4 * s + g) * kMbStage + li;
            float a[2], b[2];
#pragma unroll
            for (int i = 0; i < 2; ++i) a[i] = sr[64 + 16 * i];
#pragma unroll
            for (int j = 0; j < 2; ++j) b[j] = sr[16 * j];
#pragma unroll
            for (int i = 0; i < 2; ++i)
#pragma unroll
                for (int j = 0; j < 2; ++j) acc1[i][j] = MB_MFMA(a[i], b[j], acc1[i][j]);
        }
        MB_WAVE_SYNC();
        if (dx) {                                            // (uniform)
#pragma unroll
            for (int fo = 0; fo < 2; ++fo) {
                const mb_f32x4 d = mb_bwd<2, kMbS32>(w1b, fo, dp1);
                if (valid) *reinterpret_cast<float4 *>(dx + row * 32 + 16 * fo + 4 * g) = make_float4(d[0], d[1], d[2], d[3]);
            }
        }
    }

    // ---- the block's partial row: the waves in ascending order into one LDS image (the weights and the stages are dead)
#pragma unroll
    for (int i = 0; i < 4; ++i)
#pragma unroll
        for (int r = 0; r < 4; ++r) {                        // the 16 rows of a lane group: fixed butterfly
#pragma unroll
            for (int d = 1; d <= 8; d <<= 1) {
                sb2[i][r] += __shfl_xor(sb2[i][r], d, 64);
                if (i < 2) {
                    sb1[i][r] += __shfl_xor(sb1[i][r], d, 64);
                    sb3[i][r] += __shfl_xor(sb3[i][r], d, 64);
                }
            }
        }
    __syncthreads();
    int first_wave = -1;                                     // waves without tiles hold zeros: they are left out (block-uniform)
    for (int w = 0; w < kMlpBwdWaves; ++w) {
        const Gin64Tiles sw = mlp_bwd_tile_share(n, (int)gridDim.x, (int)blockIdx.x, w);
        if (sw.t1 <= sw.t0) continue;
        if (first_wave < 0) first_wave = w;
        if (wave == w) {                                     // (uniform per wave)
            const bool first = w == first_wave;
#define MB_PUT(idx, v)                                             \
    do {                                                           \
        const int idx__ = (idx);                                   \
        mb_lds[idx__] = first ? (v) : mb_lds[idx__] + (v);         \
    } while (0)
#pragma unroll
            for (int r = 0; r < 4; ++r) {
#pragma unroll
                for (int i = 0; i < 2; ++i)
#pragma unroll
                    for (int j = 0; j < 2; ++j) MB_PUT(kMlpBwdOffW1 + (16 * i + 4 * g + r) * 32 + 16 * j + li, acc1[i][j][r]);
#pragma unroll
                for (int i = 0; i < 4; ++i)
#pragma unroll
                    for (int j = 0; j < 2; ++j) MB_PUT(kMlpBwdOffW2 + (16 * i + 4 * g + r) * 32 + 16 * j + li, acc2[i][j][r]);
#pragma unroll
                for (int i = 0; i < 2; ++i)
#pragma unroll
                    for (int j = 0; j < 4; ++j) MB_PUT(kMlpBwdOffW3 + (16 * i + 4 * g + r) * 64 + 16 * j + li, acc3[i][j][r]);
                if (li == 0) {
#pragma unroll
                    for (int i = 0; i < 4; ++i) {
                        MB_PUT(kMlpBwdOffB2 + 16 * i + 4 * g + r, sb2[i][r]);
                        if (i < 2) {
                            MB_PUT(kMlpBwdOffB1 + 16 * i + 4 * g + r, sb1[i][r]);
                            MB_PUT(kMlpBwdOffB3 + 16 * i + 4 * g + r, sb3[i][r]);
                        }
                    }
                }
            }
#undef MB_PUT
        }
        __syncthreads();
    }
    float *prow = partial + (size_t)blockIdx.x * kMlpBwdRowFloats;
    for (int e = tid; e < kMlpBwdRowFloats; e += kMlpBwdThreads) prow[e] = first_wave >= 0 ? mb_lds[e] : 0.f;
}

struct MlpBwdOut {
    float *dw1, *db1, *dw2, *db2, *dw3, *db3;
};

// 16 consecutive elements x 16 lanes over the partial rows, fp64, butterfly over the lanes: wgrad_final_kernel's tree
__global__ __launch_bounds__(256) void mlp_bwd_fold_kernel(const float *__restrict__ partial, int n_partials, MlpBwdOut o) {
    const int pl = threadIdx.x & 15, el = threadIdx.x >> 4;
    const int i_raw = (int)blockIdx.x * 16 + el;
    const int i = i_raw < kMlpBwdRowFloats ? i_raw : kMlpBwdRowFloats - 1;
    double s = 0.0;
    for (int p = pl; p < n_partials; p += 16) s += (double)partial[(size_t)p * kMlpBwdRowFloats + i];
#pragma unroll
    for (int d = 8; d >= 1; d >>= 1) s += __shfl_xor(s, d);
    if (pl == 0 && i_raw < kMlpBwdRowFloats) {
        const float v = (float)s;
        if (i < kMlpBwdOffB1) o.dw1[i - kMlpBwdOffW1] = v;
        else if (i < kMlpBwdOffW2) o.db1[i - kMlpBwdOffB1] = v;
        else if (i < kMlpBwdOffB2) o.dw2[i - kMlpBwdOffW2] = v;
        else if (i < kMlpBwdOffW3) o.db2[i - kMlpBwdOffB2] = v;
        else if (i < kMlpBwdOffB3) o.dw3[i - kMlpBwdOffW3] = v;
        else o.db3[i - kMlpBwdOffB3] = v;
    }
}

// ------------------------------------------------------------------------------------------------ tall form at width 64
// GINConv's MLP at width 64 (64 -> 32 -> 64 -> 64): the tall scheme with four 16-feature blocks where width 32 has two -- the same
// lane map, the same stage row, 320 matrix instructions per tile.  What differs is where the wave's state lives: 32 accumulator
// tiles (128 registers), 40 bias sums, 24 bias values and a tile's activations (80) do not fit the 256 registers a wave has at two
// waves per SIMD, so the block is 4 waves, ONE per SIMD, and a wave has the unified 512-entry file (mlp_bwd64_plan.h has the grid).
// Weight images: W1 [32][64] and W3 [64][64] with row stride 68, W2 [64][32] with stride 36.
// One product is NOT on the fp32 instruction: layer 1's forward, W1 . x, runs on v_mfma_f64_16x16x4_f64 (32 of the 320).  A row of x
// times a row of W1 is 64 terms that may cancel (an input row 50 times the others' size: terms of magnitude 100, a sum of order 1),
// and fp32 partial sums of that magnitude leave 1e-5 in the pre-activation whatever their order -- which is then the relative
// error of sigmoid' on that row, and, the row being the largest, of dW1 (DESIGN section 31 has the figures: this kernel with fp32
// there and the chain of generic kernels both straddle 1e-5).  fp32 operands convert exactly; the sum is rounded to fp32 once.
// The fp64 form's C/D map is  row = (lane >> 4) + 4 reg, not 4 (lane >> 4) + reg: the A side reads W1's rows permuted
// (A row m <- feature 4 (m & 3) + (m >> 2)), so that register r of lane group g is again feature 4 g + r.
typedef double mb_f64x4 __attribute__((ext_vector_type(4)));
constexpr int kMb64W1 = 0, kMb64W2 = kMb64W1 + 32 * kMbS64, kMb64W3 = kMb64W2 + 64 * kMbS32, kMb64WFloats = kMb64W3 + 64 * kMbS64;
constexpr int kMb64LdsFloats = kMb64WFloats + kMlpBwd64Waves * kMbStageFloats;
constexpr int kMb64LdsBytes = kMb64LdsFloats * 4;          // 72 192 B
static_assert(kMb64LdsFloats >= kMlpBwd64RowFloats, "the block's partial row is folded in the same LDS");
static_assert(kMb64W2 % 4 == 0 && kMb64W3 % 4 == 0 && kMb64WFloats % 4 == 0, "16-byte fragment reads");

__global__ __launch_bounds__(kMlpBwd64Threads) void mlp_bwd_tall64_kernel(
    const float *__restrict__ x, const float *__restrict__ t3, const float *__restrict__ d_out, int64_t ld_dout,
    const float *__restrict__ w1, const float *__restrict__ b1, const float *__restrict__ w2, const float *__restrict__ b2,
    const float *__restrict__ w3, int64_t n, float *__restrict__ dx, float *__restrict__ partial) {
    extern __shared__ float mb_lds[];
    const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63, li = lane & 15, g = lane >> 4;
    for (int e = tid; e < 2048; e += kMlpBwd64Threads) mb_lds[kMb64W1 + (e >> 6) * kMbS64 + (e & 63)] = w1[e];
    for (int e = tid; e < 2048; e += kMlpBwd64Threads) mb_lds[kMb64W2 + (e >> 5) * kMbS32 + (e & 31)] = w2[e];
    for (int e = tid; e < 4096; e += kMlpBwd64Threads) mb_lds[kMb64W3 + (e >> 6) * kMbS64 + (e & 63)] = w3[e];
    __syncthreads();
    float *st = mb_lds + kMb64WFloats + wave * kMbStageFloats;

    mb_f32x4 bias1[2], bias2[4];
#pragma unroll
    for (int ft = 0; ft < 2; ++ft)
#pragma unroll
        for (int r = 0; r < 4; ++r) bias1[ft][r] = b1[16 * ft + 4 * g + r];
#pragma unroll
    for (int ft = 0; ft < 4; ++ft)
#pragma unroll
        for (int r = 0; r < 4; ++r) bias2[ft][r] = b2[16 * ft + 4 * g + r];

    mb_f32x4 acc1[2][4], acc2[4][2], acc3[4][4];            // dW1 [32][64], dW2 [64][32], dW3 [64][64] as 16 x 16 tiles
    float sb1[2][4], sb2[4][4], sb3[4][4];                  // bias gradients of the lane's row
#pragma unroll
    for (int i = 0; i < 4; ++i)
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            acc3[i][j] = mb_f32x4{0.f, 0.f, 0.f, 0.f};
            if (i < 2) acc1[i][j] = mb_f32x4{0.f, 0.f, 0.f, 0.f};
            if (j < 2) acc2[i][j] = mb_f32x4{0.f, 0.f, 0.f, 0.f};
            sb2[i][j] = sb3[i][j] = 0.f;
            if (i < 2) sb1[i][j] = 0.f;
        }

    const Gin64Tiles share = mlp_bwd_tall64_tile_share(n, (int)gridDim.x, (int)blockIdx.x, wave);
    for (int64_t tile = share.t0; tile < share.t1; ++tile) {
        // (as in mlp_bwd_tall_kernel: keeps the loop-invariant weight fragments out of registers)
        int opq = 0;
        asm volatile("" : "+v"(opq));
        const float *w1f = mb_lds + kMb64W1 + opq + (4 * (li & 3) + (li >> 2)) * kMbS64 + 4 * g;     // (permuted rows: fp64 form)
        const float *w1b = mb_lds + kMb64W1 + opq + 4 * g * kMbS64 + li;
        const float *w2f = mb_lds + kMb64W2 + opq + li * kMbS32 + 4 * g, *w2b = mb_lds + kMb64W2 + opq + 4 * g * kMbS32 + li;
        const float *w3b = mb_lds + kMb64W3 + opq + 4 * g * kMbS64 + li;

        const int64_t row_raw = tile * kMlpBwdTileRows + li;
        const bool valid = row_raw < n;
        const int64_t row = valid ? row_raw : n - 1;
        float xv[4][4], t1[2][4], t2[4][4], dp3[4][4], dp2[4][4], dp1[2][4];
#pragma unroll
        for (int ft = 0; ft < 4; ++ft) {
            const float4 xx = *reinterpret_cast<const float4 *>(x + row * 64 + 16 * ft + 4 * g);
            const float4 tt = *reinterpret_cast<const float4 *>(t3 + row * 64 + 16 * ft + 4 * g);
            const float4 dd = *reinterpret_cast<const float4 *>(d_out + row * ld_dout + 16 * ft + 4 * g);
            xv[ft][0] = xx.x; xv[ft][1] = xx.y; xv[ft][2] = xx.z; xv[ft][3] = xx.w;
            dp3[ft][0] = valid ? dd.x * tt.x * (1.0f - tt.x) : 0.f;
            dp3[ft][1] = valid ? dd.y * tt.y * (1.0f - tt.y) : 0.f;
            dp3[ft][2] = valid ? dd.z * tt.z * (1.0f - tt.z) : 0.f;
            dp3[ft][3] = valid ? dd.w * tt.w * (1.0f - tt.w) : 0.f;
        }
        // t1 = sigmoid(W1 x + b1), t2 = sigmoid(W2 t1 + b2)
#pragma unroll
        for (int fo = 0; fo < 2; ++fo) {
            mb_f64x4 p = {(double)bias1[fo][0], (double)bias1[fo][1], (double)bias1[fo][2], (double)bias1[fo][3]};
#pragma unroll
            for (int ft = 0; ft < 4; ++ft) {
                const float4 a = *reinterpret_cast<const float4 *>(w1f + fo * 16 * kMbS64 + 16 * ft);
                p = __builtin_amdgcn_mfma_f64_16x16x4f64((double)a.x, (double)xv[ft][0], p, 0, 0, 0);
                p = __builtin_amdgcn_mfma_f64_16x16x4f64((double)a.y, (double)xv[ft][1], p, 0, 0, 0);
                p = __builtin_amdgcn_mfma_f64_16x16x4f64((double)a.z, (double)xv[ft][2], p, 0, 0, 0);
                p = __builtin_amdgcn_mfma_f64_16x16x4f64((double)a.w, (double)xv[ft][3], p, 0, 0, 0);
            }
#pragma unroll
            for (int r = 0; r < 4; ++r) t1[fo][r] = sigmoid_out_f32((float)p[r]);
        }
#pragma unroll
        for (int fo = 0; fo < 4; ++fo) {
            const mb_f32x4 p = mb_fwd<2, kMbS32>(w2f, fo, t1, bias2[fo]);
#pragma unroll
            for (int r = 0; r < 4; ++r) t2[fo][r] = sigmoid_out_f32(p[r]);
        }
        // ---- layer 3: dW3 += dpre3^T t2, db3 += dpre3, d_t2 = dpre3 W3
#pragma unroll
        for (int ft = 0; ft < 4; ++ft) {
            *reinterpret_cast<float4 *>(st + li * kMbStage + 16 * ft + 4 * g) = make_float4(t2[ft][0], t2[ft][1], t2[ft][2], t2[ft][3]);
            *reinterpret_cast<float4 *>(st + li * kMbStage + 64 + 16 * ft + 4 * g) =
                make_float4(dp3[ft][0], dp3[ft][1], dp3[ft][2], dp3[ft][3]);
#pragma unroll
            for (int r = 0; r < 4; ++r) sb3[ft][r] += dp3[ft][r];
        }
        MB_WAVE_SYNC();
#pragma unroll
        for (int s = 0; s < 4; ++s) {
            const float *sr = st + (4 * s + g) * kMbStage + li;
            float a[4], b[4];
#pragma unroll
            for (int i = 0; i < 4; ++i) a[i] = sr[64 + 16 * i];
#pragma unroll
            for (int j = 0; j < 4; ++j) b[j] = sr[16 * j];
#pragma unroll
            for (int i = 0; i < 4; ++i)
#pragma unroll
                for (int j = 0; j < 4; ++j) acc3[i][j] = MB_MFMA(a[i], b[j], acc3[i][j]);
        }
#pragma unroll
        for (int fo = 0; fo < 4; ++fo) {
            const mb_f32x4 d = mb_bwd<4, kMbS64>(w3b, fo, dp3);
#pragma unroll
            for (int r = 0; r < 4; ++r) dp2[fo][r] = valid ? d[r] * t2[fo][r] * (1.0f - t2[fo][r]) : 0.f;
        }
        // ---- layer 2: dW2 += dpre2^T t1, db2 += dpre2, d_t1 = dpre2 W2
        MB_WAVE_SYNC();
#pragma unroll
        for (int ft = 0; ft < 2; ++ft)
            *reinterpret_cast<float4 *>(st + li * kMbStage + 16 * ft + 4 * g) = make_float4(t1[ft][0], t1[ft][1], t1[ft][2], t1[ft][3]);
#pragma unroll
        for (int ft = 0; ft < 4; ++ft) {
            *reinterpret_cast<float4 *>(st + li * kMbStage + 64 + 16 * ft + 4 * g) =
                make_float4(dp2[ft][0], dp2[ft][1], dp2[ft][2], dp2[ft][3]);
#pragma unroll
            for (int r = 0; r < 4; ++r) sb2[ft][r] += dp2[ft][r];
        }
        MB_WAVE_SYNC();
#pragma unroll
        for (int s = 0; s < 4; ++s) {
            const float *sr = st + (4 * s + g) * kMbStage + li;
            float a[4], b[2];
#pragma unroll
            for (int i = 0; i < 4; ++i) a[i] = sr[64 + 16 * i];
#pragma unroll
            for (int j = 0; j < 2; ++j) b[j] = sr[16 * j];
#pragma unroll
            for (int i = 0; i < 4; ++i)
#pragma unroll
                for (int j = 0; j < 2; ++j) acc2[i][j] = MB_MFMA(a[i], b[j], acc2[i][j]);
        }
#pragma unroll
        for (int fo = 0; fo < 2; ++fo) {
            const mb_f32x4 d = mb_bwd<4, kMbS32>(w2b, fo, dp2);
#pragma unroll
            for (int r = 0; r < 4; ++r) dp1[fo][r] = valid ? d[r] * t1[fo][r] * (1.0f - t1[fo][r]) : 0.f;
        }
        // ---- layer 1: dW1 += dpre1^T x, db1 += dpre1, dx = dpre1 W1
        MB_WAVE_SYNC();
#pragma unroll
        for (int ft = 0; ft < 4; ++ft)
            *reinterpret_cast<float4 *>(st + li * kMbStage + 16 * ft + 4 * g) = make_float4(xv[ft][0], xv[ft][1], xv[ft][2], xv[ft][3]);
#pragma unroll
        for (int ft = 0; ft < 2; ++ft) {
            *reinterpret_cast<float4 *>(st + li * kMbStage + 64 + 16 * ft + 4 * g) =
                make_float4(dp1[ft][0], dp1[ft][1], dp1[ft][2], dp1[ft][3]);
#pragma unroll
            for (int r = 0; r < 4; ++r) sb1[ft][r] += dp1[ft][r];
        }
        MB_WAVE_SYNC();
#pragma unroll
        for (int s = 0; s < 4; ++s) {
            const float *sr = st + (4 * s + g) * kMbStage + li;
            float a[2], b[4];
#pragma unroll
            for (int i = 0; i < 2; ++i) a[i] = sr[64 + 16 * i];
#pragma unroll
            for (int j = 0; j < 4; ++j) b[j] = sr[16 * j];
#pragma unroll
            for (int i = 0; i < 2; ++i)
#pragma unroll
                for (int j = 0; j < 4; ++j) acc1[i][j] = MB_MFMA(a[i], b[j], acc1[i][j]);
        }
        MB_WAVE_SYNC();
        if (dx) {                                            // (uniform)
#pragma unroll
            for (int fo = 0; fo < 4; ++fo) {
                const mb_f32x4 d = mb_bwd<2, kMbS64>(w1b, fo, dp1);
                if (valid) *reinterpret_cast<float4 *>(dx + row * 64 + 16 * fo + 4 * g) = make_float4(d[0], d[1], d[2], d[3]);
            }
        }
    }

    // ---- the block's partial row: the waves in ascending order into one LDS image (the weights and the stages are dead)
#pragma unroll
    for (int i = 0; i < 4; ++i)
#pragma unroll
        for (int r = 0; r < 4; ++r) {                        // the 16 rows of a lane group: fixed butterfly
#pragma unroll
            for (int d = 1; d <= 8; d <<= 1) {
                sb2[i][r] += __shfl_xor(sb2[i][r], d, 64);
                sb3[i][r] += __shfl_xor(sb3[i][r], d, 64);
                if (i < 2) sb1[i][r] += __shfl_xor(sb1[i][r], d, 64);
            }
        }
    __syncthreads();
    int first_wave = -1;                                     // waves without tiles hold zeros: they are left out (block-uniform)
    for (int w = 0; w < kMlpBwd64Waves; ++w) {
        const Gin64Tiles sw = mlp_bwd_tall64_tile_share(n, (int)gridDim.x, (int)blockIdx.x, w);
        if (sw.t1 <= sw.t0) continue;
        if (first_wave < 0) first_wave = w;
        if (wave == w) {                                     // (uniform per wave)
            const bool first = w == first_wave;
#define MB_PUT(idx, v)                                             \
    do {                                                           \
        const int idx__ = (idx);                                   \
        mb_lds[idx__] = first ? (v) : mb_lds[idx__] + (v);         \
    } while (0)
#pragma unroll
            for (int r = 0; r < 4; ++r) {
#pragma unroll
                for (int i = 0; i < 2; ++i)
#pragma unroll
                    for (int j = 0; j < 4; ++j) MB_PUT(kMlpBwd64OffW1 + (16 * i + 4 * g + r) * 64 + 16 * j + li, acc1[i][j][r]);
#pragma unroll
                for (int i = 0; i < 4; ++i)
#pragma unroll
                    for (int j = 0; j < 2; ++j) MB_PUT(kMlpBwd64OffW2 + (16 * i + 4 * g + r) * 32 + 16 * j + li, acc2[i][j][r]);
#pragma unroll
                for (int i = 0; i < 4; ++i)
#pragma unroll
                    for (int j = 0; j < 4; ++j) MB_PUT(kMlpBwd64OffW3 + (16 * i + 4 * g + r) * 64 + 16 * j + li, acc3[i][j][r]);
                if (li == 0) {
#pragma unroll
                    for (int i = 0; i < 4; ++i) {
                        MB_PUT(kMlpBwd64OffB2 + 16 * i + 4 * g + r, sb2[i][r]);
                        MB_PUT(kMlpBwd64OffB3 + 16 * i + 4 * g + r, sb3[i][r]);
                        if (i < 2) MB_PUT(kMlpBwd64OffB1 + 16 * i + 4 * g + r, sb1[i][r]);
                    }
                }
            }
#undef MB_PUT
        }
        __syncthreads();
    }
    float *prow = partial + (size_t)blockIdx.x * kMlpBwd64RowFloats;
    for (int e = tid; e < kMlpBwd64RowFloats; e += kMlpBwd64Threads) prow[e] = first_wave >= 0 ? mb_lds[e] : 0.f;
}

// mlp_bwd_fold_kernel over the width-64 row layout
__global__ __launch_bounds__(256) void mlp_bwd_fold64_kernel(const float *__restrict__ partial, int n_partials, MlpBwdOut o) {
    const int pl = threadIdx.x & 15, el = threadIdx.x >> 4;
    const int i_raw = (int)blockIdx.x * 16 + el;
    const int i = i_raw < kMlpBwd64RowFloats ? i_raw : kMlpBwd64RowFloats - 1;
    double s = 0.0;
    for (int p = pl; p < n_partials; p += 16) s += (double)partial[(size_t)p * kMlpBwd64RowFloats + i];
#pragma unroll
    for (int d = 8; d >= 1; d >>= 1) s += __shfl_xor(s, d);
    if (pl == 0 && i_raw < kMlpBwd64RowFloats) {
        const float v = (float)s;
        if (i < kMlpBwd64OffB1) o.dw1[i - kMlpBwd64OffW1] = v;
        else if (i < kMlpBwd64OffW2) o.db1[i - kMlpBwd64OffB1] = v;
        else if (i < kMlpBwd64OffB2) o.dw2[i - kMlpBwd64OffW2] = v;
        else if (i < kMlpBwd64OffW3) o.db2[i - kMlpBwd64OffB2] = v;
        else if (i < kMlpBwd64OffB3) o.dw3[i - kMlpBwd64OffW3] = v;
        else o.db3[i - kMlpBwd64OffB3] = v;
    }
}

// ------------------------------------------------------------------------------------------------ wide form
constexpr int kMbWideRows = kMlpBwdWideMaxRows;

// t1 [T][32], t2 [T][64] of all rows into LDS (xs: the rows themselves, [T][fe]); every thread of the block calls
__device__ __forceinline__ void mb_wide_rederive(const float *__restrict__ x, int T, int fe, const float *__restrict__ w1,
                                                 const float *__restrict__ b1, const float *__restrict__ w2,
                                                 const float *__restrict__ b2, float *xs, float *t1, float *t2) {
    const int tid = threadIdx.x, nthr = blockDim.x;
    for (int e = tid; e < T * fe; e += nthr) xs[e] = x[e];
    __syncthreads();
    for (int e = tid; e < T * 32; e += nthr) {
        const int r = e >> 5, j = e & 31;
        float a = b1[j];
        for (int k = 0; k < fe; ++k) a = fmaf(xs[r * fe + k], w1[j * fe + k], a);
        t1[e] = sigmoid_out_f32(a);
    }
    __syncthreads();
    for (int e = tid; e < T * 64; e += nthr) {
        const int r = e >> 6, j = e & 63;
        float a = b2[j];
#pragma unroll 8
        for (int k = 0; k < 32; ++k) a = fmaf(t1[r * 32 + k], w2[j * 32 + k], a);
        t2[e] = sigmoid_out_f32(a);
    }
    __syncthreads();
}

// block c: output columns [64 c, 64 c + 64) of layer 3
__global__ __launch_bounds__(256) void mlp_bwd_wide_a_kernel(const float *__restrict__ x, int T, int fe, int d3,
                                                             const float *__restrict__ w1, const float *__restrict__ b1,
                                                             const float *__restrict__ w2, const float *__restrict__ b2,
                                                             const float *__restrict__ w3, const float *__restrict__ t3,
                                                             const float *__restrict__ d_out, int64_t ld_dout,
                                                             float *__restrict__ dw3, float *__restrict__ db3,
                                                             float *__restrict__ part) {
    __shared__ float xs[kMbWideRows * 64], t1[kMbWideRows * 32], t2[kMbWideRows * 64], dp3[kMbWideRows * 64];
    const int tid = threadIdx.x, c0 = (int)blockIdx.x * kMlpBwdWideChunk;
    mb_wide_rederive(x, T, fe, w1, b1, w2, b2, xs, t1, t2);
    for (int e = tid; e < T * 64; e += 256) {
        const int r = e >> 6, j = e & 63;
        const float tv = t3[(int64_t)r * d3 + c0 + j];
        dp3[e] = d_out[(int64_t)r * ld_dout + c0 + j] * tv * (1.0f - tv);
    }
    __syncthreads();
    for (int e = tid; e < 64 * 64; e += 256) {               // dW3 [d3][64]: this block's 64 rows, finished
        const int j = e >> 6, k = e & 63;
        float a = 0.f;
        for (int r = 0; r < T; ++r) a = fmaf(dp3[r * 64 + j], t2[r * 64 + k], a);
        dw3[(int64_t)(c0 + j) * 64 + k] = a;
    }
    if (tid < 64) {
        float a = 0.f;
        for (int r = 0; r < T; ++r) a += dp3[r * 64 + tid];
        db3[c0 + tid] = a;
    }
    float *prow = part + (size_t)blockIdx.x * T * 64;        // this chunk's share of d_t2 [T][64]
    for (int e = tid; e < T * 64; e += 256) {
        const int r = e >> 6, k = e & 63;
        float a = 0.f;
#pragma unroll 8
        for (int j = 0; j < 64; ++j) a = fmaf(dp3[r * 64 + j], w3[(int64_t)(c0 + j) * 64 + k], a);
        prow[e] = a;
    }
}

__global__ __launch_bounds__(256) void mlp_bwd_wide_b_kernel(const float *__restrict__ x, int T, int fe,
                                                             const float *__restrict__ w1, const float *__restrict__ b1,
                                                             const float *__restrict__ w2, const float *__restrict__ b2,
                                                             const float *__restrict__ part, int n_chunks,
                                                             float *__restrict__ dw1, float *__restrict__ db1,
                                                             float *__restrict__ dw2, float *__restrict__ db2) {
    __shared__ float xs[kMbWideRows * 64], t1[kMbWideRows * 32], t2[kMbWideRows * 64], dp2[kMbWideRows * 64], dp1[kMbWideRows * 32];
    const int tid = threadIdx.x;
    mb_wide_rederive(x, T, fe, w1, b1, w2, b2, xs, t1, t2);
    for (int e = tid; e < T * 64; e += 256) {
        double s = 0.0;
#pragma unroll 8
        for (int c = 0; c < n_chunks; ++c) s += (double)part[(size_t)c * T * 64 + e];   // (loads in flight together, sums in order)
        const float tv = t2[e];
        dp2[e] = (float)s * tv * (1.0f - tv);
    }
    __syncthreads();
    for (int e = tid; e < 64 * 32; e += 256) {               // dW2 [64][32]
        const int j = e >> 5, k = e & 31;
        float a = 0.f;
        for (int r = 0; r < T; ++r) a = fmaf(dp2[r * 64 + j], t1[r * 32 + k], a);
        dw2[e] = a;
    }
    if (tid < 64) {
        float a = 0.f;
        for (int r = 0; r < T; ++r) a += dp2[r * 64 + tid];
        db2[tid] = a;
    }
    for (int e = tid; e < T * 32; e += 256) {
        const int r = e >> 5, k = e & 31;
        float a = 0.f;
#pragma unroll 8
        for (int j = 0; j < 64; ++j) a = fmaf(dp2[r * 64 + j], w2[j * 32 + k], a);
        const float tv = t1[e];
        dp1[e] = a * tv * (1.0f - tv);
    }
    __syncthreads();
    for (int e = tid; e < 32 * fe; e += 256) {               // dW1 [32][fe]
        const int j = e / fe, k = e - j * fe;
        float a = 0.f;
        for (int r = 0; r < T; ++r) a = fmaf(dp1[r * 32 + j], xs[r * fe + k], a);
        dw1[e] = a;
    }
    if (tid < 32) {
        float a = 0.f;
        for (int r = 0; r < T; ++r) a += dp1[r * 32 + tid];
        db1[tid] = a;
    }
}

static LdsOptIn g_mb_tall_lds, g_mb_tall64_lds;

}  // namespace tgnn

using namespace tgnn;

extern "C" {

int32_t tgnn_set_mlp_bwd_fused(int32_t on) {
    if (on != 0 && on != 1) return g_mlp_bwd_fused.load();
    return g_mlp_bwd_fused.exchange(on);
}

int32_t tgnn_sigmoid_mlp_bwd_fused_form(int64_t n_rows, int32_t d0, int32_t d1, int32_t d2, int32_t d3, int32_t want_dx) {
    return mlp_bwd_form(n_rows, d0, d1, d2, d3, want_dx);
}

size_t tgnn_sigmoid_mlp_bwd_fused_workspace_bytes(int64_t n_rows, int32_t d0, int32_t d1, int32_t d2, int32_t d3) {
    return mlp_bwd_fused_workspace_bytes(n_rows, d0, d1, d2, d3);
}

int tgnn_sigmoid_mlp_bwd_fused(const float *x, int64_t n_rows, int32_t d0, int32_t d1, int32_t d2, int32_t d3, const float *w1,
                               const float *b1, const float *w2, const float *b2, const float *w3, const float *t3,
                               const float *d_out, int64_t ld_dout, float *dw1, float *db1, float *dw2, float *db2, float *dw3,
                               float *db3, float *dx, void *ws, size_t ws_bytes, tgnn_stream_t stream) {
    DeviceGuard guard__(stream);
    const int form = mlp_bwd_form(n_rows, d0, d1, d2, d3, dx ? 1 : 0);
    if (form == 0) {
        set_error("tgnn_sigmoid_mlp_bwd_fused: no fused form for %lld rows of %d -> %d -> %d -> %d%s (tall: 32 -> 32 -> 64 -> 32; "
                  "wide: up to 63 rows of up to 64 -> 32 -> 64 -> a multiple of 64, no input gradient)",
                  (long long)n_rows, d0, d1, d2, d3, dx ? " with an input gradient" : "");
        return TGNN_ERR_UNSUPPORTED;
    }
    TGNN_CHECK_ARG(w1 && b1 && w2 && b2 && w3 && dw1 && db1 && dw2 && db2 && dw3 && db3, "null pointer");
    hipStream_t s = (hipStream_t)stream;
    if (n_rows == 0) {
        const size_t sz[6] = {(size_t)d1 * d0, (size_t)d1, (size_t)d2 * d1, (size_t)d2, (size_t)d3 * d2, (size_t)d3};
        float *const out[6] = {dw1, db1, dw2, db2, dw3, db3};
        for (int k = 0; k < 6; ++k) TGNN_CHECK_HIP(hipMemsetAsync(out[k], 0, sizeof(float) * sz[k], s));
        return TGNN_OK;
    }
    TGNN_CHECK_ARG(x && t3 && d_out, "null pointer");
    TGNN_CHECK_ARG(ld_dout >= d3, "row stride of d_out");
    TGNN_CHECK_ARG(ws && ws_bytes >= mlp_bwd_fused_workspace_bytes(n_rows, d0, d1, d2, d3), "workspace");
    if (form == 1) {
        TGNN_CHECK_ARG(ld_dout % 4 == 0 && ((uintptr_t)x | (uintptr_t)t3 | (uintptr_t)d_out | (uintptr_t)dx) % 16 == 0,
                       "x, t3, d_out, dx aligned to 16 bytes, row stride of d_out a multiple of 4");
        const int nblk = mlp_bwd_tall_blocks(n_rows);
        TGNN_CHECK_HIP(opt_in_dynamic_lds(mlp_bwd_tall_kernel, kMbLdsBytes, g_mb_tall_lds));
        float *partial = static_cast<float *>(ws);
        hipLaunchKernelGGL(mlp_bwd_tall_kernel, dim3(nblk), dim3(kMlpBwdThreads), kMbLdsBytes, s, x, t3, d_out, ld_dout, w1, b1,
                           w2, b2, w3, n_rows, dx, partial);
        const MlpBwdOut outs{dw1, db1, dw2, db2, dw3, db3};
        hipLaunchKernelGGL(mlp_bwd_fold_kernel, dim3((kMlpBwdRowFloats + 15) / 16), dim3(256), 0, s, partial, nblk, outs);
    } else {
        const int chunks = mlp_bwd_wide_chunks(d3);
        float *part = static_cast<float *>(ws);
        hipLaunchKernelGGL(mlp_bwd_wide_a_kernel, dim3(chunks), dim3(256), 0, s, x, (int)n_rows, d0, d3, w1, b1, w2, b2, w3, t3,
                           d_out, ld_dout, dw3, db3, part);
        hipLaunchKernelGGL(mlp_bwd_wide_b_kernel, dim3(1), dim3(256), 0, s, x, (int)n_rows, d0, w1, b1, w2, b2, part, chunks, dw1,
                           db1, dw2, db2);
    }
    TGNN_CHECK_LAUNCH();
    return TGNN_OK;
}

int32_t tgnn_set_mlp_bwd_tall64(int32_t on) {
    if (on != 0 && on != 1) return g_mlp_bwd_tall64.load();
    return g_mlp_bwd_tall64.exchange(on);
}

int32_t tgnn_sigmoid_mlp_bwd_tall64_ok(int64_t n_rows, int32_t d0, int32_t d1, int32_t d2, int32_t d3) {
    return mlp_bwd_tall64_ok(n_rows, d0, d1, d2, d3) ? 1 : 0;
}

size_t tgnn_sigmoid_mlp_bwd_tall64_workspace_bytes(int64_t n_rows, int32_t d0, int32_t d1, int32_t d2, int32_t d3) {
    return mlp_bwd_tall64_workspace_bytes(n_rows, d0, d1, d2, d3);
}

int tgnn_sigmoid_mlp_bwd_tall64(const float *x, int64_t n_rows, int32_t d0, int32_t d1, int32_t d2, int32_t d3, const float *w1,
                                const float *b1, const float *w2, const float *b2, const float *w3, const float *t3,
                                const float *d_out, int64_t ld_dout, float *dw1, float *db1, float *dw2, float *db2, float *dw3,
                                float *db3, float *dx, void *ws, size_t ws_bytes, tgnn_stream_t stream) {
    DeviceGuard guard__(stream);
    if (!mlp_bwd_tall64_ok(n_rows, d0, d1, d2, d3)) {
        set_error("tgnn_sigmoid_mlp_bwd_tall64: no tall64 form for %lld rows of %d -> %d -> %d -> %d (64 -> 32 -> 64 -> 64 only)",
                  (long long)n_rows, d0, d1, d2, d3);
        return TGNN_ERR_UNSUPPORTED;
    }
    TGNN_CHECK_ARG(w1 && b1 && w2 && b2 && w3 && dw1 && db1 && dw2 && db2 && dw3 && db3, "null pointer");
    hipStream_t s = (hipStream_t)stream;
    if (n_rows == 0) {
        const size_t sz[6] = {(size_t)d1 * d0, (size_t)d1, (size_t)d2 * d1, (size_t)d2, (size_t)d3 * d2, (size_t)d3};
        float *const out[6] = {dw1, db1, dw2, db2, dw3, db3};
        for (int k = 0; k < 6; ++k) TGNN_CHECK_HIP(hipMemsetAsync(out[k], 0, sizeof(float) * sz[k], s));
        return TGNN_OK;
    }
    TGNN_CHECK_ARG(x && t3 && d_out, "null pointer");
    TGNN_CHECK_ARG(ld_dout >= d3, "row stride of d_out");
    TGNN_CHECK_ARG(ws && ws_bytes >= mlp_bwd_tall64_workspace_bytes(n_rows, d0, d1, d2, d3), "workspace");
    TGNN_CHECK_ARG(ld_dout % 4 == 0 && ((uintptr_t)x | (uintptr_t)t3 | (uintptr_t)d_out | (uintptr_t)dx) % 16 == 0,
                   "x, t3, d_out, dx aligned to 16 bytes, row stride of d_out a multiple of 4");
    const int nblk = mlp_bwd_tall64_blocks(n_rows);
    TGNN_CHECK_HIP(opt_in_dynamic_lds(mlp_bwd_tall64_kernel, kMb64LdsBytes, g_mb_tall64_lds));
    float *partial = static_cast<float *>(ws);
    hipLaunchKernelGGL(mlp_bwd_tall64_kernel, dim3(nblk), dim3(kMlpBwd64Threads), kMb64LdsBytes, s, x, t3, d_out, ld_dout, w1, b1, w2,
                       b2, w3, n_rows, dx, partial);
    const MlpBwdOut outs{dw1, db1, dw2, db2, dw3, db3};
    hipLaunchKernelGGL(mlp_bwd_fold64_kernel, dim3((kMlpBwd64RowFloats + 15) / 16), dim3(256), 0, s, partial, nblk, outs);
    TGNN_CHECK_LAUNCH();
    return TGNN_OK;
}

}  // extern "C"
