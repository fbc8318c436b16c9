// The sums of the unsupervised loss and of the solution score, stated once for the single-layout entries (csrc/loss.hip) and the
// K-layout entries (csrc/greedy_many.hip): the block count, what one thread adds up, the block and wavefront reductions over the
// fixed tree, and the product of the three factors.  A kernel keeps only its own indexing of `partial` and its error convention.
// The first half is plain C++ (no HIP header): tests/host/loss_sums_test.cpp walks it under AddressSanitizer and UBSan.
#ifndef TGNN_LOSS_SUMS_H
#define TGNN_LOSS_SUMS_H
#include <math.h>
#include <stdint.h>

#include "many_desc.h"

namespace tgnn {

constexpr float kLossEps = 1e-7f;                           // losses.py:10
constexpr int kLossThreads = 256;
constexpr int kLossMaxBlocks = 512;                         // partial rows per (layout, map)
static_assert(kChunk == kLossThreads * 4 && kMnThreads == kLossThreads,
              "a `_many` block and a single-layout block walk the same items: loss_blocks counts in chunks of kChunk");

// blocks that share the sums of a layout of n nodes, ec collision edges and ea adjacency edges (0: a set the sums do not read)
TGNN_MANY_FN int loss_blocks(int64_t n, int64_t ec, int64_t ea) {
    int64_t work = n > ec ? n : ec;
    if (ea > work) work = ea;
    const int64_t b = (work + kChunk - 1) / kChunk;
    return (int)(b < 1 ? 1 : (b > kLossMaxBlocks ? kLossMaxBlocks : b));
}

// what thread t0 of a grid of `stride` threads adds to the three sums of the loss on one layout's arrays (p: the map's column).
// An edge end outside [0, n) is skipped and reported: torch.gather raises there.
TGNN_MANY_FN void loss_accumulate(int64_t n, int64_t ec, int64_t ea, const float *p, int64_t ldp, const float *area, int64_t lda,
                                  const int64_t *col, const int64_t *adj, const float *len, int64_t ldl, int64_t t0, int64_t stride,
                                  double &s_area, double &s_feas, double &s_align, bool &bad) {
    for (int64_t i = t0; i < n; i += stride) s_area += (double)(area[i * lda] * p[i * ldp]);
    for (int64_t e = t0; e < ec; e += stride) {
        const int64_t i = col[e], j = col[ec + e];
        if (i < 0 || i >= n || j < 0 || j >= n) { bad = true; continue; }
        float pp = p[i * ldp] * p[j * ldp];
        pp = fminf(fmaxf(pp, kLossEps), 1.0f - kLossEps);
        s_feas += (double)logf(1.0f - pp);
    }
    for (int64_t e = t0; e < ea; e += stride) {
        const int64_t i = adj[e], j = adj[ea + e];
        if (i < 0 || i >= n || j < 0 || j >= n) { bad = true; continue; }
        float pp = p[i * ldp] * p[j * ldp] * len[e * ldl];
        pp = fmaxf(pp, kLossEps);
        s_align += (double)(logf(pp) / 2.302585092994046f);
    }
}

// the same for the three sums of the solution score (losses.py:120-148): products in fp32 like the reference
TGNN_MANY_FN void score_accumulate(int64_t n, int64_t ea, const float *predict, const float *area, int64_t lda, const float *perim,
                                   const int64_t *adj, const float *len, int64_t ldl, int64_t t0, int64_t stride, double &s0,
                                   double &s1, double &s2, bool &bad) {
    for (int64_t v = t0; v < n; v += stride) {
        const float p = predict[v];
        s0 += (double)(p * area[v * lda]);
        if (p == 1.0f) s2 += (double)perim[v];
    }
    for (int64_t e = t0; e < ea; e += stride) {
        const int64_t i = adj[e], j = adj[ea + e];
        if (i < 0 || i >= n || j < 0 || j >= n) { bad = true; continue; }
        s1 += (double)(predict[i] * predict[j] * len[e * ldl]);
    }
}

// loss = (1 - Wa l_area) (1 - Wc l_feas) (1 - Wl l_align) from the three sums (losses.py:65-106); t: the three terms
TGNN_MANY_FN double loss_from_sums(const double *s, int64_t n, int64_t ec, int64_t ea, float wc, float wl, float wa, double *t) {
    t[0] = log(fmax(s[0] / (double)n, (double)kLossEps));
    t[1] = ec > 0 ? s[1] / (double)ec : 0.0;
    t[2] = ea > 0 ? s[2] / (double)ea : 0.0;
    return (1.0 - (double)wa * t[0]) * (1.0 - (double)wc * t[1]) * (1.0 - (double)wl * t[2]);
}

#if defined(__HIPCC__)
// the three sums of a block of kLossThreads threads over a fixed tree; row: where the block's partial row [3] goes
__device__ __forceinline__ void loss_block_reduce(double s0, double s1, double s2, double *__restrict__ row) {
    __shared__ double red[3][kLossThreads];
    red[0][threadIdx.x] = s0; red[1][threadIdx.x] = s1; red[2][threadIdx.x] = s2;
    __syncthreads();
    for (int d = kLossThreads / 2; d >= 1; d >>= 1) {
        if ((int)threadIdx.x < d)
            for (int k = 0; k < 3; ++k) red[k][threadIdx.x] += red[k][threadIdx.x + d];
        __syncthreads();
    }
    if (threadIdx.x < 3) row[threadIdx.x] = red[threadIdx.x][0];
}

// one wavefront sums n_blocks <= kLossMaxBlocks partial rows over a fixed tree: lane l takes rows l, l + 64, ..; then a butterfly
// leaves the sums in every lane.  (A first version let three threads walk the rows one dependent load after the other: 50 us.)
__device__ __forceinline__ void loss_fold_rows(const double *__restrict__ rows, int n_blocks, double (&s)[3]) {
    s[0] = s[1] = s[2] = 0.0;
    for (int b = threadIdx.x; b < n_blocks; b += 64)
#pragma unroll
        for (int k = 0; k < 3; ++k) s[k] += rows[(int64_t)b * 3 + k];
#pragma unroll
    for (int k = 0; k < 3; ++k)
#pragma unroll
        for (int d = 32; d >= 1; d >>= 1) s[k] += __shfl_xor(s[k], d, 64);
}

__device__ __forceinline__ double loss_nan() { return __longlong_as_double(0x7ff8000000000000ll); }
#endif

}  // namespace tgnn
#endif
