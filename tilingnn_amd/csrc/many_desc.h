// K packed layouts as the `_many` entries of csrc/greedy_many.hip see them: the offset tables, the sizes a call works on, and the
// view of one layout that the batched unsupervised loss takes.  Plain C++ (no HIP header): the kernels call these per block, and
// tests/host/loss_sums_test.cpp walks the very same code on random and deliberately broken tables under AddressSanitizer.
#ifndef TGNN_MANY_DESC_H
#define TGNN_MANY_DESC_H
#include <stdint.h>

#if defined(__HIPCC__)
#define TGNN_MANY_FN __host__ __device__ __forceinline__
#else
#define TGNN_MANY_FN inline
#endif

namespace tgnn {

constexpr int kMnThreads = 256;
constexpr int kMnSub = 4;                                   // sub-chunks of kMnThreads items per block
constexpr int kChunk = kMnThreads * kMnSub;

struct ManyDesc {
    int K;
    const int64_t *ptr[3];                                  // node / adjacency / collision offset tables [K + 1] (NULL: set unused)
    int64_t total[3];                                       // sizes of the packed arrays (host-known)
    const int32_t *active;                                  // [K] or NULL = every layout takes part
    const int64_t *counts;                                  // [K][3] sub-layout sizes, or NULL = the layouts' full sizes
};

// full size of set `s` of layout k, 0 (and bad = true) when the offset table is not 0 <= ptr[k] <= ptr[k + 1] <= total
TGNN_MANY_FN int64_t many_full_size(const ManyDesc &d, int s, int k, bool &bad) {
    const int64_t a = d.ptr[s][k], b = d.ptr[s][k + 1];
    if (a < 0 || b < a || b > d.total[s] || b - a >= (1ll << 31) - 1) { bad = true; return 0; }
    return b - a;
}
// the size this call works on: 0 for an inactive layout; the sub-layout count (checked against the full size) when counts are given
TGNN_MANY_FN int64_t many_size(const ManyDesc &d, int s, int k, bool &bad) {
    if (d.active && d.active[k] == 0) return 0;
    const int64_t full = many_full_size(d, s, k, bad);
    if (!d.counts) return full;
    const int64_t c = d.counts[(int64_t)k * 3 + s];
    if (c < 0 || c > full) { bad = true; return 0; }
    return c;
}

// ---- the unsupervised loss of K layouts: what a layout contributes, where its arrays start
struct LossManyView {
    int64_t n, ec, ea;                                      // sizes this call works on (the sub-layout's with counts)
    int64_t np, ap, cp;                                     // first node / adjacency edge / collision edge in the packed arrays
};
// false: nothing to compute -- inactive or without nodes (bad stays false), or an offset / count out of range (bad = true).
// Every offset is checked against the packed sizes before it is returned.
TGNN_MANY_FN bool loss_many_view(const ManyDesc &d, int k, LossManyView &v, bool &bad) {
    bad = false;
    v.n = many_size(d, 0, k, bad);
    v.ea = many_size(d, 1, k, bad);
    v.ec = many_size(d, 2, k, bad);
    if (bad || v.n == 0) return false;
    v.np = d.ptr[0][k]; v.ap = d.ptr[1][k]; v.cp = d.ptr[2][k];
    return true;
}

}  // namespace tgnn
#endif
