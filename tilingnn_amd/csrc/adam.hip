// Fused Adam step: every parameter tensor of a group updated by ONE launch.
//
// torch.optim.Adam's non-capturable single-tensor semantics, element by element in fp32:
//     g  = grad (+ weight_decay * p  when weight_decay != 0)
//     m' = beta1 m + (1 - beta1) g
//     v' = beta2 v + (1 - beta2) g g
//     p' = p - step_size m' / (sqrt(v') rsqrt_bc2 + eps)          step_size = lr / (1 - beta1^t), rsqrt_bc2 = 1 / sqrt(1 - beta2^t)
// The scalars come from the host (computed there in double, rounded to fp32 once).  A block takes one chunk of the plan
// (adam_plan.h): at most kAdamChunk consecutive elements of one segment, 128-bit loads and stores where parameter, gradient and
// both moments are 16-byte aligned, element by element otherwise and in the tail.  Pure streaming: 4 reads and 3 writes per
// element, no atomics, no reduction, nothing waits for another block, so the same inputs give the same bits whatever the table
// looks like.  Square root and division are the correctly rounded ones (hipcc's default for fp32).
#include "adam_plan.h"
#include "tgnn_common.h"

namespace tgnn {
namespace {

struct AdamScalars {
    float step_size, rsqrt_bc2, beta1, one_minus_beta1, beta2, one_minus_beta2, eps, weight_decay;
};

__device__ __forceinline__ void adam_one(float &p, float g, float &m, float &v, const AdamScalars &k) {
    if (k.weight_decay != 0.f) g = fmaf(k.weight_decay, p, g);                 // (uniform)
    m = fmaf(k.beta1, m, k.one_minus_beta1 * g);
    v = fmaf(k.beta2, v, (k.one_minus_beta2 * g) * g);
    const float den = fmaf(sqrtf(v), k.rsqrt_bc2, k.eps);
    p = fmaf(-k.step_size, m / den, p);
}

constexpr int kAdamThreads = 256;

__global__ __launch_bounds__(kAdamThreads) void adam_step_kernel(const AdamSegment *__restrict__ segs,
                                                                  const AdamChunk *__restrict__ chunks, const char *grad_base,
                                                                  float *exp_avg, float *exp_avg_sq, AdamScalars k) {
    const AdamChunk ch = chunks[blockIdx.x];
    const AdamSegment sg = segs[ch.segment];
    const int64_t left = sg.numel - ch.start;
    const int n = left < kAdamChunk ? (int)left : (int)kAdamChunk;
    float *p = sg.param + ch.start;
    const float *g = reinterpret_cast<const float *>(grad_base + sg.grad_off) + ch.start;
    float *m = exp_avg + sg.moment_off + ch.start;
    float *v = exp_avg_sq + sg.moment_off + ch.start;
    const int tid = threadIdx.x;
    const bool aligned = (((uintptr_t)p | (uintptr_t)g | (uintptr_t)m | (uintptr_t)v) & 15u) == 0;   // (uniform)
    int done = 0;
    if (aligned) {
        const int n4 = n >> 2;
        float4 *p4 = reinterpret_cast<float4 *>(p), *m4 = reinterpret_cast<float4 *>(m), *v4 = reinterpret_cast<float4 *>(v);
        const float4 *g4 = reinterpret_cast<const float4 *>(g);
        for (int i = tid; i < n4; i += kAdamThreads) {
            float4 pp = p4[i], mm = m4[i], vv = v4[i];
            const float4 gg = g4[i];
            adam_one(pp.x, gg.x, mm.x, vv.x, k);
            adam_one(pp.y, gg.y, mm.y, vv.y, k);
            adam_one(pp.z, gg.z, mm.z, vv.z, k);
            adam_one(pp.w, gg.w, mm.w, vv.w, k);
            p4[i] = pp;
            m4[i] = mm;
            v4[i] = vv;
        }
        done = n4 << 2;
    }
    for (int i = done + tid; i < n; i += kAdamThreads) {
        float pp = p[i], mm = m[i], vv = v[i];
        adam_one(pp, g[i], mm, vv, k);
        p[i] = pp;
        m[i] = mm;
        v[i] = vv;
    }
}

}  // namespace
}  // namespace tgnn

using namespace tgnn;

extern "C" {

int64_t tgnn_adam_chunk_elems(void) { return kAdamChunk; }

int64_t tgnn_adam_chunk_count(const int64_t *numel, int32_t n_segments) { return adam_chunk_count(numel, n_segments); }

size_t tgnn_adam_table_bytes(int32_t n_segments, int64_t n_chunks) { return adam_table_bytes(n_segments, n_chunks); }

int tgnn_adam_table_build(const void *const *params, const int64_t *grad_off_bytes, const int64_t *moment_off,
                          const int64_t *numel, int32_t n_segments, int64_t moment_floats, void *table_host,
                          size_t table_bytes, int64_t *n_chunks_out) {
    TGNN_CHECK_ARG(n_segments >= 0 && moment_floats >= 0, "negative count");
    TGNN_CHECK_ARG(n_chunks_out, "null pointer");
    TGNN_CHECK_ARG(n_segments == 0 || (params && grad_off_bytes && moment_off && numel && table_host), "null pointer");
    const int64_t n_chunks = adam_chunk_count(numel, n_segments);
    TGNN_CHECK_ARG(n_chunks >= 0, "negative element count, or more chunks than one launch holds");
    TGNN_CHECK_ARG(table_bytes >= adam_table_bytes(n_segments, n_chunks), "table buffer too small");
    TGNN_CHECK_ARG(((uintptr_t)table_host & 7u) == 0, "table buffer is not 8-byte aligned");
    AdamSegment *segs = static_cast<AdamSegment *>(table_host);
    for (int32_t s = 0; s < n_segments; ++s)
        segs[s] = AdamSegment{static_cast<float *>(const_cast<void *>(params[s])), grad_off_bytes[s], moment_off[s], numel[s]};
    if (const char *why = adam_check_segments(segs, n_segments, moment_floats)) {
        set_error("tgnn_adam_table_build: invalid argument: %s", why);
        return TGNN_ERR_INVALID_ARG;
    }
    AdamChunk *chunks = const_cast<AdamChunk *>(adam_table_chunks(table_host, n_segments));
    const int64_t cut = adam_cut_chunks(segs, n_segments, chunks);
    if (cut != n_chunks || adam_check_chunks(segs, n_segments, chunks, cut)) {
        set_error("tgnn_adam_table_build: the chunk list does not tile the segments");
        return TGNN_ERR_INVALID_ARG;
    }
    *n_chunks_out = n_chunks;
    return TGNN_OK;
}

int tgnn_adam_step(const void *table_host, const void *table_dev, int32_t n_segments, int64_t n_chunks, const void *grad_base,
                   float *exp_avg, float *exp_avg_sq, int64_t moment_floats, double step_size, double rsqrt_bc2, double beta1,
                   double beta2, double eps, double weight_decay, tgnn_stream_t stream) {
    DeviceGuard guard__(stream);
    TGNN_CHECK_ARG(n_segments >= 0 && n_chunks >= 0 && moment_floats >= 0, "negative count");
    if (n_chunks == 0) return TGNN_OK;
    // the host image first: a bad table is refused whatever else the call carries
    TGNN_CHECK_ARG(table_host && ((uintptr_t)table_host & 7u) == 0, "host table is null or not 8-byte aligned");
    const AdamSegment *segs = static_cast<const AdamSegment *>(table_host);
    const char *why = adam_check_segments(segs, n_segments, moment_floats);
    if (!why) why = adam_check_chunks(segs, n_segments, adam_table_chunks(table_host, n_segments), n_chunks);
    if (why) {
        set_error("tgnn_adam_step: invalid argument: %s", why);
        return TGNN_ERR_INVALID_ARG;
    }
    TGNN_CHECK_ARG(table_dev && grad_base && exp_avg && exp_avg_sq, "null pointer");
    TGNN_CHECK_ARG(((uintptr_t)table_dev & 7u) == 0, "device table is not 8-byte aligned");
    TGNN_CHECK_ARG(((uintptr_t)grad_base & 3u) == 0 && ((uintptr_t)exp_avg & 255u) == 0 && ((uintptr_t)exp_avg_sq & 255u) == 0,
                   "gradient base or moment buffers misaligned");
    TGNN_CHECK_ARG(exp_avg != exp_avg_sq, "the two moment buffers are the same");
    const AdamScalars k{(float)step_size,     (float)rsqrt_bc2,      (float)beta1, (float)(1.0 - beta1),
                        (float)beta2,         (float)(1.0 - beta2), (float)eps,   (float)weight_decay};
    hipLaunchKernelGGL(adam_step_kernel, dim3((unsigned)n_chunks), dim3(kAdamThreads), 0, (hipStream_t)stream,
                       static_cast<const AdamSegment *>(table_dev), adam_table_chunks(table_dev, n_segments),
                       static_cast<const char *>(grad_base), exp_avg, exp_avg_sq, k);
    TGNN_CHECK_LAUNCH();
    return TGNN_OK;
}

}  // extern "C"
