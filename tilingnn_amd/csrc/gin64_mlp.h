// The width-64 fp32 GIN layer on the matrix cores (gin64_mlp.hip) as the forward launches it (forward.hip).
#pragma once
#include "tgnn_common.h"
#include "gin64_plan.h"

namespace tgnn {

// gin_aggregate_kernel<64> into z [n_nodes][64] (16-byte aligned; the training forward keeps it), then gin64_mlp_kernel on z:
// out [n_nodes][64], BatchNorm partial rows double [blocks][sum 64 | sum of squares 64] (bn_partial may be NULL)
int gin64_fwd(const float *a, int64_t lda, const float *in_stat, const int32_t *rowptr, const int32_t *col_src, const float *eps,
              const float *w1, const float *b1, const float *w2, const float *b2, const float *w3, const float *b3, int64_t n_nodes,
              int32_t act, float *out, float *z, double *bn_partial, int32_t *n_partials_host, hipStream_t s);

}  // namespace tgnn
