// The width-64 fp32 NNConv on edge groups (nnconv64_eg.hip) as the forward launches it (forward.hip).
#pragma once
#include "tgnn_common.h"
#include "nnconv64_eg_plan.h"

namespace tgnn {

// fp16-pair weight images [depth][(T+1)][kEg64TypeFloats] from wtab_all [depth][T][64][64] and the layers' roots, one launch;
// root_max[i] = max |roots[i]| as float bits (what the kernel's unscale reads)
void launch_nnconv64_eg_images(const float *wtab_all, const float *const *roots, int n_types, int depth, float *wimg_all,
                               unsigned *root_max, hipStream_t s);
// h [n_src_rows][64] packed; h_max (device word, float bits): a bound of |h| over every row that can be gathered
int launch_nnconv64_eg(const float *h, int64_t n_src_rows, const int32_t *tile_grp_ptr, const int32_t *grp, const float *wimg,
                       int32_t n_types, const float *bias, int64_t n_nodes, int32_t act, float *out, double *bn_partial,
                       int32_t *n_partials_host, hipStream_t s, const unsigned *h_max, const unsigned *root_max,
                       const float *sum_root_rows = nullptr);
// (sum_root_rows given: the SUM form of the kernel -- edge sums instead of means, no bias / activation / BatchNorm partials, the
//  root group's rows read from sum_root_rows [n_src_rows][64]: the input gradient of the adjoint, nnconv_bwd_eg.hip)

}  // namespace tgnn
