// The unsupervised loss on the predict path.
//
// Reference: Losses.calculate_unsupervised_loss, /root/reference/solver/ml_solver/losses.py:48-116, called from
// ML_Solver.predict through get_best_prob_map (ml_solver.py:46,133-136).  Per probability map m:
//     l_area  = log( max( mean_v area[v] p[v], eps ) )                                   (:65-67)
//     l_feas  = mean_{collision edges (i,j)} log( 1 - clamp(p[i] p[j], eps, 1 - eps) )     (:69-81)   0 without such edges
//     l_align = mean_{adjacency edges (i,j)} log10( max(p[i] p[j] len_e, eps) )            (:83-98)   0 without such edges
//     loss    = (1 - Wa l_area) (1 - Wc l_feas) (1 - Wl l_align)                           (:104-106)
// The reference evaluates every element in fp32 and sums in fp32; here the elements are fp32 (same clamp / log) and
// the three sums run in fp64 over a fixed tree: per-block partials, then one block per map.  Two launches, no atomics.
#include "tgnn_common.h"
#include "loss_sums.h"

namespace tgnn {

// grid = (blocks, maps); partial[(m * gridDim.x + b) * 3 + {0,1,2}]
__global__ __launch_bounds__(kLossThreads) void loss_partial_kernel(
    const float *__restrict__ probs, int64_t ldp, const float *__restrict__ area, int64_t lda, int64_t n,
    const int64_t *__restrict__ col, int64_t ec, const int64_t *__restrict__ adj, int64_t ea,
    const float *__restrict__ len, int64_t ldl, double *__restrict__ partial, int *__restrict__ err_flag) {
    const int m = blockIdx.y;
    double s_area = 0.0, s_feas = 0.0, s_align = 0.0;
    bool bad = false;
    loss_accumulate(n, ec, ea, probs + m, ldp, area, lda, col, adj, len, ldl, (int64_t)blockIdx.x * kLossThreads + threadIdx.x,
                    (int64_t)gridDim.x * kLossThreads, s_area, s_feas, s_align, bad);
    if (bad) *err_flag = 1;
    loss_block_reduce(s_area, s_feas, s_align, partial + ((int64_t)m * gridDim.x + blockIdx.x) * 3);
}

// one wavefront per map: the map's partial rows folded, then the product of the three factors
__global__ __launch_bounds__(64) void loss_final_kernel(const double *__restrict__ partial, int n_blocks, int64_t n,
                                                        int64_t ec, int64_t ea, float wc, float wl, float wa,
                                                        double *__restrict__ losses, double *__restrict__ terms,
                                                        const int *__restrict__ err_flag) {
    const int m = blockIdx.x;
    double s[3];
    loss_fold_rows(partial + (int64_t)m * n_blocks * 3, n_blocks, s);
    if (threadIdx.x == 0) {
        double t[3];
        const double l = loss_from_sums(s, n, ec, ea, wc, wl, wa, t);
        if (terms) { terms[m * 3] = t[0]; terms[m * 3 + 1] = t[1]; terms[m * 3 + 2] = t[2]; }
        losses[m] = *err_flag ? loss_nan() : l;               // NaN = "edge index out of range"
    }
}

// ---- Losses.solution_score (losses.py:120-148): the three sums of the score of a 0/1 selection
//   s0 = sum_v predict[v] area_ratio[v]                 (:126: predict . (x[:, -1] max_area) / contour area)
//   s1 = sum_e predict[i_e] predict[j_e] len_ratio[e]   (:131-141: (p_i p_j) . (len max_align_length))
//   s2 = sum_{v: predict[v] == 1} perimeter[v]          (:143-144)
// products in fp32 like the reference, sums in fp64 over the fixed tree of the loss kernels.
__global__ __launch_bounds__(kLossThreads) void score_partial_kernel(
    const float *__restrict__ predict, const float *__restrict__ area, int64_t lda, const float *__restrict__ perim,
    int64_t n, const int64_t *__restrict__ adj, int64_t ea, const float *__restrict__ len, int64_t ldl,
    double *__restrict__ partial, int *__restrict__ err_flag) {
    double s0 = 0.0, s1 = 0.0, s2 = 0.0;
    bool bad = false;
    score_accumulate(n, ea, predict, area, lda, perim, adj, len, ldl, (int64_t)blockIdx.x * kLossThreads + threadIdx.x,
                     (int64_t)gridDim.x * kLossThreads, s0, s1, s2, bad);
    if (bad) *err_flag = 1;
    loss_block_reduce(s0, s1, s2, partial + (int64_t)blockIdx.x * 3);
}

__global__ __launch_bounds__(64) void score_final_kernel(const double *__restrict__ partial, int n_blocks,
                                                         const int *__restrict__ err_flag, double *__restrict__ sums) {
    const int lane = threadIdx.x;
    double s[3];
    loss_fold_rows(partial, n_blocks, s);
    if (lane < 3) sums[lane] = *err_flag ? loss_nan() : s[lane];
}

}  // namespace tgnn

using namespace tgnn;

extern "C" size_t tgnn_unsupervised_loss_workspace_bytes(int32_t n_maps) {
    return (size_t)(n_maps > 0 ? n_maps : 1) * kLossMaxBlocks * 3 * sizeof(double) + 256;     // partial rows + the error flag
}

extern "C" int tgnn_unsupervised_loss(const float *probs, int64_t ld_probs, int32_t n_maps, const float *area_ratio,
                                      int64_t ld_area, int64_t n_nodes, const int64_t *col_edge_index,
                                      int64_t n_col_edges, const int64_t *adj_edge_index, int64_t n_adj_edges,
                                      const float *adj_edge_len, int64_t ld_len, float collision_weight,
                                      float align_length_weight, float avg_area_weight, double *losses,
                                      double *terms, void *ws, size_t ws_bytes, tgnn_stream_t stream) {
    DeviceGuard guard__(stream);
    TGNN_CHECK_ARG(n_maps >= 1 && n_maps <= 65535 && n_nodes >= 1, "shape");
    TGNN_CHECK_ARG(probs && area_ratio && losses && ld_probs >= n_maps && ld_area >= 1, "null pointer / strides");
    TGNN_CHECK_ARG(n_col_edges >= 0 && (n_col_edges == 0 || col_edge_index), "collision edges");
    TGNN_CHECK_ARG(n_adj_edges >= 0 && (n_adj_edges == 0 || (adj_edge_index && adj_edge_len && ld_len >= 1)), "adjacency edges");
    if (!ws || ws_bytes < tgnn_unsupervised_loss_workspace_bytes(n_maps)) {
        set_error("tgnn_unsupervised_loss: workspace too small");
        return TGNN_ERR_WORKSPACE;
    }
    hipStream_t s = static_cast<hipStream_t>(stream);
    double *partial = static_cast<double *>(ws);
    int *err_flag = reinterpret_cast<int *>(partial + (size_t)n_maps * kLossMaxBlocks * 3);
    TGNN_CHECK_HIP(hipMemsetAsync(err_flag, 0, sizeof(int), s));
    const int blocks = loss_blocks(n_nodes, n_col_edges, n_adj_edges);
    loss_partial_kernel<<<dim3(blocks, n_maps), kLossThreads, 0, s>>>(probs, ld_probs, area_ratio, ld_area, n_nodes,
                                                                      col_edge_index, n_col_edges, adj_edge_index,
                                                                      n_adj_edges, adj_edge_len, ld_len, partial, err_flag);
    loss_final_kernel<<<n_maps, 64, 0, s>>>(partial, blocks, n_nodes, n_col_edges, n_adj_edges, collision_weight,
                                            align_length_weight, avg_area_weight, losses, terms, err_flag);
    TGNN_CHECK_LAUNCH();
    return TGNN_OK;
}

extern "C" int tgnn_solution_score_sums(const float *predict, const float *area_ratio, int64_t ld_area,
                                        const float *perimeter, int64_t n_nodes, const int64_t *adj_edge_index,
                                        int64_t n_adj_edges, const float *adj_edge_len, int64_t ld_len, double *sums,
                                        void *ws, size_t ws_bytes, tgnn_stream_t stream) {
    DeviceGuard guard__(stream);
    TGNN_CHECK_ARG(n_nodes >= 1 && predict && area_ratio && perimeter && sums && ld_area >= 1, "null pointer / shape");
    TGNN_CHECK_ARG(n_adj_edges >= 0 && (n_adj_edges == 0 || (adj_edge_index && adj_edge_len && ld_len >= 1)), "adjacency edges");
    if (!ws || ws_bytes < tgnn_unsupervised_loss_workspace_bytes(1)) {
        set_error("tgnn_solution_score_sums: workspace too small (tgnn_unsupervised_loss_workspace_bytes(1))");
        return TGNN_ERR_WORKSPACE;
    }
    hipStream_t s = static_cast<hipStream_t>(stream);
    double *partial = static_cast<double *>(ws);
    int *err_flag = reinterpret_cast<int *>(partial + (size_t)kLossMaxBlocks * 3);
    TGNN_CHECK_HIP(hipMemsetAsync(err_flag, 0, sizeof(int), s));
    const int blocks = loss_blocks(n_nodes, 0, n_adj_edges);
    score_partial_kernel<<<blocks, kLossThreads, 0, s>>>(predict, area_ratio, ld_area, perimeter, n_nodes, adj_edge_index,
                                                         n_adj_edges, adj_edge_len, ld_len, partial, err_flag);
    score_final_kernel<<<1, 64, 0, s>>>(partial, blocks, err_flag, sums);
    TGNN_CHECK_LAUNCH();
    return TGNN_OK;
}
