// K independent greedy solves in ONE loop (tilingnn_amd.util.algorithms.solve_many_by_device_greedy): the bookkeeping of a round --
// sub-layout compaction (graph_prep.hip: tgnn_sublayout_compact), batched acceptance and the one-launch finish (greedy.hip), the
// sums of the solution score (loss.hip: tgnn_solution_score_sums) -- for K layouts per launch instead of per layout; and the
// unsupervised loss (loss.hip: tgnn_unsupervised_loss) of K layouts per call, for the best-map pick of a round and for the
// evaluation of a split (solver/ml_solver/trainer.py: cal_avg_loss_many).
//
// Reference: the crop loop of /root/reference/Tiling-Shape.py:60-64 calls solver.solve(layout) once per crop; the layouts have
// nothing to do with each other.
//
// PACKED LAYOUTS.  The K layouts' arrays are concatenated: nodes of layout k at node_ptr[k] .. node_ptr[k + 1], its adjacency
// edges at adj_ptr[k] .., its collision edges at col_ptr[k] .. (int64 [K + 1] on the device).  An edge index block of layout k is
// its own [2][E_k] array (row 1 starts E_k entries after row 0) at element 2 * ptr[k]; ends are LOCAL node numbers.  Outputs of
// layout k are written at layout k's own offsets into buffers sized for the un-compacted counts, a compacted [2][E'] block with
// rows E' apart -- so layout k's sub-layout is a plain view, and no scan crosses a layout boundary.
//
// GEOMETRY.  A layout's items (nodes, edges) are cut into chunks of kChunk; one block works on one chunk.  Which chunk a block
// owns is looked up ONCE PER BLOCK in a table of first-chunk numbers per layout (many_plan_kernel builds it on the device from the
// offset tables or from the sub-layout counts; thread 0 bisects, the block reads the answer from LDS).  The host only knows the
// totals, so the grid is an upper bound (total / kChunk + K) and surplus blocks leave at once.
//
// EQUALITY.  Per layout every entry computes exactly what its single-layout counterpart computes, because both call the same
// code: the acceptance rule and the finishing block of greedy_rule.h (mean, visiting order, test, draw keyed by (seed_k, round,
// local original node)), the block count, per-thread sums, reductions and final formula of loss_sums.h (same number of blocks
// per layout, same strides, same fixed tree).  Compaction keeps ascending order (block scans, chunk bases from a per-layout
// scan).  The only atomics add integers (n_selected) or store one value.  Every offset and index read from the device is
// range-checked (many_desc.h): a bad one sets the layout's error word and is skipped.
#include "tgnn_common.h"
#include "greedy_rule.h"
#include "loss_sums.h"

namespace tgnn {

// exclusive scan of one int per thread over the block (kMnThreads = 4 wavefronts); sh: >= 4 ints of LDS
__device__ __forceinline__ int block_excl_scan(int v, int *sh, int &total) {
    const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
    int inc = v;
#pragma unroll
    for (int d = 1; d < 64; d <<= 1) {
        const int t = __shfl_up(inc, d, 64);
        if (lane >= d) inc += t;
    }
    if (lane == 63) sh[w] = inc;
    __syncthreads();
    int off = 0;
    for (int i = 0; i < w; ++i) off += sh[i];
    total = sh[0] + sh[1] + sh[2] + sh[3];
    __syncthreads();
    return off + inc - v;
}

// start[s * (K + 1) + k] = number of blocks of set s in front of layout k (start[..K] = all of them).  mode 0: chunks of kChunk
// items; mode 1 (set 0 only): the block count of the score sums, loss_blocks(n, 0, ea); mode 2 (set 0 only): the block count
// of the unsupervised loss, loss_blocks(n, ec, ea) over the sizes this call works on (0 for a layout without nodes).
__global__ __launch_bounds__(kMnThreads) void many_plan_kernel(ManyDesc d, int n_sets, int mode, int *__restrict__ start,
                                                               int *__restrict__ err) {
    __shared__ int sh[4];
    for (int s = 0; s < n_sets; ++s) {
        if (!d.ptr[s]) continue;
        int carry = 0;
        for (int k0 = 0; k0 < d.K; k0 += kMnThreads) {
            const int k = k0 + threadIdx.x;
            int blocks = 0;
            if (k < d.K) {
                bool bad = false;
                if (mode == 0) {
                    blocks = (int)((many_size(d, s, k, bad) + kChunk - 1) / kChunk);
                } else if (mode == 2) {
                    LossManyView v;
                    blocks = loss_many_view(d, k, v, bad) ? loss_blocks(v.n, v.ec, v.ea) : 0;
                } else if (!(d.active && d.active[k] == 0)) {
                    const int64_t n = many_full_size(d, 0, k, bad), ea = many_full_size(d, 1, k, bad);
                    blocks = bad ? 0 : loss_blocks(n, 0, ea);
                }
                if (bad) err[k] = 1;
            }
            int total;
            const int ex = block_excl_scan(blocks, sh, total);
            if (k < d.K) start[s * (d.K + 1) + k] = carry + ex;
            carry += total;
        }
        if (threadIdx.x == 0) start[s * (d.K + 1) + d.K] = carry;
    }
}

// the layout and the chunk of block `b` of a set (start: that set's K + 1 entries); false = a surplus block
__device__ __forceinline__ bool many_find(const int *__restrict__ start, int K, int b, int &k, int &chunk) {
    __shared__ int found[2];
    if (threadIdx.x == 0) {
        int lo = 0, hi = K;                                 // largest lo with start[lo] <= b
        if (b >= start[K]) lo = -1;
        else
            while (hi - lo > 1) {
                const int mid = (lo + hi) >> 1;
                if (start[mid] <= b) lo = mid; else hi = mid;
            }
        found[0] = lo;
        found[1] = lo >= 0 ? b - start[lo] : 0;
    }
    __syncthreads();
    k = found[0];
    chunk = found[1];
    return k >= 0;
}
// which set a block of a combined grid belongs to: sets in order, ub[s] blocks each
__device__ __forceinline__ int many_set_of(int &b, int ub0, int ub1) {
    if (b < ub0) return 0;
    b -= ub0;
    if (b < ub1) return 1;
    b -= ub1;
    return 2;
}

// ------------------------------------------------------------------------------------------ compaction
struct CompactArgs {
    const int32_t *alive;
    const float *x;
    int fx;
    const int64_t *ei[2];                                   // adjacency, collision (packed)
    const float *attr;
    int fe;
    float *x_out;
    int64_t *inverse_out, *ei_out[2];
    float *attr_out;
    int64_t *counts_out;
    int32_t *err;
    int *start, *cnt, *npos;                                // workspace
    int ub[3];
};

// flag of item i of (set, layout k): node alive / edge with both ends alive (an end outside [0, n_k) sets the error word)
__device__ __forceinline__ int compact_flag(const ManyDesc &d, const CompactArgs &a, int set, int k, int64_t i, int64_t size, int64_t n_k,
                                            int64_t &ea, int64_t &eb) {
    if (i >= size) return 0;
    const int64_t np = d.ptr[0][k];
    if (set == 0) return a.alive[np + i] != 0;
    const int64_t *ei = a.ei[set - 1] + 2 * d.ptr[set][k];
    ea = ei[i];
    eb = ei[size + i];
    if (ea < 0 || ea >= n_k || eb < 0 || eb >= n_k) { a.err[k] = 1; return 0; }
    return a.alive[np + ea] != 0 && a.alive[np + eb] != 0;
}

__global__ __launch_bounds__(kMnThreads) void compact_count_kernel(ManyDesc d, CompactArgs a) {
    __shared__ int sh[4];
    int b = blockIdx.x, k, chunk;
    const int set = many_set_of(b, a.ub[0], a.ub[1]);
    if (!many_find(a.start + set * (d.K + 1), d.K, b, k, chunk)) return;
    bool bad = false;
    const int64_t size = many_size(d, set, k, bad), n_k = many_full_size(d, 0, k, bad);
    int mine = 0;
    int64_t ea, eb;
    for (int j = 0; j < kMnSub; ++j)
        mine += compact_flag(d, a, set, k, (int64_t)chunk * kChunk + j * kMnThreads + threadIdx.x, size, n_k, ea, eb);
#pragma unroll
    for (int s = 32; s >= 1; s >>= 1) mine += __shfl_xor(mine, s, 64);
    if ((threadIdx.x & 63) == 0) sh[threadIdx.x >> 6] = mine;
    __syncthreads();
    if (threadIdx.x == 0) a.cnt[blockIdx.x] = sh[0] + sh[1] + sh[2] + sh[3];
}

// per (layout, set): chunk counts -> chunk bases (in place), total -> counts_out
__global__ __launch_bounds__(kMnThreads) void compact_scan_kernel(ManyDesc d, CompactArgs a) {
    __shared__ int sh[4];
    const int k = blockIdx.x, set = blockIdx.y;
    if (d.active && d.active[k] == 0) return;
    const int *start = a.start + set * (d.K + 1);
    const int c0 = start[k], nc = start[k + 1] - c0;
    int *cnt = a.cnt + (set == 0 ? 0 : set == 1 ? a.ub[0] : a.ub[0] + a.ub[1]) + c0;
    int carry = 0;
    for (int t0 = 0; t0 < nc; t0 += kMnThreads) {
        const int t = t0 + threadIdx.x;
        const int v = t < nc ? cnt[t] : 0;
        int total;
        const int ex = block_excl_scan(v, sh, total);
        if (t < nc) cnt[t] = carry + ex;
        carry += total;
    }
    if (threadIdx.x == 0) a.counts_out[(int64_t)k * 3 + set] = carry;
}

// sets 0 (nodes: x_out, inverse_out, npos) in the first launch, 1 and 2 (edges, which read npos) in the second: set0 = first set
__global__ __launch_bounds__(kMnThreads) void compact_scatter_kernel(ManyDesc d, CompactArgs a, int edges) {
    __shared__ int sh[4];
    int b = blockIdx.x, k, chunk, set = 0;
    int cnt_at = b;
    if (edges) {
        set = b < a.ub[1] ? 1 : 2;
        if (set == 2) b -= a.ub[1];
        cnt_at = blockIdx.x + a.ub[0];
    }
    if (!many_find(a.start + set * (d.K + 1), d.K, b, k, chunk)) return;
    bool bad = false;
    const int64_t size = many_size(d, set, k, bad), n_k = many_full_size(d, 0, k, bad);
    const int64_t np = d.ptr[0][k], sp = d.ptr[set][k];
    int64_t pos0 = a.cnt[cnt_at];
    const int64_t e_out = edges ? a.counts_out[(int64_t)k * 3 + set] : 0;
    for (int j = 0; j < kMnSub; ++j) {
        const int64_t i = (int64_t)chunk * kChunk + j * kMnThreads + threadIdx.x;
        int64_t ea = 0, eb = 0;
        const int f = compact_flag(d, a, set, k, i, size, n_k, ea, eb);
        int total;
        const int64_t pos = pos0 + block_excl_scan(f, sh, total);
        pos0 += total;
        if (!f) continue;
        if (set == 0) {
            a.inverse_out[np + pos] = i;
            a.npos[np + i] = (int)pos;
            for (int c = 0; c < a.fx; ++c) a.x_out[(np + pos) * a.fx + c] = a.x[(np + i) * a.fx + c];
        } else {
            int64_t *out = a.ei_out[set - 1] + 2 * sp;
            out[pos] = a.npos[np + ea];
            out[e_out + pos] = a.npos[np + eb];
            if (set == 1)
                for (int c = 0; c < a.fe; ++c) a.attr_out[(sp + pos) * a.fe + c] = a.attr[(sp + i) * a.fe + c];
        }
    }
}

// ------------------------------------------------------------------------------------------ acceptance (greedy.hip, per layout)
struct RoundArgs {
    const float *const *prob;                               // [K] device pointers (NULL entry: probability 1 for every node)
    int64_t ldp;
    const int64_t *inverse, *col;                           // packed sub-layouts
    int round;
    const unsigned long long *seeds;
    double *saved;
    int32_t *alive, *selected;
    long long *n_selected;
    int32_t *err;
    int *start;
    double *p;
    int *flags;
};

// step 0: running mean, 1: beaten, 2: accept, 3: label -- greedy_{mean,beaten,accept,label}_kernel on the chunk of one layout
__global__ __launch_bounds__(kMnThreads) void round_step_kernel(ManyDesc d, RoundArgs a, int step) {
    int k, chunk;
    const int set = (step == 1 || step == 3) ? 2 : 0;
    if (!many_find(a.start + set * (d.K + 1), d.K, blockIdx.x, k, chunk)) return;
    bool bad = false;
    const int64_t n_sub = many_size(d, 0, k, bad), n_k = many_full_size(d, 0, k, bad);
    const int64_t np = d.ptr[0][k];
    const int64_t *inverse = a.inverse + np;
    double *p = a.p + np;
    int *flags = a.flags + np;
    int mine = 0;
    if (set == 0) {
        const float *prob = a.prob[k];
        const unsigned long long seed = a.seeds[k];
        for (int j = 0; j < kMnSub; ++j) {
            const int64_t i = (int64_t)chunk * kChunk + j * kMnThreads + threadIdx.x;
            if (i >= n_sub) continue;
            const int64_t o = inverse[i];
            if (o < 0 || o >= n_k) {                          // never accepted
                a.err[k] = 1;
                if (step == 0) { p[i] = 0.0; flags[i] = kGreedyBeaten; }
                continue;
            }
            if (step == 0) {
                const double pr = prob ? (double)prob[i * a.ldp] : (double)1.0f;
                const double v = greedy_mean(a.saved[np + o], pr, a.round);
                a.saved[np + o] = v;
                p[i] = v;
                flags[i] = 0;
            } else {
                if (flags[i] & kGreedyBeaten) continue;
                if (greedy_accepts(p[i], seed, a.round, o)) {
                    flags[i] = kGreedyAccepted;
                    a.alive[np + o] = 0;
                    a.selected[np + o] = a.round;
                    ++mine;
                }
            }
        }
        if (step == 2) {
#pragma unroll
            for (int s = 32; s >= 1; s >>= 1) mine += __shfl_xor(mine, s, 64);
            if ((threadIdx.x & 63) == 0 && mine)
                atomicAdd(reinterpret_cast<unsigned long long *>(a.n_selected + k), (unsigned long long)mine);
        }
        return;
    }
    const int64_t ec = many_size(d, 2, k, bad);
    const int64_t *col = a.col + 2 * d.ptr[2][k];
    for (int j = 0; j < kMnSub; ++j) {
        const int64_t e = (int64_t)chunk * kChunk + j * kMnThreads + threadIdx.x;
        if (e >= ec) continue;
        const int64_t u = col[e], v = col[ec + e];
        if (u < 0 || u >= n_sub || v < 0 || v >= n_sub) { a.err[k] = 1; continue; }
        if (step == 1) {
            if (u == v) continue;
            flags[greedy_beaten_end(u, v, p[u], p[v])] = kGreedyBeaten;   // (every writer stores the same word)
        } else if (flags[u] & kGreedyAccepted) {
            const int64_t o = inverse[v];
            if (o >= 0 && o < n_k) a.alive[np + o] = 0;
        }
    }
}

// greedy_finish_block on layout k's own arrays, one block per layout whose finish word is set
__global__ __launch_bounds__(kFinThreads) void finish_many_kernel(ManyDesc d, const int32_t *__restrict__ finish,
                                                                  const int64_t *__restrict__ inverse_all,
                                                                  const int64_t *__restrict__ col_all, int first_round, int max_rounds,
                                                                  const unsigned long long *__restrict__ seeds,
                                                                  double *__restrict__ saved_all, int *__restrict__ alive_all,
                                                                  int *__restrict__ selected_all, long long *__restrict__ count_all,
                                                                  int *__restrict__ err_all, int *__restrict__ out_all) {
    const int k = blockIdx.x;
    if (finish[k] == 0) return;
    int *out = out_all + 2 * k, *err = err_all + k;
    bool bad = false;
    const int64_t n64 = many_size(d, 0, k, bad), n_k = many_full_size(d, 0, k, bad), ec = many_size(d, 2, k, bad);
    if (bad || n64 > kFinMaxNodes) {                          // (uniform over the block)
        if (threadIdx.x == 0) { *err = 1; out[0] = 0; out[1] = (int)(n64 > 0x7fffffff ? 0x7fffffff : n64); }
        return;
    }
    const int64_t np = d.ptr[0][k];
    greedy_finish_block<true>(inverse_all + np, (int)n64, n_k, col_all + 2 * d.ptr[2][k], ec, first_round, max_rounds, seeds[k],
                              saved_all + np, alive_all + np, selected_all + np, count_all + k, err, out);
}

// ------------------------------------------------------------------------------------------ score sums (loss.hip, per layout)
__global__ __launch_bounds__(kMnThreads) void score_many_partial_kernel(ManyDesc d, const int *__restrict__ start,
                                                                        const float *__restrict__ predict_all,
                                                                        const float *__restrict__ area_all, int64_t lda,
                                                                        const float *__restrict__ perim_all,
                                                                        const int64_t *__restrict__ adj_all,
                                                                        const float *__restrict__ len_all, int64_t ldl,
                                                                        double *__restrict__ partial_all, int *__restrict__ err) {
    int k, bl;
    if (!many_find(start, d.K, blockIdx.x, k, bl)) return;
    const int nb = start[k + 1] - start[k];
    bool bad = false;
    const int64_t n = many_full_size(d, 0, k, bad), ea = many_full_size(d, 1, k, bad);
    const int64_t np = d.ptr[0][k], ap = d.ptr[1][k];
    double s0 = 0.0, s1 = 0.0, s2 = 0.0;
    score_accumulate(n, ea, predict_all + np, area_all + np * lda, lda, perim_all + np, adj_all + 2 * ap, len_all + ap * ldl, ldl,
                     (int64_t)bl * kMnThreads + threadIdx.x, (int64_t)nb * kMnThreads, s0, s1, s2, bad);
    if (bad) err[k] = 1;
    loss_block_reduce(s0, s1, s2, partial_all + ((int64_t)k * kLossMaxBlocks + bl) * 3);
}

__global__ __launch_bounds__(64) void score_many_final_kernel(int K, const int32_t *__restrict__ active, const int *__restrict__ start,
                                                              const double *__restrict__ partial_all, const int *__restrict__ err,
                                                              double *__restrict__ sums) {
    const int k = blockIdx.x, lane = threadIdx.x;
    if (active && active[k] == 0) return;
    double s[3];
    loss_fold_rows(partial_all + (int64_t)k * kLossMaxBlocks * 3, start[k + 1] - start[k], s);
    if (lane < 3) sums[(int64_t)k * 3 + lane] = err[k] ? loss_nan() : s[lane];
}

// ------------------------------------------------------------------------------------------ unsupervised loss (loss.hip, per layout)
struct LossManyArgs {
    const float *const *probs;                              // [K] device pointers: layout k's [n_k, ldp]
    int64_t ldp;
    int n_maps;
    const float *area;
    int64_t lda;
    const int64_t *adj;
    const float *len;
    int64_t ldl;
    const int64_t *col;
    float wc, wl, wa;
    double *losses, *terms;
    int32_t *err;
    const int *start;                                       // workspace
    double *partial;                                        // [K][n_maps][kLossMaxBlocks][3]
};

// grid = (upper bound of blocks over all layouts, maps); partial[((k * n_maps + m) * kLossMaxBlocks + block of the layout) * 3 + {0,1,2}]
__global__ __launch_bounds__(kMnThreads) void loss_many_partial_kernel(ManyDesc d, LossManyArgs a) {
    int k, bl;
    if (!many_find(a.start, d.K, blockIdx.x, k, bl)) return;
    const int nb = a.start[k + 1] - a.start[k], m = blockIdx.y;
    LossManyView v;
    bool bad;
    if (!loss_many_view(d, k, v, bad) || bl >= kLossMaxBlocks) return;      // (the plan gives such a layout no block)
    const float *p = a.probs[k];
    if (!p) {                                               // (uniform over the block)
        if (threadIdx.x == 0) a.err[k] = 1;
        return;
    }
    double s_area = 0.0, s_feas = 0.0, s_align = 0.0;
    loss_accumulate(v.n, v.ec, v.ea, p + m, a.ldp, a.area + v.np * a.lda, a.lda, a.col + 2 * v.cp, a.adj + 2 * v.ap, a.len + v.ap * a.ldl,
                    a.ldl, (int64_t)bl * kMnThreads + threadIdx.x, (int64_t)nb * kMnThreads, s_area, s_feas, s_align, bad);
    if (bad) a.err[k] = 1;
    loss_block_reduce(s_area, s_feas, s_align, a.partial + (((int64_t)k * a.n_maps + m) * kLossMaxBlocks + bl) * 3);
}

// one wavefront per (layout, map): loss_final_kernel on the layout's partial rows
__global__ __launch_bounds__(64) void loss_many_final_kernel(ManyDesc d, LossManyArgs a) {
    const int k = blockIdx.x, m = blockIdx.y, lane = threadIdx.x;
    LossManyView v;
    bool bad;
    const bool live = loss_many_view(d, k, v, bad);
    if (!live && !bad) return;                              // inactive or without nodes: the caller's rows stay
    const int64_t row = (int64_t)k * a.n_maps + m;
    if (bad || a.err[k]) {                                  // NaN = "offset, count or edge index out of range"
        const double nan = loss_nan();
        if (lane == 0) {
            if (bad) a.err[k] = 1;
            a.losses[row] = nan;
            if (a.terms) { a.terms[row * 3] = nan; a.terms[row * 3 + 1] = nan; a.terms[row * 3 + 2] = nan; }
        }
        return;
    }
    double s[3];
    loss_fold_rows(a.partial + row * kLossMaxBlocks * 3, a.start[k + 1] - a.start[k], s);
    if (lane == 0) {
        double t[3];
        a.losses[row] = loss_from_sums(s, v.n, v.ec, v.ea, a.wc, a.wl, a.wa, t);
        if (a.terms) { a.terms[row * 3] = t[0]; a.terms[row * 3 + 1] = t[1]; a.terms[row * 3 + 2] = t[2]; }
    }
}

static int many_blocks_ub(int64_t total, int64_t k) { return (int)(total / kChunk + k); }

}  // namespace tgnn

using namespace tgnn;

#define TGNN_MANY_CHECK_K(K) TGNN_CHECK_ARG((K) >= 0 && (K) <= (1 << 20), "number of layouts")

static bool many_totals_ok(int64_t a, int64_t b, int64_t c) {
    const int64_t lim = (1ll << 31) - 1;
    return a >= 0 && b >= 0 && c >= 0 && a < lim && b < lim && c < lim;
}

extern "C" size_t tgnn_sublayout_compact_many_workspace_bytes(int32_t n_layouts, int64_t total_nodes, int64_t total_adj_edges,
                                                              int64_t total_col_edges) {
    if (n_layouts < 0 || !many_totals_ok(total_nodes, total_adj_edges, total_col_edges)) return 0;
    const size_t k = (size_t)n_layouts;
    const size_t blocks = (size_t)many_blocks_ub(total_nodes, k) + many_blocks_ub(total_adj_edges, k) + many_blocks_ub(total_col_edges, k);
    return align_up(3 * (k + 1) * sizeof(int), 256) + align_up((blocks + 1) * sizeof(int), 256) +
           align_up(((size_t)total_nodes + 1) * sizeof(int), 256) + 256;
}

extern "C" int tgnn_sublayout_compact_many(int32_t n_layouts, const int32_t *active, const int64_t *node_ptr, const int64_t *adj_ptr,
                                           const int64_t *col_ptr, int64_t total_nodes, int64_t total_adj_edges,
                                           int64_t total_col_edges, const int32_t *alive, const float *x, int32_t fx,
                                           const int64_t *adj_edge_index, const float *adj_edge_attr, int32_t fe,
                                           const int64_t *col_edge_index, float *x_out, int64_t *inverse_out, int64_t *adj_out,
                                           float *adj_attr_out, int64_t *col_out, int64_t *counts_out, int32_t *err_flag, void *ws,
                                           size_t ws_bytes, tgnn_stream_t stream) {
    DeviceGuard guard__(stream);
    TGNN_MANY_CHECK_K(n_layouts);
    TGNN_CHECK_ARG(many_totals_ok(total_nodes, total_adj_edges, total_col_edges) && fx >= 1, "totals must fit int32");
    if (n_layouts == 0) return TGNN_OK;
    TGNN_CHECK_ARG(node_ptr && adj_ptr && col_ptr, "null offset table");
    TGNN_CHECK_ARG(counts_out && err_flag, "null pointer");
    TGNN_CHECK_ARG(total_nodes == 0 || (alive && x && x_out && inverse_out), "node arrays");
    TGNN_CHECK_ARG(total_adj_edges == 0 || (adj_edge_index && adj_out && adj_edge_attr && adj_attr_out && fe >= 1), "adjacency arrays");
    TGNN_CHECK_ARG(total_col_edges == 0 || (col_edge_index && col_out), "collision arrays");
    if (!ws || ws_bytes < tgnn_sublayout_compact_many_workspace_bytes(n_layouts, total_nodes, total_adj_edges, total_col_edges)) {
        set_error("tgnn_sublayout_compact_many: workspace too small");
        return TGNN_ERR_WORKSPACE;
    }
    hipStream_t s = static_cast<hipStream_t>(stream);
    const int K = n_layouts;
    ManyDesc d{K, {node_ptr, adj_ptr, col_ptr}, {total_nodes, total_adj_edges, total_col_edges}, active, nullptr};
    CompactArgs a{};
    a.alive = alive; a.x = x; a.fx = fx; a.ei[0] = adj_edge_index; a.ei[1] = col_edge_index; a.attr = adj_edge_attr; a.fe = fe;
    a.x_out = x_out; a.inverse_out = inverse_out; a.ei_out[0] = adj_out; a.ei_out[1] = col_out; a.attr_out = adj_attr_out;
    a.counts_out = counts_out; a.err = err_flag;
    a.ub[0] = many_blocks_ub(total_nodes, K); a.ub[1] = many_blocks_ub(total_adj_edges, K); a.ub[2] = many_blocks_ub(total_col_edges, K);
    Carver cv(ws, ws_bytes);
    a.start = cv.take<int>(3 * (size_t)(K + 1));
    a.cnt = cv.take<int>((size_t)a.ub[0] + a.ub[1] + a.ub[2] + 1);
    a.npos = cv.take<int>((size_t)total_nodes + 1);
    many_plan_kernel<<<1, kMnThreads, 0, s>>>(d, 3, 0, a.start, err_flag);
    compact_count_kernel<<<a.ub[0] + a.ub[1] + a.ub[2], kMnThreads, 0, s>>>(d, a);
    compact_scan_kernel<<<dim3(K, 3), kMnThreads, 0, s>>>(d, a);
    compact_scatter_kernel<<<a.ub[0], kMnThreads, 0, s>>>(d, a, 0);
    compact_scatter_kernel<<<a.ub[1] + a.ub[2], kMnThreads, 0, s>>>(d, a, 1);
    TGNN_CHECK_LAUNCH();
    return TGNN_OK;
}

extern "C" size_t tgnn_greedy_round_many_workspace_bytes(int32_t n_layouts, int64_t total_nodes) {
    if (n_layouts < 0 || total_nodes < 0) return 0;
    return align_up(3 * ((size_t)n_layouts + 1) * sizeof(int), 256) + align_up(((size_t)total_nodes + 1) * sizeof(double), 256) +
           align_up(((size_t)total_nodes + 1) * sizeof(int), 256) + 256;
}

extern "C" int tgnn_greedy_round_many(int32_t n_layouts, const int32_t *active, const float *const *prob, int64_t ld_prob,
                                      const int64_t *node_ptr, const int64_t *col_ptr, int64_t total_nodes, int64_t total_col_edges,
                                      const int64_t *counts, const int64_t *inverse, const int64_t *col_edge_index, int32_t round,
                                      const uint64_t *seeds, double *prob_saved, int32_t *alive, int32_t *selected_round,
                                      int64_t *n_selected, int32_t *err_flag, void *ws, size_t ws_bytes, tgnn_stream_t stream) {
    DeviceGuard guard__(stream);
    TGNN_MANY_CHECK_K(n_layouts);
    TGNN_CHECK_ARG(many_totals_ok(total_nodes, 0, total_col_edges) && round >= 1 && ld_prob >= 1, "shape");
    if (n_layouts == 0 || total_nodes == 0) return TGNN_OK;
    TGNN_CHECK_ARG(node_ptr && col_ptr && counts, "null offset table");
    TGNN_CHECK_ARG(prob && inverse && seeds && prob_saved && alive && selected_round && n_selected && err_flag, "null pointer");
    TGNN_CHECK_ARG(total_col_edges == 0 || col_edge_index, "null edge index");
    if (!ws || ws_bytes < tgnn_greedy_round_many_workspace_bytes(n_layouts, total_nodes)) {
        set_error("tgnn_greedy_round_many: workspace too small");
        return TGNN_ERR_WORKSPACE;
    }
    hipStream_t s = static_cast<hipStream_t>(stream);
    const int K = n_layouts;
    ManyDesc d{K, {node_ptr, nullptr, col_ptr}, {total_nodes, 0, total_col_edges}, active, counts};   // (no adjacency set here)
    RoundArgs a{};
    a.prob = prob; a.ldp = ld_prob; a.inverse = inverse; a.col = col_edge_index; a.round = round;
    a.seeds = reinterpret_cast<const unsigned long long *>(seeds); a.saved = prob_saved; a.alive = alive; a.selected = selected_round;
    a.n_selected = reinterpret_cast<long long *>(n_selected); a.err = err_flag;
    Carver cv(ws, ws_bytes);
    a.start = cv.take<int>(3 * (size_t)(K + 1));
    a.p = cv.take<double>((size_t)total_nodes + 1);
    a.flags = cv.take<int>((size_t)total_nodes + 1);
    const int nb = many_blocks_ub(total_nodes, K), eb = many_blocks_ub(total_col_edges, K);
    many_plan_kernel<<<1, kMnThreads, 0, s>>>(d, 3, 0, a.start, err_flag);
    round_step_kernel<<<nb, kMnThreads, 0, s>>>(d, a, 0);
    if (total_col_edges > 0) round_step_kernel<<<eb, kMnThreads, 0, s>>>(d, a, 1);
    round_step_kernel<<<nb, kMnThreads, 0, s>>>(d, a, 2);
    if (total_col_edges > 0) round_step_kernel<<<eb, kMnThreads, 0, s>>>(d, a, 3);
    TGNN_CHECK_LAUNCH();
    return TGNN_OK;
}

extern "C" int tgnn_greedy_finish_many(int32_t n_layouts, const int32_t *finish, const int64_t *node_ptr, const int64_t *col_ptr,
                                       int64_t total_nodes, int64_t total_col_edges, const int64_t *counts, const int64_t *inverse,
                                       const int64_t *col_edge_index, int32_t first_round, int32_t max_rounds, const uint64_t *seeds,
                                       double *prob_saved, int32_t *alive, int32_t *selected_round, int64_t *n_selected,
                                       int32_t *err_flag, int32_t *out, tgnn_stream_t stream) {
    DeviceGuard guard__(stream);
    TGNN_MANY_CHECK_K(n_layouts);
    TGNN_CHECK_ARG(many_totals_ok(total_nodes, 0, total_col_edges) && first_round >= 1 && max_rounds >= 1, "shape");
    if (n_layouts == 0) return TGNN_OK;
    TGNN_CHECK_ARG(finish && node_ptr && col_ptr && counts, "null offset table");
    TGNN_CHECK_ARG(inverse && seeds && prob_saved && alive && selected_round && n_selected && err_flag && out, "null pointer");
    TGNN_CHECK_ARG(total_col_edges == 0 || col_edge_index, "null edge index");
    ManyDesc d{n_layouts, {node_ptr, nullptr, col_ptr}, {total_nodes, 0, total_col_edges}, finish, counts};
    finish_many_kernel<<<n_layouts, kFinThreads, 0, static_cast<hipStream_t>(stream)>>>(
        d, finish, inverse, col_edge_index, first_round, max_rounds, reinterpret_cast<const unsigned long long *>(seeds), prob_saved,
        alive, selected_round, reinterpret_cast<long long *>(n_selected), err_flag, out);
    TGNN_CHECK_LAUNCH();
    return TGNN_OK;
}

extern "C" size_t tgnn_solution_score_sums_many_workspace_bytes(int32_t n_layouts) {
    const size_t k = n_layouts > 0 ? (size_t)n_layouts : 1;
    return align_up((k + 1) * sizeof(int), 256) + align_up(k * kLossMaxBlocks * 3 * sizeof(double), 256) +
           align_up(k * sizeof(int), 256) + 256;
}

extern "C" int tgnn_solution_score_sums_many(int32_t n_layouts, const int32_t *active, const int64_t *node_ptr, const int64_t *adj_ptr,
                                             int64_t total_nodes, int64_t total_adj_edges, const float *predict,
                                             const float *area_ratio, int64_t ld_area, const float *perimeter,
                                             const int64_t *adj_edge_index, const float *adj_edge_len, int64_t ld_len, double *sums,
                                             void *ws, size_t ws_bytes, tgnn_stream_t stream) {
    DeviceGuard guard__(stream);
    TGNN_MANY_CHECK_K(n_layouts);
    TGNN_CHECK_ARG(many_totals_ok(total_nodes, total_adj_edges, 0) && ld_area >= 1, "shape");
    if (n_layouts == 0) return TGNN_OK;
    TGNN_CHECK_ARG(node_ptr && adj_ptr, "null offset table");
    TGNN_CHECK_ARG(sums && (total_nodes == 0 || (predict && area_ratio && perimeter)), "null pointer");
    TGNN_CHECK_ARG(total_adj_edges == 0 || (adj_edge_index && adj_edge_len && ld_len >= 1), "adjacency edges");
    if (!ws || ws_bytes < tgnn_solution_score_sums_many_workspace_bytes(n_layouts)) {
        set_error("tgnn_solution_score_sums_many: workspace too small");
        return TGNN_ERR_WORKSPACE;
    }
    hipStream_t s = static_cast<hipStream_t>(stream);
    const int K = n_layouts;
    Carver cv(ws, ws_bytes);
    int *start = cv.take<int>((size_t)K + 1);
    double *partial = cv.take<double>((size_t)K * kLossMaxBlocks * 3);
    int *err = cv.take<int>((size_t)K);
    TGNN_CHECK_HIP(hipMemsetAsync(err, 0, (size_t)K * sizeof(int), s));
    ManyDesc d{K, {node_ptr, adj_ptr, nullptr}, {total_nodes, total_adj_edges, 0}, active, nullptr};
    many_plan_kernel<<<1, kMnThreads, 0, s>>>(d, 1, 1, start, err);
    // blocks of layout k: loss_blocks(n, 0, ea) <= (n + ea) / kChunk + 1
    const int ub = many_blocks_ub(total_nodes + total_adj_edges, K);
    score_many_partial_kernel<<<ub, kMnThreads, 0, s>>>(d, start, predict, area_ratio, ld_area, perimeter, adj_edge_index, adj_edge_len,
                                                        ld_len, partial, err);
    score_many_final_kernel<<<K, 64, 0, s>>>(K, active, start, partial, err, sums);
    TGNN_CHECK_LAUNCH();
    return TGNN_OK;
}

extern "C" size_t tgnn_unsupervised_loss_many_workspace_bytes(int32_t n_layouts, int32_t n_maps) {
    const size_t k = n_layouts > 0 ? (size_t)n_layouts : 1, m = n_maps > 0 ? (size_t)n_maps : 1;
    return align_up((k + 1) * sizeof(int), 256) + align_up(k * m * kLossMaxBlocks * 3 * sizeof(double), 256) + 256;
}

extern "C" int tgnn_unsupervised_loss_many(int32_t n_layouts, const int32_t *active, const int64_t *node_ptr, const int64_t *adj_ptr,
                                           const int64_t *col_ptr, int64_t total_nodes, int64_t total_adj_edges,
                                           int64_t total_col_edges, const int64_t *counts, const float *const *probs,
                                           int64_t ld_probs, int32_t n_maps, const float *area_ratio, int64_t ld_area,
                                           const int64_t *adj_edge_index, const float *adj_edge_len, int64_t ld_len,
                                           const int64_t *col_edge_index, float collision_weight, float align_length_weight,
                                           float avg_area_weight, double *losses, double *terms, int32_t *err, void *ws,
                                           size_t ws_bytes, tgnn_stream_t stream) {
    DeviceGuard guard__(stream);
    TGNN_MANY_CHECK_K(n_layouts);
    TGNN_CHECK_ARG(many_totals_ok(total_nodes, total_adj_edges, total_col_edges), "totals must fit int32");
    TGNN_CHECK_ARG(n_maps >= 1 && n_maps <= 65535 && ld_probs >= n_maps && ld_area >= 1, "maps / strides");
    if (n_layouts == 0) return TGNN_OK;
    TGNN_CHECK_ARG(node_ptr && adj_ptr && col_ptr, "null offset table");
    TGNN_CHECK_ARG(probs && losses && err && (total_nodes == 0 || area_ratio), "null pointer");
    TGNN_CHECK_ARG(total_adj_edges == 0 || (adj_edge_index && adj_edge_len && ld_len >= 1), "adjacency edges");
    TGNN_CHECK_ARG(total_col_edges == 0 || col_edge_index, "collision edges");
    if (!ws || ws_bytes < tgnn_unsupervised_loss_many_workspace_bytes(n_layouts, n_maps)) {
        set_error("tgnn_unsupervised_loss_many: workspace too small");
        return TGNN_ERR_WORKSPACE;
    }
    hipStream_t s = static_cast<hipStream_t>(stream);
    const int K = n_layouts;
    Carver cv(ws, ws_bytes);
    int *start = cv.take<int>((size_t)K + 1);
    double *partial = cv.take<double>((size_t)K * n_maps * kLossMaxBlocks * 3);
    TGNN_CHECK_HIP(hipMemsetAsync(err, 0, (size_t)K * sizeof(int32_t), s));
    ManyDesc d{K, {node_ptr, adj_ptr, col_ptr}, {total_nodes, total_adj_edges, total_col_edges}, active, counts};
    LossManyArgs a{probs, ld_probs, n_maps, area_ratio, ld_area, adj_edge_index, adj_edge_len, ld_len, col_edge_index,
                   collision_weight, align_length_weight, avg_area_weight, losses, terms, err, start, partial};
    many_plan_kernel<<<1, kMnThreads, 0, s>>>(d, 1, 2, start, err);
    // blocks of layout k: loss_blocks(n, ec, ea) <= (n + ec + ea) / kChunk + 1
    const int ub = many_blocks_ub(total_nodes + total_adj_edges + total_col_edges, K);
    loss_many_partial_kernel<<<dim3(ub, n_maps), kMnThreads, 0, s>>>(d, a);
    loss_many_final_kernel<<<dim3(K, n_maps), 64, 0, s>>>(d, a);
    TGNN_CHECK_LAUNCH();
    return TGNN_OK;
}
