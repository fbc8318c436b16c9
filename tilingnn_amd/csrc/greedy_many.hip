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
// EQUALITY.  Per layout every entry computes exactly what its single-layout counterpart computes: compaction keeps ascending
// order (block scans, chunk bases from a per-layout scan), the acceptance uses the same expressions (pow / exp in fp64, the
// same counter-based draw keyed by (seed_k, round, local original node)), the score sums run over the same fixed tree (same
// number of blocks per layout, same strides, same reduction).  The only atomics add integers (n_selected) or store one value.
// Every offset and index read from the device is range-checked: a bad one sets the layout's error word and is skipped.
#include "tgnn_common.h"

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
__host__ __device__ __forceinline__ int64_t many_full_size(const ManyDesc &d, int s, int k, bool &bad) {
    const int64_t a = d.ptr[s][k], b = d.ptr[s][k + 1];
    if (a < 0 || b < a || b > d.total[s] || b - a >= (1ll << 31) - 1) { bad = true; return 0; }
    return b - a;
}
// the size this call works on: 0 for an inactive layout; the sub-layout count (checked against the full size) when counts are given
__host__ __device__ __forceinline__ int64_t many_size(const ManyDesc &d, int s, int k, bool &bad) {
    if (d.active && d.active[k] == 0) return 0;
    const int64_t full = many_full_size(d, s, k, bad);
    if (!d.counts) return full;
    const int64_t c = d.counts[(int64_t)k * 3 + s];
    if (c < 0 || c > full) { bad = true; return 0; }
    return c;
}

// ---- the unsupervised loss of K layouts (loss.hip per layout): what a layout contributes, where its arrays start.  Host and
// device: scratch/loss_many_host_check.cpp walks these on random offset tables under AddressSanitizer.
struct LossManyView {
    int64_t n, ec, ea;                                      // sizes this call works on (the sub-layout's with counts)
    int64_t np, ap, cp;                                     // first node / adjacency edge / collision edge in the packed arrays
};
// false: nothing to compute -- inactive or without nodes (bad stays false), or an offset / count out of range (bad = true).
// Every offset is checked against the packed sizes before it is returned.
__host__ __device__ __forceinline__ bool loss_many_view(const ManyDesc &d, int k, LossManyView &v, bool &bad) {
    bad = false;
    v.n = many_size(d, 0, k, bad);
    v.ea = many_size(d, 1, k, bad);
    v.ec = many_size(d, 2, k, bad);
    if (bad || v.n == 0) return false;
    v.np = d.ptr[0][k]; v.ap = d.ptr[1][k]; v.cp = d.ptr[2][k];
    return true;
}
// loss.hip: loss_blocks(n, ec, ea)
__host__ __device__ __forceinline__ int loss_many_blocks(int64_t n, int64_t ec, int64_t ea) {
    int64_t work = n > ec ? n : ec;
    if (ea > work) work = ea;
    int64_t b = (work + kChunk - 1) / kChunk;
    return (int)(b < 1 ? 1 : (b > 512 ? 512 : b));
}

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
// items; mode 1 (set 0 only): the block count of the score sums, loss.hip: loss_blocks(n, 0, ea); mode 2 (set 0 only): the block
// count of the unsupervised loss, loss_blocks(n, ec, ea) over the sizes this call works on (0 for a layout without nodes).
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
                    blocks = loss_many_view(d, k, v, bad) ? loss_many_blocks(v.n, v.ec, v.ea) : 0;
                } else if (!(d.active && d.active[k] == 0)) {
                    const int64_t n = many_full_size(d, 0, k, bad), ea = many_full_size(d, 1, k, bad);
                    int64_t b = ((n > ea ? n : ea) + kChunk - 1) / kChunk;
                    blocks = bad ? 0 : (int)(b < 1 ? 1 : (b > 512 ? 512 : b));
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
// splitmix64 of (seed, round, node) -> uniform double in [0, 1): greedy.hip's greedy_uniform
__device__ __forceinline__ double many_uniform(unsigned long long seed, unsigned round, unsigned long long node) {
    unsigned long long z = seed + 0x9E3779B97F4A7C15ull * (node + 1ull) + 0xD1B54A32D192ED03ull * (unsigned long long)(round + 1u);
    z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull;
    z = (z ^ (z >> 27)) * 0x94D049BB133111EBull;
    z ^= z >> 31;
    return (double)(z >> 11) * (1.0 / 9007199254740992.0);
}

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
                if (step == 0) { p[i] = 0.0; flags[i] = 1; }
                continue;
            }
            if (step == 0) {
                const double pr = prob ? (double)prob[i * a.ldp] : (double)1.0f;
                const double v = pow(pow(a.saved[np + o], (double)(a.round - 1)) * pr, 1.0 / (double)a.round);
                a.saved[np + o] = v;
                p[i] = v;
                flags[i] = 0;                                 // bit 0: beaten by a neighbour, bit 1: accepted
            } else {
                if (flags[i] & 1) continue;
                if (exp((p[i] - 1.0) * 1.0) > many_uniform(seed, (unsigned)a.round, (unsigned long long)o)) {
                    flags[i] = 2;
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
            const double pu = p[u], pv = p[v];
            if (pv > pu || (pv == pu && v < u)) flags[u] = 1;  // (every writer stores the same word)
            else flags[v] = 1;
        } else if (flags[u] & 2) {
            const int64_t o = inverse[v];
            if (o >= 0 && o < n_k) a.alive[np + o] = 0;
        }
    }
}

// greedy.hip's greedy_finish_kernel, one block per layout whose finish word is set
constexpr int kFinThreads = 1024;
constexpr int kFinMaxNodes = 4096;                          // == tgnn_greedy_finish_max_nodes()
__global__ __launch_bounds__(kFinThreads) void finish_many_kernel(ManyDesc d, const int32_t *__restrict__ finish,
                                                                  const int64_t *__restrict__ inverse_all,
                                                                  const int64_t *__restrict__ col_all, int first_round, int max_rounds,
                                                                  const unsigned long long *__restrict__ seeds,
                                                                  double *__restrict__ saved_all, int *__restrict__ alive_all,
                                                                  int *__restrict__ selected_all, long long *__restrict__ count_all,
                                                                  int *__restrict__ err_all, int *__restrict__ out_all) {
    __shared__ double p[kFinMaxNodes];
    __shared__ __attribute__((aligned(16))) unsigned char flags[kFinMaxNodes];   // bit 0 beaten, bit 1 accepted, bit 2 gone, bit 3 leaving
    __shared__ int left, accepted, bad_inverse;
    const int k = blockIdx.x, tid = threadIdx.x;
    if (finish[k] == 0) return;
    int *out = out_all + 2 * k, *err = err_all + k;
    bool bad = false;
    const int64_t n64 = many_size(d, 0, k, bad), n_k = many_full_size(d, 0, k, bad), ec = many_size(d, 2, k, bad);
    if (bad || n64 > kFinMaxNodes) {                          // (uniform over the block)
        if (tid == 0) { *err = 1; out[0] = 0; out[1] = (int)(n64 > 0x7fffffff ? 0x7fffffff : n64); }
        return;
    }
    const int n_sub = (int)n64;
    const int64_t np = d.ptr[0][k];
    const int64_t *inverse = inverse_all + np, *col = col_all + 2 * d.ptr[2][k];
    double *saved = saved_all + np;
    int *alive = alive_all + np, *selected = selected_all + np;
    long long *count = count_all + k;
    const unsigned long long seed = seeds[k];
    if (tid == 0) bad_inverse = 0;
    __syncthreads();
    for (int i = tid; i < n_sub; i += kFinThreads) {
        const int64_t o = inverse[i];
        if (o < 0 || o >= n_k) { bad_inverse = 1; flags[i] = 4; continue; }
        flags[i] = alive[o] ? 0 : 4;
    }
    __syncthreads();
    if (bad_inverse && tid == 0) *err = 1;
    int round = first_round, rounds_run = 0;
    for (;; ++round) {
        if (tid == 0) { left = 0; accepted = 0; }
        __syncthreads();
        int mine = 0;
        for (int i = tid; i < n_sub; i += kFinThreads) {
            if (flags[i] & 4) continue;
            ++mine;
            const int64_t o = inverse[i];
            const double v = pow(pow(saved[o], (double)(round - 1)) * 1.0, 1.0 / (double)round);     // (greedy_mean_kernel, prob = 1)
            saved[o] = v;
            p[i] = v;
            flags[i] = 0;
        }
        if (mine) atomicAdd(&left, mine);
        __syncthreads();
        if (left == 0 || rounds_run >= max_rounds) break;    // (uniform)
        ++rounds_run;
        for (int64_t e = tid; e < ec; e += kFinThreads) {      // greedy_beaten_kernel
            const int64_t u = col[e], v = col[ec + e];
            if (u < 0 || u >= n_sub || v < 0 || v >= n_sub) { *err = 1; continue; }
            if (u == v || ((flags[u] | flags[v]) & 4)) continue;
            const double pu = p[u], pv = p[v];
            if (pv > pu || (pv == pu && v < u)) atomicOr(reinterpret_cast<unsigned *>(flags) + (u >> 2), 1u << (8 * (u & 3)));
            else atomicOr(reinterpret_cast<unsigned *>(flags) + (v >> 2), 1u << (8 * (v & 3)));
        }
        __syncthreads();
        int acc = 0;
        for (int i = tid; i < n_sub; i += kFinThreads) {       // greedy_accept_kernel
            if (flags[i] & 5) continue;
            const int64_t o = inverse[i];
            if (exp((p[i] - 1.0) * 1.0) > many_uniform(seed, (unsigned)round, (unsigned long long)o)) {
                flags[i] |= 2;
                alive[o] = 0;
                selected[o] = round;
                ++acc;
            }
        }
        if (acc) atomicAdd(&accepted, acc);
        __syncthreads();
        for (int64_t e = tid; e < ec; e += kFinThreads) {      // greedy_label_kernel
            const int64_t u = col[e], v = col[ec + e];
            if (u < 0 || u >= n_sub || v < 0 || v >= n_sub) continue;
            if ((flags[u] & 2) && !(flags[v] & 4)) {
                alive[inverse[v]] = 0;
                atomicOr(reinterpret_cast<unsigned *>(flags) + (v >> 2), 8u << (8 * (v & 3)));   // bit 3: leaves behind this round
            }
        }
        __syncthreads();
        for (int i = tid; i < n_sub; i += kFinThreads)
            if (flags[i] & (2 | 8)) flags[i] = 4;
        if (tid == 0 && accepted) atomicAdd(reinterpret_cast<unsigned long long *>(count), (unsigned long long)accepted);
        __syncthreads();
    }
    if (tid == 0) {
        out[0] = rounds_run;
        out[1] = left;
    }
}

// ------------------------------------------------------------------------------------------ score sums (loss.hip, per layout)
constexpr int kScoreMaxBlocks = 512;
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
    const float *predict = predict_all + np, *area = area_all + np * lda, *perim = perim_all + np;
    const int64_t *adj = adj_all + 2 * ap;
    const float *len = len_all + ap * ldl;
    double s0 = 0.0, s1 = 0.0, s2 = 0.0;
    const int64_t stride = (int64_t)nb * kMnThreads, t0 = (int64_t)bl * kMnThreads + threadIdx.x;
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
    if (bad) err[k] = 1;
    __shared__ double red[3][kMnThreads];
    red[0][threadIdx.x] = s0; red[1][threadIdx.x] = s1; red[2][threadIdx.x] = s2;
    __syncthreads();
    for (int s = kMnThreads / 2; s >= 1; s >>= 1) {
        if ((int)threadIdx.x < s)
            for (int c = 0; c < 3; ++c) red[c][threadIdx.x] += red[c][threadIdx.x + s];
        __syncthreads();
    }
    if (threadIdx.x < 3) partial_all[((int64_t)k * kScoreMaxBlocks + bl) * 3 + threadIdx.x] = red[threadIdx.x][0];
}

__global__ __launch_bounds__(64) void score_many_final_kernel(int K, const int32_t *__restrict__ active, const int *__restrict__ start,
                                                              const double *__restrict__ partial_all, const int *__restrict__ err,
                                                              double *__restrict__ sums) {
    const int k = blockIdx.x, lane = threadIdx.x;
    if (active && active[k] == 0) return;
    const int n_blocks = start[k + 1] - start[k];
    const double *partial = partial_all + (int64_t)k * kScoreMaxBlocks * 3;
    double s[3] = {0.0, 0.0, 0.0};
    for (int b = lane; b < n_blocks; b += 64)
#pragma unroll
        for (int c = 0; c < 3; ++c) s[c] += partial[(int64_t)b * 3 + c];
#pragma unroll
    for (int c = 0; c < 3; ++c)
#pragma unroll
        for (int t = 32; t >= 1; t >>= 1) s[c] += __shfl_xor(s[c], t, 64);
    if (lane < 3) sums[(int64_t)k * 3 + lane] = err[k] ? __longlong_as_double(0x7ff8000000000000ll) : s[lane];
}

// ------------------------------------------------------------------------------------------ unsupervised loss (loss.hip, per layout)
constexpr float kLossManyEps = 1e-7f;                       // loss.hip: kLossEps
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
    double *partial;                                        // [K][n_maps][512][3]
};

// what thread t0 of a grid of `stride` threads adds up: loss_partial_kernel's three loops on one layout's arrays (p: the map's
// column, area / col / adj / len: the layout's own blocks).  An edge end outside [0, n) is skipped and reported.
__host__ __device__ __forceinline__ void loss_many_accumulate(const LossManyView &v, const float *p, int64_t ldp, const float *area,
                                                              int64_t lda, const int64_t *col, const int64_t *adj, const float *len,
                                                              int64_t ldl, int64_t t0, int64_t stride, double &s_area, double &s_feas,
                                                              double &s_align, bool &bad) {
    const int64_t n = v.n, ec = v.ec, ea = v.ea;
    for (int64_t i = t0; i < n; i += stride) s_area += (double)(area[i * lda] * p[i * ldp]);
    for (int64_t e = t0; e < ec; e += stride) {
        const int64_t i = col[e], j = col[ec + e];
        if (i < 0 || i >= n || j < 0 || j >= n) { bad = true; continue; }
        float pp = p[i * ldp] * p[j * ldp];
        pp = fminf(fmaxf(pp, kLossManyEps), 1.0f - kLossManyEps);
        s_feas += (double)logf(1.0f - pp);
    }
    for (int64_t e = t0; e < ea; e += stride) {
        const int64_t i = adj[e], j = adj[ea + e];
        if (i < 0 || i >= n || j < 0 || j >= n) { bad = true; continue; }
        float pp = p[i * ldp] * p[j * ldp] * len[e * ldl];
        pp = fmaxf(pp, kLossManyEps);
        s_align += (double)(logf(pp) / 2.302585092994046f);
    }
}

// grid = (upper bound of blocks over all layouts, maps); partial[((k * n_maps + m) * 512 + block of the layout) * 3 + {0,1,2}]
__global__ __launch_bounds__(kMnThreads) void loss_many_partial_kernel(ManyDesc d, LossManyArgs a) {
    int k, bl;
    if (!many_find(a.start, d.K, blockIdx.x, k, bl)) return;
    const int nb = a.start[k + 1] - a.start[k], m = blockIdx.y;
    LossManyView v;
    bool bad;
    if (!loss_many_view(d, k, v, bad) || bl >= kScoreMaxBlocks) return;      // (the plan gives such a layout no block)
    const float *p = a.probs[k];
    if (!p) {                                               // (uniform over the block)
        if (threadIdx.x == 0) a.err[k] = 1;
        return;
    }
    double s_area = 0.0, s_feas = 0.0, s_align = 0.0;
    loss_many_accumulate(v, p + m, a.ldp, a.area + v.np * a.lda, a.lda, a.col + 2 * v.cp, a.adj + 2 * v.ap, a.len + v.ap * a.ldl, a.ldl,
                         (int64_t)bl * kMnThreads + threadIdx.x, (int64_t)nb * kMnThreads, s_area, s_feas, s_align, bad);
    if (bad) a.err[k] = 1;
    __shared__ double red[3][kMnThreads];
    red[0][threadIdx.x] = s_area; red[1][threadIdx.x] = s_feas; red[2][threadIdx.x] = s_align;
    __syncthreads();
    for (int s = kMnThreads / 2; s >= 1; s >>= 1) {
        if ((int)threadIdx.x < s)
            for (int c = 0; c < 3; ++c) red[c][threadIdx.x] += red[c][threadIdx.x + s];
        __syncthreads();
    }
    if (threadIdx.x < 3)
        a.partial[(((int64_t)k * a.n_maps + m) * kScoreMaxBlocks + bl) * 3 + threadIdx.x] = red[threadIdx.x][0];
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
        const double nan = __longlong_as_double(0x7ff8000000000000ll);
        if (lane == 0) {
            if (bad) a.err[k] = 1;
            a.losses[row] = nan;
            if (a.terms) { a.terms[row * 3] = nan; a.terms[row * 3 + 1] = nan; a.terms[row * 3 + 2] = nan; }
        }
        return;
    }
    const int n_blocks = a.start[k + 1] - a.start[k];
    const double *partial = a.partial + row * kScoreMaxBlocks * 3;
    double s[3] = {0.0, 0.0, 0.0};
    for (int b = lane; b < n_blocks; b += 64)
#pragma unroll
        for (int c = 0; c < 3; ++c) s[c] += partial[(int64_t)b * 3 + c];
#pragma unroll
    for (int c = 0; c < 3; ++c)
#pragma unroll
        for (int t = 32; t >= 1; t >>= 1) s[c] += __shfl_xor(s[c], t, 64);
    if (lane == 0) {
        const double t0 = log(fmax(s[0] / (double)v.n, (double)kLossManyEps));
        const double t1 = v.ec > 0 ? s[1] / (double)v.ec : 0.0;
        const double t2 = v.ea > 0 ? s[2] / (double)v.ea : 0.0;
        if (a.terms) { a.terms[row * 3] = t0; a.terms[row * 3 + 1] = t1; a.terms[row * 3 + 2] = t2; }
        a.losses[row] = (1.0 - (double)a.wa * t0) * (1.0 - (double)a.wc * t1) * (1.0 - (double)a.wl * t2);
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
    return align_up((k + 1) * sizeof(int), 256) + align_up(k * kScoreMaxBlocks * 3 * sizeof(double), 256) +
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
    double *partial = cv.take<double>((size_t)K * kScoreMaxBlocks * 3);
    int *err = cv.take<int>((size_t)K);
    TGNN_CHECK_HIP(hipMemsetAsync(err, 0, (size_t)K * sizeof(int), s));
    ManyDesc d{K, {node_ptr, adj_ptr, nullptr}, {total_nodes, total_adj_edges, 0}, active, nullptr};
    many_plan_kernel<<<1, kMnThreads, 0, s>>>(d, 1, 1, start, err);
    // blocks of layout k: clamp(ceil(max(n, ea) / kChunk), 1, 512) <= (n + ea) / kChunk + 1
    const int ub = many_blocks_ub(total_nodes + total_adj_edges, K);
    score_many_partial_kernel<<<ub, kMnThreads, 0, s>>>(d, start, predict, area_ratio, ld_area, perimeter, adj_edge_index, adj_edge_len,
                                                        ld_len, partial, err);
    score_many_final_kernel<<<K, 64, 0, s>>>(K, active, start, partial, err, sums);
    TGNN_CHECK_LAUNCH();
    return TGNN_OK;
}

extern "C" size_t tgnn_unsupervised_loss_many_workspace_bytes(int32_t n_layouts, int32_t n_maps) {
    const size_t k = n_layouts > 0 ? (size_t)n_layouts : 1, m = n_maps > 0 ? (size_t)n_maps : 1;
    return align_up((k + 1) * sizeof(int), 256) + align_up(k * m * kScoreMaxBlocks * 3 * sizeof(double), 256) + 256;
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
    double *partial = cv.take<double>((size_t)K * n_maps * kScoreMaxBlocks * 3);
    TGNN_CHECK_HIP(hipMemsetAsync(err, 0, (size_t)K * sizeof(int32_t), s));
    ManyDesc d{K, {node_ptr, adj_ptr, col_ptr}, {total_nodes, total_adj_edges, total_col_edges}, active, counts};
    LossManyArgs a{probs, ld_probs, n_maps, area_ratio, ld_area, adj_edge_index, adj_edge_len, ld_len, col_edge_index,
                   collision_weight, align_length_weight, avg_area_weight, losses, terms, err, start, partial};
    many_plan_kernel<<<1, kMnThreads, 0, s>>>(d, 1, 2, start, err);
    // blocks of layout k: clamp(ceil(max(n, ec, ea) / kChunk), 1, 512) <= (n + ec + ea) / kChunk + 1
    const int ub = many_blocks_ub(total_nodes + total_adj_edges + total_col_edges, K);
    loss_many_partial_kernel<<<dim3(ub, n_maps), kMnThreads, 0, s>>>(d, a);
    loss_many_final_kernel<<<dim3(K, n_maps), 64, 0, s>>>(d, a);
    TGNN_CHECK_LAUNCH();
    return TGNN_OK;
}
