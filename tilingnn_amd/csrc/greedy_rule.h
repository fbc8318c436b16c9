// The acceptance rule of the device greedy loop, stated once for csrc/greedy.hip (one layout) and csrc/greedy_many.hip (K layouts):
// the running mean, the visiting order, the test against a counter-based draw, the flag bits of a round, and the one-block loop
// that runs the remaining rounds of a solve.  The rule (first half) is plain C++ on purpose (no HIP header, no global state): the
// kernels call it per node and per edge, and tests/host/greedy_rule_test.cpp walks rounds with the very same code under
// AddressSanitizer and UBSan.  What the rule substitutes in the reference, and why: the head of csrc/greedy.hip.
#ifndef TGNN_GREEDY_RULE_H
#define TGNN_GREEDY_RULE_H
#include <math.h>
#include <stdint.h>

#if defined(__HIPCC__)
#define TGNN_GREEDY_FN __host__ __device__ __forceinline__
#else
#define TGNN_GREEDY_FN inline
#endif

namespace tgnn {

// flags of a sub-layout node within a round; the last two only in the finishing block, which keeps nodes that have left
constexpr int kGreedyBeaten = 1;                            // a collision neighbour comes first in the visiting order
constexpr int kGreedyAccepted = 2;
constexpr int kGreedyGone = 4;                              // labelled before this round: takes no part, nor do the edges at it
constexpr int kGreedyLeaving = 8;                           // labelled by an acceptance of this round: gone from the next
constexpr int kFinThreads = 1024;                           // the finishing block
constexpr int kFinMaxNodes = 4096;                          // == tgnn_greedy_finish_max_nodes()

// splitmix64 of (seed, round, node) -> uniform double in [0, 1)
TGNN_GREEDY_FN double greedy_uniform(unsigned long long seed, unsigned round, unsigned long long node) {
    unsigned long long z = seed + 0x9E3779B97F4A7C15ull * (node + 1ull) + 0xD1B54A32D192ED03ull * (unsigned long long)(round + 1u);
    z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull;
    z = (z ^ (z >> 27)) * 0x94D049BB133111EBull;
    z ^= z >> 31;
    return (double)(z >> 11) * (1.0 / 9007199254740992.0);
}
// p_v of the round (algorithms.py:33-34): the round's probability folded into the running geometric mean
TGNN_GREEDY_FN double greedy_mean(double saved, double prob, int round) {
    return pow(pow(saved, (double)(round - 1)) * prob, 1.0 / (double)round);
}
// Of a collision edge (u, v), u != v, the end that comes LATER in the visiting order (larger p first, the smaller node number on
// ties): that end is beaten.  Callers mark it from EITHER direction of the pair, so that a collision stored one way only still
// keeps the two apart WITHIN THIS ROUND.  Labelling follows the stored direction only, so the final selection is collision free
// only when both directions are stored, as the reference stores them (tile_graph.py:206-207).
TGNN_GREEDY_FN int64_t greedy_beaten_end(int64_t u, int64_t v, double pu, double pv) {
    return (pv > pu || (pv == pu && v < u)) ? u : v;
}
// the reference's test exp(p_v - 1) > u_v (algorithms.py:51), u_v keyed by (seed, round, ORIGINAL node number)
TGNN_GREEDY_FN bool greedy_accepts(double p, unsigned long long seed, int round, int64_t original_node) {
    return exp((p - 1.0) * 1.0) > greedy_uniform(seed, (unsigned)round, (unsigned long long)original_node);
}

#if defined(__HIPCC__)
// The END of a solve as ONE block: a sub-layout without adjacency edges (or without collision edges) gets probability 1 for every
// node from ML_Solver.predict without the network (ml_solver.py:31-32), and so does every sub-layout of it -- the remaining
// rounds are mean, beaten, accept, label with prob = 1 on ever smaller sub-layouts.  The block runs them all on the sub-layout it
// is given: nodes that have left (alive == 0) and the edges at them are skipped instead of compacted away; the geometric mean, the
// visiting order (ties by node number: compaction keeps the order), the draws (keyed by seed, round and ORIGINAL node number) and
// the round numbers are those of the round-by-round path, hence the same selection, order and round count.
// kPacked = false: `inverse` may be NULL (the identity) and is trusted.  kPacked = true (a layout of a packed batch): `inverse`
// is given, and an entry outside [0, n_full) sets *err and its node never takes part.  n_sub <= kFinMaxNodes, kFinThreads threads.
// out[0] rounds run, out[1] nodes left.
template <bool kPacked>
__device__ __forceinline__ void greedy_finish_block(const int64_t *__restrict__ inverse, int n_sub, int64_t n_full,
                                                    const int64_t *__restrict__ col, int64_t ec, int first_round, int max_rounds,
                                                    unsigned long long seed, double *__restrict__ saved, int *__restrict__ alive,
                                                    int *__restrict__ selected, long long *__restrict__ count, int *__restrict__ err,
                                                    int *__restrict__ out) {
    __shared__ double p[kFinMaxNodes];
    __shared__ __attribute__((aligned(16))) unsigned char flags[kFinMaxNodes];
    __shared__ int left, accepted, bad_inverse;
    const int tid = threadIdx.x;
    const auto original = [&](int64_t i) -> int64_t { return kPacked || inverse ? inverse[i] : i; };
    const auto set_bit = [&](int64_t i, unsigned bit) {          // four byte flags to the word
        atomicOr(reinterpret_cast<unsigned *>(flags) + (i >> 2), bit << (8 * (i & 3)));
    };
    if (kPacked) {
        if (tid == 0) bad_inverse = 0;
        __syncthreads();
    }
    for (int i = tid; i < n_sub; i += kFinThreads) {
        const int64_t o = original(i);
        if (kPacked && (o < 0 || o >= n_full)) { bad_inverse = 1; flags[i] = kGreedyGone; continue; }
        flags[i] = alive[o] ? 0 : kGreedyGone;
    }
    __syncthreads();
    if (kPacked && bad_inverse && tid == 0) *err = 1;
    int round = first_round, rounds_run = 0;
    for (;; ++round) {
        if (tid == 0) { left = 0; accepted = 0; }
        __syncthreads();
        int mine = 0;
        for (int i = tid; i < n_sub; i += kFinThreads) {       // mean
            if (flags[i] & kGreedyGone) continue;
            ++mine;
            const int64_t o = original(i);
            const double v = greedy_mean(saved[o], 1.0, round);
            saved[o] = v;
            p[i] = v;
            flags[i] = 0;
        }
        if (mine) atomicAdd(&left, mine);
        __syncthreads();
        if (left == 0 || rounds_run >= max_rounds) break;    // (uniform)
        ++rounds_run;
        for (int64_t e = tid; e < ec; e += kFinThreads) {      // beaten
            const int64_t u = col[e], v = col[ec + e];
            if (u < 0 || u >= n_sub || v < 0 || v >= n_sub) { *err = 1; continue; }
            if (u == v || ((flags[u] | flags[v]) & kGreedyGone)) continue;
            set_bit(greedy_beaten_end(u, v, p[u], p[v]), kGreedyBeaten);
        }
        __syncthreads();
        int acc = 0;
        for (int i = tid; i < n_sub; i += kFinThreads) {       // accept
            if (flags[i] & (kGreedyBeaten | kGreedyGone)) continue;
            const int64_t o = original(i);
            if (greedy_accepts(p[i], seed, round, o)) {
                flags[i] |= kGreedyAccepted;
                alive[o] = 0;
                selected[o] = round;
                ++acc;
            }
        }
        if (acc) atomicAdd(&accepted, acc);
        __syncthreads();
        for (int64_t e = tid; e < ec; e += kFinThreads) {      // label
            const int64_t u = col[e], v = col[ec + e];
            if (u < 0 || u >= n_sub || v < 0 || v >= n_sub) continue;
            if ((flags[u] & kGreedyAccepted) && !(flags[v] & kGreedyGone)) {
                alive[original(v)] = 0;
                set_bit(v, kGreedyLeaving);
            }
        }
        __syncthreads();
        for (int i = tid; i < n_sub; i += kFinThreads)
            if (flags[i] & (kGreedyAccepted | kGreedyLeaving)) flags[i] = kGreedyGone;
        if (tid == 0 && accepted) atomicAdd(reinterpret_cast<unsigned long long *>(count), (unsigned long long)accepted);
        __syncthreads();
    }
    if (tid == 0) {
        out[0] = rounds_run;
        out[1] = left;
    }
}
#endif

}  // namespace tgnn
#endif
