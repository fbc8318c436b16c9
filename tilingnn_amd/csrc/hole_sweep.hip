// The guarded acceptance sweep of the greedy loop on the device -- util/algorithms.py: HostSweep.round(ids, prob, guard) with a
// HoleGuard, i.e. the reference's algorithms.py:41-54 with the hole veto of :150-152 before the draw -- for K layouts cut from ONE
// complete graph, one call per greedy round: tgnn_hole_sweep_many.  The sweep stays the reference's SEQUENTIAL sweep, decision for
// decision; what moves is where it runs.  Parallel across layouts (one block each), sequential within one, and a visited node's
// d holes is computed when the walk reaches it instead of for every tile after every acceptance (csrc/union_hole_delta.hip's
// map): the per-visit code is hole_sweep_step.h, which a host program runs as well.
//
// hole_sweep_walk_kernel   ONE BLOCK of 128 threads per layout walks the round's visiting order.  Per position: a node that is
//                          no longer unlabelled ends the walk (the `break`); d holes of its tile under the layout's tile_alive
//                          -- the labels of its contact row counted by all threads (topo::distinct_labels), then the slots of
//                          d chi that name a tile with a share listed in LDS and eight threads per listed slot, summed by
//                          integer atomics in LDS -- ; d holes > 0 is a veto and consumes NO draw; else the next u is consumed
//                          and thr > u (a plain fp64 compare of two host-made numbers) accepts: the node leaves `unlabelled`,
//                          its tile enters tile_alive, the labels of the components it joins are rewritten in two strided
//                          passes over the tiles (hole_sweep_step.h: mark, join, close) so that every label is again the lowest
//                          alive tile of its component, and the node's unlabelled collision neighbours are cleared and appended
//                          to the killed list in row order (a vote per wave gives each its place: the same list on every run)
//                          -- block_accept of hole_sweep_block.h, which the branch walk of tree_sweep.hip calls as well.
//                          The labels live in LDS for the walk on graphs of up to kLabelLdsTiles tiles (copied in and out) and
//                          in the caller's label array beyond; tile_alive and unlabelled are the caller's arrays throughout.
//                          d chi of a visited tile is kept in the caller's chi_cache until a tile of its contact row is
//                          accepted (hole_sweep_step.h): a veto repeated round after round costs the label count alone.
// hole_sweep_stop_kernel   grid (32, K): the stop rule of solve_by_probablistic_greedy -- whether EVERY still-unlabelled node
//                          of the layout is vetoed under the final selection -- with the same block-wide d holes, a node per
//                          block at a time, ending at the first node that is not vetoed.
//
// The walk never tests a visited node against the complete graph's collision rows: an unlabelled node cannot collide with a
// selected node of its own layout, because the layout's collision edges are the graph's restricted to it and every acceptance
// clears the node's collision neighbours.
//
// Every output word of a layout that ran is written by the call (nothing is zeroed first), sums are integer sums, and the lists
// are in a fixed order: the same bytes on every call.  A layout that is inactive or has an empty visiting list is not touched.
#include "hole_sweep_block.h"

namespace tgnn {

constexpr int kSwStopBlocks = 32;            // blocks that share one layout's unlabelled nodes in the stop rule

struct SweepArgs {
    topo::Tiles g;
    int64_t n_layouts, n_nodes, n_nbr, n_visit;
    const int32_t *node_ptr;                 // [K + 1]
    const int32_t *tile_of_node;             // [N]
    const int32_t *nbr_ptr;                  // [N + 1]
    const int32_t *nbr_idx;                  // [n_nbr], local node numbers
    int32_t *unlabelled;                     // [N]
    int32_t *tile_alive;                     // [K][n_tiles]
    int32_t *label;                          // [K][n_tiles]
    int32_t *chi_cache;                      // [K][n_tiles]
    const int32_t *active;                   // [K]
    const int32_t *visit_ptr;                // [K + 1]
    const int32_t *visit_node;               // [V]
    const double *thr, *u;                   // [V]
    int32_t *stats;                          // [K][kStatWords]
    int32_t *accepted;                       // [V]
    int32_t *killed;                         // [N]
    int32_t *trace;                          // [V][2]
    int32_t *err;                            // [K]
    int32_t *found;                          // [K]  (workspace) a node that is not vetoed was found
};

// What the block of layout k works on.  live: active with a visiting list; bad: a table entry outside its array.
struct SweepLayout {
    int64_t n0, n_nodes, v0, n_visit;
    bool live, bad;
};

__device__ __forceinline__ SweepLayout layout_of(const SweepArgs &a, int64_t k) {
    SweepLayout l{0, 0, 0, 0, false, false};
    if (a.active[k] == 0) return l;
    const int64_t v0 = a.visit_ptr[k], v1 = a.visit_ptr[k + 1], n0 = a.node_ptr[k], n1 = a.node_ptr[k + 1];
    if (v0 == v1) return l;
    l.live = true;
    l.bad = v0 < 0 || v1 < v0 || v1 > a.n_visit || n0 < 0 || n1 < n0 || n1 > a.n_nodes;
    l.n0 = n0, l.n_nodes = n1 - n0, l.v0 = v0, l.n_visit = v1 - v0;
    return l;
}

// kInLds: the labels live in LDS for the walk (n_tiles words of dynamic LDS), else in a.label throughout.
template <bool kInLds>
__global__ __launch_bounds__(kSwThreads) void hole_sweep_walk_kernel(SweepArgs a, int64_t layout0) {
    extern __shared__ int32_t label_lds[];
    __shared__ double arc_lo[topo::kMaxWedges][kSwThreads], arc_hi[topo::kMaxWedges][kSwThreads];
    __shared__ SweepShared sh;
    const int tid = threadIdx.x;
    const int64_t k = layout0 + blockIdx.x;
    const int64_t n = a.g.n_tiles;
    const SweepLayout l = layout_of(a, k);
    if (!l.live) return;
    int32_t *stats = a.stats + k * sweep::kStatWords;
    if (l.bad) {
        if (tid < sweep::kStatWords) stats[tid] = 0;
        if (tid == 0) a.err[k] = topo::kErrIndex, a.found[k] = 1;
        return;
    }
    int32_t *alive = a.tile_alive + k * n, *glab = a.label + k * n, *chi = a.chi_cache + k * n, *unl = a.unlabelled + l.n0;
    int32_t *lab = kInLds ? label_lds : glab;
    int32_t *trace = a.trace + 2 * l.v0;
    if (kInLds)
        for (int64_t i = tid; i < n; i += kSwThreads) lab[i] = glab[i];
    if (tid == 0) sh.err_all = 0;
    __syncthreads();
    LdsArcs<kSwThreads> arcs{arc_lo, arc_hi, tid};
    SweepWalk w{a.nbr_ptr + l.n0, a.nbr_idx, a.n_nbr, l.n_nodes, unl, alive, lab, chi, a.accepted + l.v0, a.killed + l.n0, 0, 0};
    int visited = 0, vetoes = 0, draws = 0;                  // the same in every thread
    int err = 0, terr = 0;                                   // err: uniform, ends the walk; terr: this thread's
    for (int64_t pos = 0; pos < l.n_visit; ++pos) {
        const int64_t node = a.visit_node[l.v0 + pos];
        if (node < 0 || node >= l.n_nodes) {
            err |= topo::kErrIndex;
            break;
        }
        const int64_t t = a.tile_of_node[l.n0 + node];
        if (t < 0 || t >= n) {
            err |= topo::kErrIndex;
            break;
        }
        if (unl[node] == 0) {                                // labelled in this round: the walk ends here
            if (tid == 0) trace[2 * pos] = sweep::kBreak, trace[2 * pos + 1] = 0;
            ++visited;
            break;
        }
        const int d = block_hole_delta<true>(a.g, alive, lab, chi, t, arcs, &sh, err);
        if (err != 0) break;                                 // reported, not answered
        ++visited;
        int code = sweep::kVetoed;
        if (d <= 0) {
            const double u = a.u[l.v0 + draws];
            ++draws;
            code = a.thr[l.v0 + pos] > u ? sweep::kAccepted : sweep::kRejected;
        } else {
            ++vetoes;
        }
        if (tid == 0) trace[2 * pos] = code, trace[2 * pos + 1] = d;
        if (code != sweep::kAccepted) continue;
        err |= block_accept<true>(a.g, w, node, t, l.n_nodes, &sh, terr);  // (a layout's killed list holds every node of it)
        if (err != 0) break;
    }
    __syncthreads();
    for (int64_t pos = visited + tid; pos < l.n_visit; pos += kSwThreads) trace[2 * pos] = sweep::kNotReached, trace[2 * pos + 1] = 0;
    if (kInLds)
        for (int64_t i = tid; i < n; i += kSwThreads) glab[i] = lab[i];
    if (terr != 0) atomicOr(&sh.err_all, terr);
    __syncthreads();
    if (tid == 0) {
        stats[sweep::kStatVisited] = visited;
        stats[sweep::kStatVetoes] = vetoes;
        stats[sweep::kStatDraws] = draws;
        stats[sweep::kStatAccepted] = w.n_accepted;
        stats[sweep::kStatKilled] = w.n_killed;
        stats[sweep::kStatAllVetoed] = 1;                    // until hole_sweep_stop_kernel finds a node that is not
        stats[6] = stats[7] = 0;
        a.err[k] = err | sh.err_all;
        a.found[k] = err | sh.err_all;                       // (an error: the stop rule is not evaluated)
    }
}

// The stop rule: stats[kStatAllVetoed] of layout k stays 1 unless an unlabelled node of it has d holes <= 0 under the selection
// the walk left.  Block x of the layout takes the nodes x, x + gridDim.x, ...; a block ends when any block has found one.
__global__ __launch_bounds__(kSwThreads) void hole_sweep_stop_kernel(SweepArgs a, int64_t layout0) {
    __shared__ double arc_lo[topo::kMaxWedges][kSwThreads], arc_hi[topo::kMaxWedges][kSwThreads];
    __shared__ SweepShared sh;
    const int tid = threadIdx.x;
    const int64_t k = layout0 + blockIdx.y;
    const int64_t n = a.g.n_tiles;
    const SweepLayout l = layout_of(a, k);
    if (!l.live || l.bad) return;
    const int32_t *alive = a.tile_alive + k * n, *lab = a.label + k * n, *unl = a.unlabelled + l.n0;
    int32_t *chi = a.chi_cache + k * n;
    LdsArcs<kSwThreads> arcs{arc_lo, arc_hi, tid};
    for (int64_t node = blockIdx.x; node < l.n_nodes; node += gridDim.x) {
        if (unl[node] == 0) continue;
        __syncthreads();
        if (tid == 0) sh.stop = *(volatile int32_t *)(a.found + k);
        __syncthreads();
        if (sh.stop != 0) break;                             // (the next store to sh.stop lies behind the barriers of the evaluation)
        const int64_t t = a.tile_of_node[l.n0 + node];
        int err = t < 0 || t >= n ? topo::kErrIndex : 0;
        const int d = err == 0 ? block_hole_delta<false>(a.g, alive, lab, chi, t, arcs, &sh, err) : 0;
        if (err != 0) {
            if (tid == 0) atomicOr(a.err + k, err), a.found[k] = 1;
            break;
        }
        if (d <= 0) {
            if (tid == 0) a.stats[k * sweep::kStatWords + sweep::kStatAllVetoed] = 0, a.found[k] = 1;
            break;
        }
    }
}

}  // namespace tgnn

using namespace tgnn;

extern "C" size_t tgnn_hole_sweep_workspace_bytes(int64_t n_layouts) {
    if (n_layouts <= 0 || n_layouts > (1ll << 58)) return 0;
    return (size_t)n_layouts * sizeof(int32_t);
}

extern "C" int tgnn_hole_sweep_many(const double *ring_xy, const int32_t *ring_ptr, int64_t n_tiles, const int32_t *touch_ptr,
                                    const int32_t *touch_idx, double tol, double dir_x, double dir_y, int64_t n_layouts,
                                    const int32_t *node_ptr, int64_t n_nodes, const int32_t *tile_of_node, const int32_t *nbr_ptr,
                                    const int32_t *nbr_idx, int64_t n_nbr, int32_t *unlabelled, int32_t *tile_alive, int32_t *label,
                                    int32_t *chi_cache, const int32_t *active, const int32_t *visit_ptr, const int32_t *visit_node, const double *thr,
                                    const double *u, int64_t n_visit, int32_t *stats_out, int32_t *accepted_out,
                                    int32_t *killed_out, int32_t *trace_out, int32_t *err_out, void *ws, size_t ws_bytes,
                                    tgnn_stream_t stream) {
    DeviceGuard guard__(stream);
    if (int rc = check_mask_shape(__func__, n_tiles, n_layouts, tol, dir_x, dir_y)) return rc;
    TGNN_CHECK_ARG(n_nodes >= 0 && n_nodes < (1ll << 31) - 1 && n_nbr >= 0 && n_nbr < (1ll << 31) - 1 && n_visit >= 0 &&
                       n_visit < (1ll << 31) - 1, "n_nodes / n_nbr / n_visit");
    if (n_layouts == 0 || n_tiles == 0 || n_nodes == 0 || n_visit == 0) return TGNN_OK;      // nothing to walk: no output word
    TGNN_CHECK_ARG(node_ptr && tile_of_node && nbr_ptr && (nbr_idx || n_nbr == 0), "null layout table");
    TGNN_CHECK_ARG(unlabelled && tile_alive && label && chi_cache, "null state array");
    TGNN_CHECK_ARG(active && visit_ptr && visit_node && thr && u, "null round array");
    TGNN_CHECK_ARG(stats_out && accepted_out && killed_out && trace_out && err_out, "null output");
    if (int rc = check_mask_arrays(__func__, n_layouts, (1ll << 58) / (n_tiles + 2), ring_xy && ring_ptr && touch_ptr, ws, ws_bytes,
                                   tgnn_hole_sweep_workspace_bytes(n_layouts), sizeof(int32_t)))
        return rc;
    hipStream_t s = static_cast<hipStream_t>(stream);
    SweepArgs a{{reinterpret_cast<const topo::Pt *>(ring_xy), ring_ptr, n_tiles, touch_ptr, touch_idx, tol, dir_x, dir_y},
                n_layouts, n_nodes, n_nbr, n_visit, node_ptr, tile_of_node, nbr_ptr, nbr_idx, unlabelled, tile_alive, label,
                chi_cache, active, visit_ptr, visit_node, thr, u, stats_out, accepted_out, killed_out, trace_out, err_out,
                static_cast<int32_t *>(ws)};
    for_mask_chunks(n_layouts, kMaskGridX, [&](int64_t k0, unsigned g) {
        if (n_tiles <= kLabelLdsTiles)
            hole_sweep_walk_kernel<true><<<g, kSwThreads, sizeof(int32_t) * n_tiles, s>>>(a, k0);
        else
            hole_sweep_walk_kernel<false><<<g, kSwThreads, 0, s>>>(a, k0);
    });
    for_mask_chunks(n_layouts, kMaskGridY, [&](int64_t k0, unsigned gy) {
        hole_sweep_stop_kernel<<<dim3(kSwStopBlocks, gy), kSwThreads, 0, s>>>(a, k0);
    });
    TGNN_CHECK_LAUNCH();
    return TGNN_OK;
}
