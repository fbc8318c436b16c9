// The branch sweeps of the tree search on the device -- util/algorithms.py: solve_by_treesearch, i.e. the reference's
// algorithms.py:138-157 with its hole veto (:150-152) -- for K branches of ONE layout cut from one complete graph, one call per
// step of the search: tgnn_tree_sweep_many.  The branches of a step are K independent SEQUENTIAL walks over the same layout, each
// from its own copy of a queued state: parallel across branches (one block each), sequential within one, and a visited node's
// d holes is computed when the walk reaches it (hole_sweep_block.h, hole_sweep_step.h: the code of hole_sweep.hip).  The per-visit
// rule is tree_sweep_step.h, which a host program runs as well.
//
// tree_fork_kernel         grid (8, K): the four rows of branch k's parent slot are copied to its child slot (nothing to do
//                          when the child reuses its parent's slot); block (0, k) leaves in the workspace whether both slots
//                          lie inside the pool.  The slot contract (include/tgnn.h) makes the copies of a call independent:
//                          no child row is any branch's parent row unless it is that branch's own.
// tree_sweep_walk_kernel   ONE BLOCK of 128 threads per branch walks the branch's visiting order on its child slot.  Per
//                          position: a node that is no longer unlabelled consumes the branch's next u -- u < p passes over it,
//                          else the walk ends --; with check_holes, d holes of the node's tile under the slot's tile_alive, and
//                          d holes > 0 passes over it, no draw; every other node is accepted, no draw, by block_accept of
//                          hole_sweep_block.h, the acceptance of hole_sweep.hip: it leaves `unlabelled`, its tile enters
//                          tile_alive, the labels are rewritten (mark, join, close), the cache forgets the tile's contact row,
//                          and the node's unlabelled collision neighbours are cleared and appended to the killed list in row
//                          order (a vote per wave: the same list on every run), as long as both lists fit the visiting list.
//                          The labels live in LDS for the walk on graphs of up to kLabelLdsTiles tiles and in the slot's row beyond.
//                          Without the geometry (check_holes == 0 only) the slot's three tile rows are never touched.
//
// Every loop is bounded by a list length: no spin, no grid barrier, no atomics on global memory.  Every output word of a branch
// that ran is written by the call, sums are integer sums and the lists are in a fixed order: the same bytes on every call.
#include "hole_sweep_block.h"
#include "tree_sweep_step.h"

namespace tgnn {

constexpr int kForkBlocks = 8;               // blocks that share one branch's copy

struct TreeArgs {
    topo::Tiles g;                           // ring_xy == nullptr: no tile state (check_holes == 0)
    int64_t n_nodes, n_nbr, n_slots, n_branches, n_visit;
    const int32_t *tile_of_node;             // [n_nodes]
    const int32_t *nbr_ptr;                  // [n_nodes + 1]
    const int32_t *nbr_idx;                  // [n_nbr]
    int32_t *unlabelled;                     // [S][n_nodes]
    int32_t *tile_alive;                     // [S][n_tiles]
    int32_t *label;                          // [S][n_tiles]
    int32_t *chi_cache;                      // [S][n_tiles]
    const int32_t *parent_slot;              // [K]
    const int32_t *slot;                     // [K]
    const int32_t *visit_ptr;                // [K + 1]
    const int32_t *visit_node;               // [V]
    const double *p, *u;                     // [V]
    int32_t check_holes;
    int32_t *stats;                          // [K][kStatWords]
    int32_t *accepted;                       // [V]
    int32_t *killed;                         // [V]
    int32_t *trace;                          // [V][2]
    int32_t *err;                            // [K]
    int32_t *fork_err;                       // [K]  (workspace) a slot of the branch lies outside the pool
};

__global__ __launch_bounds__(kSwThreads) void tree_fork_kernel(TreeArgs a, int64_t branch0) {
    const int64_t k = branch0 + blockIdx.y;
    const int64_t from = a.parent_slot[k], to = a.slot[k];
    const bool bad = from < 0 || from >= a.n_slots || to < 0 || to >= a.n_slots;
    if (blockIdx.x == 0 && threadIdx.x == 0) a.fork_err[k] = bad ? topo::kErrIndex : 0;
    if (bad || from == to) return;
    const int64_t first = (int64_t)blockIdx.x * kSwThreads + threadIdx.x, step = (int64_t)gridDim.x * kSwThreads;
    for (int64_t i = first; i < a.n_nodes; i += step) a.unlabelled[to * a.n_nodes + i] = a.unlabelled[from * a.n_nodes + i];
    if (a.g.ring_xy == nullptr) return;
    const int64_t n = a.g.n_tiles;
    for (int64_t i = first; i < n; i += step) {
        a.tile_alive[to * n + i] = a.tile_alive[from * n + i];
        a.label[to * n + i] = a.label[from * n + i];
        a.chi_cache[to * n + i] = a.chi_cache[from * n + i];
    }
}

// kInLds: the labels live in LDS for the walk (n_tiles words of dynamic LDS), else in the slot's row throughout.
// kTiles: the slot's tile rows are kept (the geometry was given); without them nothing of a tile is read.
template <bool kInLds, bool kTiles>
__global__ __launch_bounds__(kSwThreads) void tree_sweep_walk_kernel(TreeArgs a, int64_t branch0) {
    extern __shared__ int32_t label_lds[];
    __shared__ double arc_lo[topo::kMaxWedges][kSwThreads], arc_hi[topo::kMaxWedges][kSwThreads];
    __shared__ SweepShared sh;
    const int tid = threadIdx.x;
    const int64_t k = branch0 + blockIdx.x;
    const int64_t n = a.g.n_tiles;
    const int64_t v0 = a.visit_ptr[k], v1 = a.visit_ptr[k + 1];
    int32_t *stats = a.stats + k * tree::kStatWords;
    if (v0 < 0 || v1 < v0 || v1 > a.n_visit || a.fork_err[k] != 0) {         // (the fork did not run: nothing of a slot is touched)
        if (tid < tree::kStatWords) stats[tid] = 0;
        if (tid == 0) a.err[k] = topo::kErrIndex;
        return;
    }
    const int64_t n_visit = v1 - v0, s = a.slot[k];
    int32_t *unl = a.unlabelled + s * a.n_nodes;
    int32_t *alive = kTiles ? a.tile_alive + s * n : nullptr, *glab = kTiles ? a.label + s * n : nullptr;
    int32_t *chi = kTiles ? a.chi_cache + s * n : nullptr;
    int32_t *lab = kInLds ? label_lds : glab;
    int32_t *trace = a.trace + 2 * v0, *accepted = a.accepted + v0, *killed = a.killed + v0;
    const bool check_holes = kTiles && a.check_holes != 0;
    if (kInLds)
        for (int64_t i = tid; i < n; i += kSwThreads) lab[i] = glab[i];
    if (tid == 0) sh.err_all = 0;
    __syncthreads();
    LdsArcs<kSwThreads> arcs{arc_lo, arc_hi, tid};
    SweepWalk w{a.nbr_ptr, a.nbr_idx, a.n_nbr, a.n_nodes, unl, alive, lab, chi, accepted, killed, 0, 0};
    int visited = 0, vetoes = 0, draws = 0, skipped = 0;     // the same in every thread
    int err = 0, terr = 0;                                   // err: uniform, ends the walk; terr: this thread's
    for (int64_t pos = 0; pos < n_visit; ++pos) {
        const int64_t node = a.visit_node[v0 + pos];
        if (node < 0 || node >= a.n_nodes) {
            err |= topo::kErrIndex;
            break;
        }
        const bool labelled = unl[node] == 0;
        int64_t t = 0;
        int d = 0;
        double u = 0.0;
        if (tree::consumes_draw(labelled)) {                 // (draws <= pos: inside the branch's part of u)
            u = a.u[v0 + draws];
            ++draws;
        } else if (kTiles) {
            t = a.tile_of_node[node];
            if (t < 0 || t >= n) {
                err |= topo::kErrIndex;
                break;
            }
            if (check_holes) {
                d = block_hole_delta<true>(a.g, alive, lab, chi, t, arcs, &sh, err);
                if (err != 0) break;                         // reported, not answered
            }
        }
        const int code = tree::visit_code(labelled, u, a.p[v0 + pos], check_holes, d);
        ++visited;
        if (tid == 0) trace[2 * pos] = code, trace[2 * pos + 1] = d;
        if (code == sweep::kBreak) break;
        skipped += code == tree::kSkipped;
        vetoes += code == sweep::kVetoed;
        if (code != sweep::kAccepted) continue;
        // tree::lists_fit for this node and every chunk of its row: both lists together never exceed the visiting list
        err |= block_accept<kTiles>(a.g, w, node, t, n_visit - w.n_accepted - 1, &sh, terr);
        if (err != 0) break;
    }
    __syncthreads();
    for (int64_t pos = visited + tid; pos < n_visit; pos += kSwThreads) trace[2 * pos] = sweep::kNotReached, trace[2 * pos + 1] = 0;
    for (int64_t i = w.n_accepted + tid; i < n_visit; i += kSwThreads) accepted[i] = -1;
    for (int64_t i = w.n_killed + tid; i < n_visit; i += kSwThreads) killed[i] = -1;
    if (kInLds)
        for (int64_t i = tid; i < n; i += kSwThreads) glab[i] = lab[i];
    if (terr != 0) atomicOr(&sh.err_all, terr);
    __syncthreads();
    if (tid == 0) {
        stats[tree::kStatVisited] = visited;
        stats[tree::kStatVetoes] = vetoes;
        stats[tree::kStatDraws] = draws;
        stats[tree::kStatAccepted] = w.n_accepted;
        stats[tree::kStatKilled] = w.n_killed;
        stats[tree::kStatSkipped] = skipped;
        stats[6] = stats[7] = 0;
        a.err[k] = err | sh.err_all;
    }
}

}  // namespace tgnn

using namespace tgnn;

extern "C" size_t tgnn_tree_sweep_workspace_bytes(int64_t n_branches) {
    if (n_branches <= 0 || n_branches > (1ll << 58)) return 0;
    return (size_t)n_branches * sizeof(int32_t);
}

extern "C" int tgnn_tree_sweep_many(const double *ring_xy, const int32_t *ring_ptr, int64_t n_tiles, const int32_t *touch_ptr,
                                    const int32_t *touch_idx, double tol, double dir_x, double dir_y, int64_t n_nodes,
                                    const int32_t *tile_of_node, const int32_t *nbr_ptr, const int32_t *nbr_idx, int64_t n_nbr,
                                    int64_t n_slots, int32_t *unlabelled, int32_t *tile_alive, int32_t *label, int32_t *chi_cache,
                                    int64_t n_branches, const int32_t *parent_slot, const int32_t *slot, const int32_t *visit_ptr,
                                    const int32_t *visit_node, const double *p, const double *u, int64_t n_visit,
                                    int32_t check_holes, int32_t *stats_out, int32_t *accepted_out, int32_t *killed_out,
                                    int32_t *trace_out, int32_t *err_out, void *ws, size_t ws_bytes, tgnn_stream_t stream) {
    DeviceGuard guard__(stream);
    if (int rc = check_mask_shape(__func__, n_tiles, n_branches, tol, dir_x, dir_y)) return rc;
    TGNN_CHECK_ARG(n_nodes >= 0 && n_nodes < (1ll << 31) - 1 && n_nbr >= 0 && n_nbr < (1ll << 31) - 1 && n_visit >= 0 &&
                       n_visit < (1ll << 31) - 1 && n_slots >= 0 && n_slots < (1ll << 31) - 1, "n_nodes / n_nbr / n_visit / n_slots");
    if (n_branches == 0 || n_nodes == 0 || n_visit == 0) return TGNN_OK;     // nothing to walk: no output word
    const bool no_geometry = !ring_xy && !ring_ptr && !touch_ptr && !touch_idx;
    const bool geometry = ring_xy && ring_ptr && touch_ptr;                   // (touch_idx may be NULL: no contact)
    TGNN_CHECK_ARG(geometry || (no_geometry && check_holes == 0), "null tile array");
    TGNN_CHECK_ARG(n_slots > 0 && n_slots <= (1ll << 58) / (n_tiles + n_nodes + 2), "n_slots");
    TGNN_CHECK_ARG(nbr_ptr && (nbr_idx || n_nbr == 0) && (tile_of_node || !geometry), "null layout table");
    TGNN_CHECK_ARG(unlabelled && (!geometry || (tile_alive && label && chi_cache)), "null state array");
    TGNN_CHECK_ARG(parent_slot && slot && visit_ptr && visit_node && p && u, "null step array");
    TGNN_CHECK_ARG(stats_out && accepted_out && killed_out && trace_out && err_out, "null output");
    if (int rc = check_mask_arrays(__func__, n_branches, 1ll << 58, true, ws, ws_bytes, tgnn_tree_sweep_workspace_bytes(n_branches),
                                   sizeof(int32_t)))
        return rc;
    hipStream_t s = static_cast<hipStream_t>(stream);
    TreeArgs a{{reinterpret_cast<const topo::Pt *>(ring_xy), ring_ptr, n_tiles, touch_ptr, touch_idx, tol, dir_x, dir_y},
               n_nodes, n_nbr, n_slots, n_branches, n_visit, tile_of_node, nbr_ptr, nbr_idx, unlabelled, tile_alive, label,
               chi_cache, parent_slot, slot, visit_ptr, visit_node, p, u, check_holes, stats_out, accepted_out, killed_out,
               trace_out, err_out, static_cast<int32_t *>(ws)};
    for_mask_chunks(n_branches, kMaskGridY, [&](int64_t k0, unsigned gy) {
        tree_fork_kernel<<<dim3(kForkBlocks, gy), kSwThreads, 0, s>>>(a, k0);
    });
    for_mask_chunks(n_branches, kMaskGridX, [&](int64_t k0, unsigned g) {
        if (!geometry)
            tree_sweep_walk_kernel<false, false><<<g, kSwThreads, 0, s>>>(a, k0);
        else if (n_tiles <= kLabelLdsTiles)
            tree_sweep_walk_kernel<true, true><<<g, kSwThreads, sizeof(int32_t) * n_tiles, s>>>(a, k0);
        else
            tree_sweep_walk_kernel<false, true><<<g, kSwThreads, 0, s>>>(a, k0);
    });
    TGNN_CHECK_LAUNCH();
    return TGNN_OK;
}
