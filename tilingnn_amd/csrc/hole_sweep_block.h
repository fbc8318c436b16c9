// What the walks over one complete graph share on the device (csrc/hole_sweep.hip: a block per layout; csrc/tree_sweep.hip: a
// block per branch of a tree search): the block's size, its words of LDS, d holes of one tile by the whole block
// (block_hole_delta) and the acceptance of a node by the whole block (block_accept), the only statement of it on the device.  The
// per-visit steps themselves are hole_sweep_step.h.
#pragma once
#include "union_masks.h"
#include "hole_sweep_step.h"

namespace tgnn {

constexpr int kSwThreads = 128;
constexpr int kSwWaves = kSwThreads / 64;

struct SweepShared {
    int distinct, touching, dchi, err, n_items, merged, stop, err_all;
    int wave_kills[kSwWaves];
    int items[kSwThreads];
};

// d holes of tile t under (alive, lab) by the whole block; the same value in every thread.  Begins and ends behind a barrier.
// d chi comes from chi_cache when it is known there; kStore: a computed one is stored there (the walk; the stop rule only reads,
// so that what the cache knows does not depend on which of its blocks ended first).
// err_out gets the error bits of the evaluation: then the value is not to be used.
template <bool kStore>
__device__ __forceinline__ int block_hole_delta(const topo::Tiles &g, const int32_t *alive, const int32_t *lab, int32_t *chi_cache,
                                                int64_t t, LdsArcs<kSwThreads> &arcs, SweepShared *sh, int &err_out) {
    const int tid = threadIdx.x;
    __syncthreads();                                         // the words of the last evaluation have been read
    if (tid == 0) sh->distinct = sh->touching = sh->dchi = sh->err = sh->n_items = 0;
    __syncthreads();
    const bool open = sweep::may_change_holes(g, alive, t);
    int err = 0;
    if (open) {
        int here;
        const int found = topo::distinct_labels(g, lab, t, tid, kSwThreads, here, err);
        if (here != 0) {
            atomicAdd(&sh->distinct, found);
            atomicAdd(&sh->touching, here);
        }
    }
    if (err != 0) atomicOr(&sh->err, err);
    __syncthreads();
    const bool touching = open && sh->touching != 0 && sh->err == 0;    // (uniform: read behind a barrier)
    const int32_t known = touching ? chi_cache[t] : 0;       // (stored, if at all, behind the barriers of the loop below)
    const bool work = touching && known == sweep::kChiUnknown;
    if (work) {
        const int slots = sweep::chi_slots(g, t);
        for (int s0 = 0; s0 < slots; s0 += kSwThreads) {
            err = 0;
            const int slot = s0 + tid;
            // an eighth of a row is alive: list the slots with a share first, then kChiSub threads per listed slot
            if (slot < slots && sweep::chi_slot_has_share(g, alive, t, slot, err)) sh->items[atomicAdd(&sh->n_items, 1)] = slot;
            __syncthreads();
            const int count = sh->n_items;
            int share = 0;
            for (int w = tid; w < count * sweep::kChiSub; w += kSwThreads)
                share += sweep::chi_item(g, alive, t, sh->items[w / sweep::kChiSub], w % sweep::kChiSub, arcs, err);
            if (share != 0) atomicAdd(&sh->dchi, share);
            if (err != 0) atomicOr(&sh->err, err);
            __syncthreads();
            if (tid == 0) sh->n_items = 0;
            __syncthreads();
        }
    }
    err_out |= sh->err;
    if (kStore && work && tid == 0 && sh->err == 0) chi_cache[t] = sh->dchi;
    return touching ? 1 - sh->distinct - (work ? sh->dchi : known) : 0;
}

// What the walk accepts into: a layout's or a slot's own rows and tables (node numbers local to them) and the walk's two lists.
// n_accepted and n_killed are the same in every thread.
struct SweepWalk {
    const int32_t *nbr_ptr, *nbr_idx;        // the collision rows of the nodes: [n_nodes + 1], [n_nbr]
    int64_t n_nbr, n_nodes;
    int32_t *unl, *alive, *lab, *chi;        // unlabelled [n_nodes]; the tile rows [n_tiles] (not read without kTiles)
    int32_t *accepted, *killed;
    int n_accepted, n_killed;
};

// Accepts `node`, of tile t, by the whole block: the node leaves `unl` and enters the accepted list, its tile enters `alive` with
// the labels of the component it joins rewritten (hole_sweep_step.h: mark, join, close) and d chi of its contact row forgotten,
// and its unlabelled collision neighbours are cleared and appended to the killed list in row order (a vote per wave gives each
// its place).  Begins and ends behind a barrier.  Returns error bits, the same in every thread: a collision row outside
// [0, n_nbr] is met before anything is written, and so is a killed list without room; a row that outgrows `room` -- the nodes the
// killed list may hold beside this acceptance -- ends the acceptance with the chunk unwritten.  terr gets this thread's own bits.
// kTiles: false when there is no tile state; then t, g and the tile rows are not read.
template <bool kTiles>
__device__ __forceinline__ int block_accept(const topo::Tiles &g, SweepWalk &w, int64_t node, int64_t t, int64_t room, SweepShared *sh,
                                            int &terr) {
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    __syncthreads();                                         // every thread has read unl[node] and the words of the last vote
    // label_collision_neighbor's row
    const int64_t r0 = w.nbr_ptr[node], r1 = w.nbr_ptr[node + 1];
    if (r0 < 0 || r1 < r0 || r1 > w.n_nbr || w.n_killed > room) return topo::kErrIndex;
    const bool fresh = kTiles && w.alive[t] == 0;
    if (tid == 0) {
        w.unl[node] = 0;
        w.accepted[w.n_accepted] = (int32_t)node;
    }
    ++w.n_accepted;
    __syncthreads();
    if (fresh) {
        const int64_t n = g.n_tiles;
        if (tid == 0) sh->merged = sweep::begin_merge(w.alive, w.lab, t);
        __syncthreads();
        for (int cc = g.touch_ptr[t] + tid; cc < g.touch_ptr[t + 1]; cc += kSwThreads) {
            const int32_t root = sweep::mark_root(g, w.lab, t, cc, terr);
            if (root < n) atomicMin(&sh->merged, root);
            sweep::forget_chi(g, w.chi, cc, terr);
        }
        __syncthreads();
        const int32_t m = sh->merged;
        for (int64_t i = tid; i < n; i += kSwThreads) sweep::join_member(w.lab, n, i, m);
        __syncthreads();
        for (int64_t i = tid; i < n; i += kSwThreads) sweep::close_root(w.lab, i, m);
        __syncthreads();
    }
    for (int64_t c0 = r0; c0 < r1; c0 += kSwThreads) {
        const int64_t cc = c0 + tid;
        const int32_t v = cc < r1 ? sweep::killed_by(w.nbr_idx, r0, cc, w.unl, w.n_nodes, terr) : -1;
        const unsigned long long vote = __ballot(v >= 0);
        if (lane == 0) sh->wave_kills[wave] = __popcll(vote);
        __syncthreads();
        int before = __popcll(vote & ((1ull << lane) - 1ull)), total = 0;
        for (int wv = 0; wv < kSwWaves; ++wv) {
            before += wv < wave ? sh->wave_kills[wv] : 0;
            total += sh->wave_kills[wv];
        }
        const bool full = w.n_killed + total > room;         // (uniform: total is the block's)
        if (v >= 0 && !full) {
            w.killed[w.n_killed + before] = v;
            w.unl[v] = 0;
        }
        __syncthreads();
        if (full) return topo::kErrIndex;
        w.n_killed += total;
    }
    return 0;
}

}  // namespace tgnn
