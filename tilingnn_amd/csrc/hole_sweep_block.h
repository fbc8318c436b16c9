// What the walks over one complete graph share on the device (csrc/hole_sweep.hip: a block per layout; csrc/tree_sweep.hip: a
// block per branch of a tree search): the block's size, its words of LDS and d holes of one tile by the whole block.  The
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

}  // namespace tgnn
