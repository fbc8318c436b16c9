// What every candidate tile would do to the topology of a collision-free selection -- the map behind the reference's hole veto
// (util/algorithms.py:150-152, check_holes -> exist_hole: refuse a tile whose union with the selection has an interior ring) --
// for K masks of the complete graph and ALL their candidates in one call: delta_out[k][t] = {d components, d holes} =
// tgnn_union_topology(mask k + {t}) - tgnn_union_topology(mask k), state_out[k][t] = candidate / alive / blocked / refused.
// Inputs are those of csrc/union_topology.hip.  holes = components - chi (Euler), and one tile changes both only near itself:
// union_hole_delta_point.h has the derivation and the code per candidate, which a host program runs as well.
//
// Launch shape.
//   union_hole_delta_label_kernel  ONE BLOCK per mask: label_components of union_masks.h (min-label propagation over the
//                                  contact rows with pointer jumping, at most n_tiles + 1 rounds), the labels in LDS for graphs
//                                  of up to 6 144 tiles and in the workspace beyond, written to the workspace at the end; and
//                                  the mask's refusal word from the collision rows of its alive tiles.
//   union_hole_delta_kernel        grid (ceil(n_tiles / 32), K), 128 threads.  First FOUR THREADS per tile of the block's 32,
//                                  each a quarter of the tile's rows: alive, blocked (collision row) or candidate; a candidate
//                                  counts the labels of its contact row (d components) and, touching nothing, is answered
//                                  {+1, 0} on the spot; the others enter the block's list in LDS.  Then the (listed candidate, slot) pairs -- the candidate itself and
//                                  the entries of its contact row -- that name an alive tile are listed in LDS, and EIGHT THREADS
//                                  per listed pair compute that tile's share of d chi (every fourth vertex each, with or
//                                  without the candidate): candidates are a fraction of the tiles
//                                  and alive tiles an eighth of a contact row, so threads per candidate, or per pair, would idle
//                                  most lanes (the finding of section 35, twice).  A point's arcs live in LDS, [slot][thread],
//                                  128 threads x 16 arcs x 16 B = 32 KB as in union_topology_chi_kernel.  The shares are added
//                                  per candidate by integer atomics in LDS and written once.
// Every word of both outputs and every workspace word that is read is written by the call itself: nothing is zeroed first, and
// integer sums make every call give the same bytes.
#include "union_masks.h"
#include "union_hole_delta_point.h"

namespace tgnn {

constexpr int kHdThreads = 128;
constexpr int kHdWhoBits = 5;
constexpr int kHdTiles = 1 << kHdWhoBits;    // tiles of one block of the delta kernel: 32, so that one mask alone fills 40 blocks on ring 9
constexpr int kHdParts = kHdThreads / kHdTiles;    // threads that share one tile's rows in the first phase
constexpr int kHdSub = 8;                    // threads that share one (candidate, tile) pair in the second phase
constexpr int kHdItems = 1024;               // (candidate, slot) pairs listed at a time: 4 KB of LDS (37 KB a block: 4 blocks a CU)
constexpr int kHdLabelThreads = 256;

struct HoleArgs : MaskSet {
    int32_t *refused;                        // [K]            (workspace)
    int32_t *label;                          // [K][n_tiles]   (workspace)
    int32_t *delta;                          // [K][n_tiles][2]
    int32_t *state;                          // [K][n_tiles]
};

// kInLds: the labels and the list of the mask's alive tiles live in LDS (2 n_tiles words of dynamic LDS), a round visits the
// alive tiles only and the labels are copied to the workspace at the end; otherwise they live in the workspace throughout
// (union_masks.h: label_components runs the rounds).
template <bool kInLds>
__global__ __launch_bounds__(kHdLabelThreads) void union_hole_delta_label_kernel(HoleArgs a, int64_t mask0) {
    extern __shared__ int32_t label_lds[];
    __shared__ int changed, collide, n_alive;
    const int tid = threadIdx.x;
    const int64_t k = mask0 + blockIdx.x;
    const int n = (int)a.g.n_tiles;
    const int32_t *al = a.alive + k * a.g.n_tiles;
    int32_t *out = a.label + k * a.g.n_tiles;
    volatile int32_t *lab = kInLds ? label_lds : out;
    int32_t *list = label_lds + n;                           // (kInLds only)
    if (tid == 0) collide = n_alive = 0;
    __syncthreads();
    int err = 0;
    for (int i = tid; i < n; i += kHdLabelThreads) {
        const bool alive = al[i] != 0;
        lab[i] = alive ? i : -1;
        if (!alive) continue;
        if (kInLds) list[atomicAdd(&n_alive, 1)] = i;
        if (topo::collides(a.col_ptr, a.col_idx, al, i, n, 0, 1, err)) collide = 1;
    }
    label_components<kHdLabelThreads, kInLds>(a.g, lab, list, &n_alive, &changed, err);
    if (kInLds)
        for (int i = tid; i < n; i += kHdLabelThreads) out[i] = lab[i];
    if (tid == 0) a.refused[k] = collide;                    // (set before the barriers of the loop's first round)
    if (err != 0) atomicOr(a.err_flag, err);
}

__global__ __launch_bounds__(kHdThreads) void union_hole_delta_kernel(HoleArgs a, int64_t mask0) {
    __shared__ double arc_lo[topo::kMaxWedges][kHdThreads], arc_hi[topo::kMaxWedges][kHdThreads];
    __shared__ int list[kHdTiles], dchi[kHdTiles], blocked[kHdTiles], distinct[kHdTiles], touching[kHdTiles], items[kHdItems];
    __shared__ int n_list, max_row, n_items;
    const int tid = threadIdx.x, mine = tid & (kHdTiles - 1), part = tid >> kHdWhoBits;
    const int64_t n = a.g.n_tiles;
    const int64_t t0 = (int64_t)blockIdx.x * kHdTiles, t = t0 + mine;
    const int64_t k = mask0 + blockIdx.y;
    const int32_t *al = a.alive + k * n;
    const int32_t *lab = a.label + k * n;
    if (tid == 0) n_list = max_row = n_items = 0;
    if (tid < kHdTiles) dchi[tid] = blocked[tid] = distinct[tid] = touching[tid] = 0;
    __syncthreads();
    const bool refused = a.refused[k] != 0;                  // (uniform over the block)
    int err = 0;
    // 1. kHdParts threads per tile of the block, each an equal share of the tile's rows: the collision row says whether a dead
    // tile is blocked, the labels of the contact row of a candidate give d components; then the first of them answers or lists it
    const bool dead = t < n && !refused && al[t] == 0;
    if (dead) {
        bool hit = part == 0 && a.g.ring_ptr[t + 1] - a.g.ring_ptr[t] < 3;
        hit |= topo::collides(a.col_ptr, a.col_idx, al, t, n, part, kHdParts, err);
        if (hit) blocked[mine] = 1;
    }
    __syncthreads();
    if (dead && blocked[mine] == 0) {
        int alive_here;
        const int found = topo::distinct_labels(a.g, lab, t, part, kHdParts, alive_here, err);
        if (alive_here != 0) {
            atomicAdd(&distinct[mine], found);
            atomicAdd(&touching[mine], alive_here);
        }
    }
    __syncthreads();
    int state = topo::kStateRefused, dcomp = 0;
    bool listed = false;
    if (tid < kHdTiles && t < n && !refused) {
        state = !dead ? topo::kStateAlive : blocked[mine] != 0 ? topo::kStateBlocked : topo::kStateCandidate;
        if (state == topo::kStateCandidate) {
            dcomp = 1 - distinct[mine];
            if (touching[mine] != 0) {
                listed = true;
                list[atomicAdd(&n_list, 1)] = mine;
                atomicMax(&max_row, a.g.touch_ptr[t + 1] - a.g.touch_ptr[t]);
            }
        }
    }
    __syncthreads();
    // 2. the (listed candidate, slot) pairs -- slot 0 the candidate itself, slot s entry s - 1 of its contact row -- a chunk of
    // slots at a time: first the pairs that name a tile with a share (alive, 3 vertices or more) are listed, then kHdSub threads
    // per listed pair do the work.  An eighth of a row is alive: without the list seven lanes in eight would wait for the eighth.
    const int cands = n_list, slots = max_row + 1;
    const int step = cands > 0 ? kHdItems / cands : 1;       // cands <= kHdTiles: a chunk never overflows the list
    LdsArcs<kHdThreads> arcs{arc_lo, arc_hi, tid};
    for (int s0 = 0; cands > 0 && s0 < slots; s0 += step) {
        const int chunk = (slots - s0 < step ? slots - s0 : step) * cands;
        for (int w = tid; w < chunk; w += kHdThreads) {
            const int who = list[w % cands], slot = s0 + w / cands;
            const int64_t c = t0 + who;
            if (slot > 0) {
                const int cc = a.g.touch_ptr[c] + slot - 1;
                int64_t j;
                if (cc >= a.g.touch_ptr[c + 1] || !topo::delta_chi_row_tile(a.g, al, c, cc, j, err)) continue;
            }
            items[atomicAdd(&n_items, 1)] = who | (slot << kHdWhoBits);
        }
        __syncthreads();
        const int count = n_items;
        // kHdSub threads per listed pair: every fourth vertex of the tile each, the term with the candidate or the one without
        for (int w = tid; w < count * kHdSub; w += kHdThreads) {
            const int item = items[w / kHdSub], sub = w % kHdSub;
            const int who = item & (kHdTiles - 1), slot = item >> kHdWhoBits;
            const int64_t c = t0 + who;
            const int64_t i = slot == 0 ? c : a.g.touch_idx[a.g.touch_ptr[c] + slot - 1];     // (checked when it was listed)
            const int verts = a.g.ring_ptr[i + 1] - a.g.ring_ptr[i];
            int share = 0;
            for (int v = sub >> 1; v < verts; v += kHdSub / 2) share += topo::delta_chi_vertex(a.g, al, c, i, v, (sub & 1) != 0, arcs, err);
            if (share != 0) atomicAdd(&dchi[who], share);
        }
        __syncthreads();
        if (tid == 0) n_items = 0;
        __syncthreads();
    }
    if (tid < kHdTiles && t < n) {
        a.state[k * n + t] = state;
        a.delta[2 * (k * n + t) + 0] = state == topo::kStateCandidate ? dcomp : 0;
        a.delta[2 * (k * n + t) + 1] = listed ? dcomp - dchi[tid] : 0;
    }
    if (err != 0) atomicOr(a.err_flag, err);
}

}  // namespace tgnn

using namespace tgnn;

extern "C" size_t tgnn_union_hole_delta_workspace_bytes(int64_t n_masks, int64_t n_tiles) {
    if (n_masks <= 0 || n_tiles <= 0 || n_masks > (1ll << 58) / (n_tiles + 2)) return 0;
    return (size_t)n_masks * ((size_t)n_tiles + 1) * sizeof(int32_t);
}

extern "C" int tgnn_union_hole_delta(const double *ring_xy, const int32_t *ring_ptr, int64_t n_tiles, const int32_t *col_ptr,
                                     const int32_t *col_idx, const int32_t *touch_ptr, const int32_t *touch_idx,
                                     const int32_t *alive, int64_t n_masks, double tol, double dir_x, double dir_y,
                                     int32_t *delta_out, int32_t *state_out, int32_t *err_flag, void *ws, size_t ws_bytes,
                                     tgnn_stream_t stream) {
    DeviceGuard guard__(stream);
    if (int rc = check_mask_shape(__func__, n_tiles, n_masks, tol, dir_x, dir_y)) return rc;
    if (n_masks == 0 || n_tiles == 0) return TGNN_OK;        // no output word
    TGNN_CHECK_ARG(delta_out && state_out && err_flag, "null delta_out / state_out / err_flag");
    if (int rc = check_mask_arrays(__func__, n_masks, (1ll << 58) / (n_tiles + 2), ring_xy && ring_ptr && col_ptr && touch_ptr && alive,
                                   ws, ws_bytes, tgnn_union_hole_delta_workspace_bytes(n_masks, n_tiles), sizeof(int32_t)))
        return rc;
    hipStream_t s = static_cast<hipStream_t>(stream);
    int32_t *words = static_cast<int32_t *>(ws);
    HoleArgs a{{{reinterpret_cast<const topo::Pt *>(ring_xy), ring_ptr, n_tiles, touch_ptr, touch_idx, tol, dir_x, dir_y},
                col_ptr, col_idx, alive, n_masks, err_flag},
               words, words + n_masks, delta_out, state_out};
    for_mask_chunks(n_masks, kMaskGridX, [&](int64_t k0, unsigned g) {
        if (n_tiles <= kLabelLdsTiles)
            union_hole_delta_label_kernel<true><<<g, kHdLabelThreads, 2 * sizeof(int32_t) * n_tiles, s>>>(a, k0);
        else
            union_hole_delta_label_kernel<false><<<g, kHdLabelThreads, 0, s>>>(a, k0);
    });
    const unsigned gx = (unsigned)((n_tiles + kHdTiles - 1) / kHdTiles);
    for_mask_chunks(n_masks, kMaskGridY, [&](int64_t k0, unsigned gy) {
        union_hole_delta_kernel<<<dim3(gx, gy), kHdThreads, 0, s>>>(a, k0);
    });
    TGNN_CHECK_LAUNCH();
    return TGNN_OK;
}
