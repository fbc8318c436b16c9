// What the calls over K tile masks of the complete graph share (csrc/union_area.hip, union_topology.hip, union_contour.hip,
// union_hole_delta.hip): the arguments every kernel of theirs takes, the block-wide component labelling, a point's arcs in LDS,
// and on the host the argument checks and the chunked launch loops of the entry points.  The per-tile code is union_components.h.
#pragma once
#include "tgnn_common.h"
#include "union_components.h"

namespace tgnn {

constexpr int64_t kMaskGridY = 65535;        // masks one launch takes along grid y
constexpr int64_t kMaskGridX = 1ll << 30;    // ... and along grid x
constexpr int64_t kLabelLdsTiles = 6144;     // label_components in LDS: 2 x 4 B x 6 144 = 48 KB of dynamic LDS at the most

struct MaskSet {
    topo::Tiles g;
    const int32_t *col_ptr;                  // [n_tiles + 1]
    const int32_t *col_idx;
    const int32_t *alive;                    // [K][n_tiles]
    int64_t n_masks;
    int32_t *err_flag;
};

// The arcs of one point per thread, [slot][thread] (conflict free): what union_topology_point.h asks of its Arcs.
template <int kThreads>
struct LdsArcs {
    double (*lo_)[kThreads], (*hi_)[kThreads];
    int tid;
    __device__ __forceinline__ double &lo(int q) { return lo_[q][tid]; }
    __device__ __forceinline__ double &hi(int q) { return hi_[q][tid]; }
};

// The components of one mask by the whole block (kThreads threads): rounds of topo::lower_label between barriers until a round
// stores nothing.  The caller has written lab[i] = i for an alive tile and -1 for a dead one (no barrier needed after it: a round
// begins with one); only thread w % kThreads ever writes the label of item w.  kInLds: lab is in LDS, list[0 .. *n_alive) names
// the alive tiles and a round visits those only; otherwise lab is in global memory, a round strides over all tiles and list /
// n_alive are not looked at.  changed: a word of LDS.  Ends behind a barrier: every label is final and visible to the block.
// The rounds are capped at n_tiles + 1, which never binds: after round r every tile within r contacts of its component's lowest
// tile carries that tile's index (labels only ever decrease, and a read sees a label no older than the round before), so round
// n_tiles at the latest stores nothing.
template <int kThreads, bool kInLds>
__device__ __forceinline__ void label_components(const topo::Tiles &g, volatile int32_t *lab, const int32_t *list,
                                                 const int *n_alive, int *changed, int &err) {
    const int tid = threadIdx.x;
    const int n = (int)g.n_tiles;
    for (int64_t round = 0; round <= n; ++round) {
        __syncthreads();                                     // labels of the last round (or the initial ones) are in place
        if (tid == 0) *changed = 0;
        __syncthreads();
        const int items = kInLds ? *n_alive : n;
        bool any = false;
        for (int w = tid; w < items; w += kThreads) any |= topo::lower_label(g, lab, kInLds ? list[w] : w, err);
        if (any) *changed = 1;
        __syncthreads();
        if (*changed == 0) break;                            // (uniform: read between two barriers)
    }
}

// ---------------------------------------------------------------------------------------------- host side of the entry points
// The argument checks the entry points have in common, in two parts: what an entry point does with an empty input and with its
// own outputs sits between them, and the order decides which error a bad call gets.  fn: the entry point, for the message.
#define TGNN_MASKS_CHECK(cond, msg)                                                \
    do {                                                                           \
        if (!(cond)) {                                                             \
            ::tgnn::set_error("%s: invalid argument: %s (%s)", fn, msg, #cond);    \
            return TGNN_ERR_INVALID_ARG;                                           \
        }                                                                          \
    } while (0)

// (dir_x, dir_y): the sweep direction; an entry point without one passes (1, 0)
static inline int check_mask_shape(const char *fn, int64_t n_tiles, int64_t n_masks, double tol, double dir_x, double dir_y) {
    TGNN_MASKS_CHECK(n_tiles >= 0 && n_tiles < (1ll << 31) - 1 && n_masks >= 0, "shape");
    TGNN_MASKS_CHECK(tol >= 0.0, "tol");                     // (false for a NaN too)
    TGNN_MASKS_CHECK(fabs(dir_x * dir_x + dir_y * dir_y - 1.0) <= 1e-9, "(dir_x, dir_y) is not a unit vector");
    return TGNN_OK;
}

// max_masks: the K beyond which K * n_tiles words overflow; tile_arrays: none of the arrays that may not be NULL is (col_idx /
// touch_idx may: no collision edge / no contact); ws_need: the entry point's own workspace size; ws_align: of its widest word.
static inline int check_mask_arrays(const char *fn, int64_t n_masks, int64_t max_masks, bool tile_arrays, const void *ws,
                                    size_t ws_bytes, size_t ws_need, size_t ws_align) {
    TGNN_MASKS_CHECK(n_masks <= max_masks, "K * n_tiles overflows");
    TGNN_MASKS_CHECK(tile_arrays, "null tile array");
    TGNN_MASKS_CHECK(ws && ws_bytes >= ws_need, "workspace too small");
    TGNN_MASKS_CHECK(reinterpret_cast<uintptr_t>(ws) % ws_align == 0, "workspace alignment");
    return TGNN_OK;
}
#undef TGNN_MASKS_CHECK

// launch(k0, count) for the masks k0 .. k0 + count, `step` (kMaskGridY or kMaskGridX) at a time.
template <class Launch>
static inline void for_mask_chunks(int64_t n_masks, int64_t step, Launch launch) {
    for (int64_t k0 = 0; k0 < n_masks; k0 += step) launch(k0, (unsigned)(n_masks - k0 < step ? n_masks - k0 : step));
}

}  // namespace tgnn
