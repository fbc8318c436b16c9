// The NNConv adjoint on edge groups (nnconv_bwd_eg.hip: dh on the forward's edge-group kernels over the transposed graph, the weight
// gradients as per-type sums of 16-edge outer products on the exact-fp32 matrix instruction): the predicate, the grid of the dW kernel,
// a block's share of the type-major group list, the partial-slot layout and the workspace, as plain C++17: no HIP header, testable on
// the CPU (tests/host/nnconv_bwd_eg_plan_test.cpp).
#pragma once
#include <stddef.h>
#include <stdint.h>

#include "nnconv64_eg_plan.h"

namespace tgnn {

constexpr int kBwdEgMaxTypes32 = 22;                        // width 32: tgnn_nnconv_cols_max_types(), what the group structure is built for
constexpr int kBwdEgMaxDegree = 2048;                       // the stated range of the group structure, in- and out-degree alike
constexpr int kBwdEgDwWaves = 4;                            // the dW block: one wave per SIMD, every wave holds a whole C x C tile
constexpr int kBwdEgDwThreads = kBwdEgDwWaves * 64;
constexpr int kBwdEgDwMaxBlocks = 512;                      // two blocks per CU of the largest part
constexpr int kBwdEgDwGroupsPerWave = 4;                    // below this a wave's share is not worth a block of its own
constexpr int kBwdEgListHeader = 64;                        // ints in front of the type-major list: offsets of types 0 .. T + 1
constexpr int kBwdEgImageFloats32 = 2 * 2 * 64 * 4;         // one entry's fp16-pair weight image at width 32 (= kWtTypeF16)

constexpr int nnconv_bwd_eg_max_types(int c) { return c == 64 ? nnconv64_eg_max_types() : c == 32 ? kBwdEgMaxTypes32 : 0; }

// tgnn_backward takes the edge-group adjoint iff this holds (and its switch is on); the op refuses everything else
constexpr bool nnconv_bwd_eg_ok(int c, int64_t n, int n_types, int max_in_degree, int max_out_degree, bool has_fwd_groups,
                                bool has_bwd_groups) {
    return (c == 32 || c == 64) && n >= 1 && n_types >= 1 && n_types <= nnconv_bwd_eg_max_types(c) && max_in_degree >= 1 &&
           max_in_degree <= kBwdEgMaxDegree && max_out_degree >= 1 && max_out_degree <= kBwdEgMaxDegree &&
           n * c * 4 < (int64_t(1) << 31) && has_fwd_groups && has_bwd_groups;
}
// which limit fails, as the error message names it (NULL: the predicate holds)
constexpr const char *nnconv_bwd_eg_why_not(int c, int64_t n, int n_types, int max_in_degree, int max_out_degree, bool has_fwd_groups,
                                            bool has_bwd_groups) {
    return (c != 32 && c != 64)                                         ? "network width must be 32 or 64"
           : n < 1                                                      ? "no rows"
           : (n_types < 1 || n_types > nnconv_bwd_eg_max_types(c))      ? (c == 64 ? "edge types must lie in 1 .. 18 at width 64 (LDS weight image)"
                                                                                   : "edge types must lie in 1 .. 22 at width 32 (edge-group structure)")
           : (max_in_degree < 1 || max_in_degree > kBwdEgMaxDegree)     ? "largest in-degree must lie in 1 .. 2048"
           : (max_out_degree < 1 || max_out_degree > kBwdEgMaxDegree)   ? "largest out-degree must lie in 1 .. 2048"
           : n * c * 4 >= (int64_t(1) << 31)                            ? "rows must lie within 2 GB"
           : !has_fwd_groups                                            ? "forward edge groups missing"
           : !has_bwd_groups                                            ? "transposed edge groups missing"
                                                                        : nullptr;
}

// ---- the dW kernel.  The type-major list holds the forward structure's groups sorted by type (stable: by group index), the root
// groups as type T behind them: L entries.  A block takes a contiguous share; per type it meets it sums into one partial slot.
constexpr int nnconv_bwd_eg_dw_blocks(int64_t n_list, int cap = kBwdEgDwMaxBlocks) {
    const int64_t per = (int64_t)kBwdEgDwWaves * kBwdEgDwGroupsPerWave;
    const int64_t b = (n_list + per - 1) / per;
    const int64_t c = cap < 1 ? 1 : (cap > kBwdEgDwMaxBlocks ? kBwdEgDwMaxBlocks : cap);
    return (int)(b < 1 ? 1 : (b > c ? c : b));
}
struct BwdEgShare {
    int64_t begin, end;
};
constexpr BwdEgShare nnconv_bwd_eg_dw_share(int64_t n_list, int nblk, int block) {
    return BwdEgShare{n_list * block / nblk, n_list * (block + 1) / nblk};
}
// The slot block `block` stores its sum over type `type` in.  Shares are contiguous in a type-sorted list, so the last type of a block
// is at most the first type of the next one: block + type is strictly increasing along (block, type) and below nblk + T + 1.
constexpr int nnconv_bwd_eg_dw_slot(int block, int type) { return block + type; }
constexpr int nnconv_bwd_eg_dw_slots(int n_types) { return kBwdEgDwMaxBlocks + n_types + 1; }

// the op's workspace: [bounds 256 B | transposed table (T+1) C C | its fp16-pair image | partial slots]
constexpr size_t nnconv_bwd_eg_up256(size_t v) { return (v + 255) / 256 * 256; }
constexpr size_t nnconv_bwd_eg_image_floats(int n_types, int c) {
    return (size_t)(n_types + 1) * (c == 64 ? (size_t)kEg64TypeFloats : (size_t)kBwdEgImageFloats32);
}
struct BwdEgWorkspace {
    size_t bounds, wt, wimg, slots, total;
};
constexpr BwdEgWorkspace nnconv_bwd_eg_workspace(int n_types, int c) {
    BwdEgWorkspace w{};
    w.bounds = 0;
    w.wt = 256;
    w.wimg = w.wt + nnconv_bwd_eg_up256((size_t)(n_types + 1) * c * c * sizeof(float));
    w.slots = w.wimg + nnconv_bwd_eg_up256(nnconv_bwd_eg_image_floats(n_types, c) * sizeof(float));
    w.total = w.slots + nnconv_bwd_eg_up256((size_t)nnconv_bwd_eg_dw_slots(n_types) * c * c * sizeof(float));
    return w;
}
// bytes tgnn_nnconv_bwd_eg wants; 0 where no layout of this size can hold the predicate.  n_groups_cap: the capacity of the forward
// structure (tgnn_nnconv_eg_max_groups) -- the list lives with the layout, not here; it only has to be addressable
constexpr size_t nnconv_bwd_eg_workspace_bytes(int64_t n, int64_t n_groups_cap, int n_types, int c) {
    if (!nnconv_bwd_eg_ok(c, n, n_types, 1, 1, true, true) || n_groups_cap < 0 || n_groups_cap >= (int64_t(1) << 27)) return 0;
    return nnconv_bwd_eg_workspace(n_types, c).total;
}
// ints of the type-major list of a structure of n_groups_cap groups
constexpr size_t nnconv_bwd_eg_list_ints(int64_t n_groups_cap) { return (size_t)kBwdEgListHeader + 2 * (size_t)(n_groups_cap > 0 ? n_groups_cap : 0); }

}  // namespace tgnn
