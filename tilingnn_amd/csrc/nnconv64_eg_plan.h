// Limits of the width-64 fp32 NNConv on edge groups (nnconv64_eg.hip) and the predicate that sends a forward to it, as plain
// C++17: no HIP header, testable on the CPU (tests/host/nnconv64_eg_plan_test.cpp).
//
// LDS of a block: the fp16-pair weight image of ONE HALF of the output columns for every type and the root -- per entry
// [2 planes (hi, lo)][2 N blocks][2 K chunks][64 lanes] x 16 B = 8 KiB -- and the 16-entry selection table; behind the group
// stream the same memory holds the block's BatchNorm reduction.
#pragma once
#include <stddef.h>
#include <stdint.h>

namespace tgnn {

constexpr size_t kEg64MaxLds = 160 * 1024 - 256;           // (= kMaxLds64 of the bf16 sibling, bf16_path.hip)
constexpr int kEg64Waves = 8;                               // waves of a block: two per SIMD, 256 registers each
constexpr int kEg64HalfFloats = 2 * 2 * 2 * 64 * 4;         // floats of one entry's image for one half of the columns (8 KiB)
constexpr int kEg64TypeFloats = 2 * kEg64HalfFloats;        // floats of one entry's image (16 KiB)
// the edge-group structure counts the edges of a (row, type) and of a (tile, type) in 16 bits and is stated for in-degrees up to
// 2 048 (graph_prep.hip: nnconv_eg_kernel); the kernel itself has no limit (the mean is an fp32 reciprocal, not an fp16 operand)
constexpr int kEg64MaxInDegree = 2048;

constexpr size_t nnconv64_eg_lds_bytes(int n_types, int waves = kEg64Waves) {
    const size_t a = (size_t)(n_types + 1) * kEg64HalfFloats * sizeof(float) + 16 * 8;
    const size_t b = (size_t)waves * 64 * 8 * sizeof(double);          // BatchNorm reduction: 4 sums + 4 sums of squares per lane
    return a > b ? a : b;
}
constexpr int nnconv64_eg_max_types() {
    int t = 0;
    while (nnconv64_eg_lds_bytes(t + 1) <= kEg64MaxLds) ++t;
    return t;
}
static_assert(nnconv64_eg_max_types() == 18, "T <= 18: the limit of the bf16-storage path");

// tgnn_forward / tgnn_forward_train run their NNConv on nnconv64_eg_kernel iff this holds.  Train-mode BatchNorm only: a forward
// on running statistics (eval mode) stays on the generic kernel.
inline bool nnconv64_eg_ok(int c, bool sharded, bool has_groups, int64_t nr, int n_types, int max_in_degree, bool use_running_stats,
                           int switch_on) {
    return c == 64 && !sharded && has_groups && nr * 256 < (int64_t(1) << 31) && n_types >= 1 && n_types <= nnconv64_eg_max_types() &&
           max_in_degree >= 1 && max_in_degree <= kEg64MaxInDegree && !use_running_stats && switch_on != 0;
}

}  // namespace tgnn
