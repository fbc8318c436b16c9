// The fused adjoint of GINConv's MLP at width 64 (mlp_bwd.hip: mlp_bwd_tall64_kernel + mlp_bwd_fold64_kernel): the predicate, the
// grid, the tile share of a wave, the partial-row layout and the workspace, as plain C++17: no HIP header, testable on the CPU
// (tests/host/mlp_bwd64_plan_test.cpp).  A form of its own beside mlp_bwd_plan.h's two: mlp_bwd_form keeps answering 0 for this shape,
// and the kernel has its own entry (tgnn_sigmoid_mlp_bwd_tall64) and its own switch (tgnn_set_mlp_bwd_tall64).
#pragma once
#include <stddef.h>
#include <stdint.h>

#include "mlp_bwd_plan.h"

namespace tgnn {

constexpr int kMlpBwd64Waves = 4;                          // the block: ONE wave per SIMD -- the wave then has the unified 512-entry file
constexpr int kMlpBwd64Threads = kMlpBwd64Waves * 64;
// one partial row of a block / the fold's elements: [dW1 32x64 | db1 32 | dW2 64x32 | db2 64 | dW3 64x64 | db3 64]
constexpr int kMlpBwd64OffW1 = 0, kMlpBwd64OffB1 = 2048, kMlpBwd64OffW2 = 2080, kMlpBwd64OffB2 = 4128, kMlpBwd64OffW3 = 4192,
              kMlpBwd64OffB3 = 8288, kMlpBwd64RowFloats = 8352;

// (d0, d1, d2, d3) = (64, 32, 64, 64) exactly, any number of rows.  No row floor: the kernel is taken from one row on (DESIGN
// section 31 has the times at 1 254 rows).
constexpr bool mlp_bwd_tall64_ok(int64_t n_rows, int d0, int d1, int d2, int d3) {
    return n_rows >= 0 && d0 == 64 && d1 == 32 && d2 == 64 && d3 == 64;
}

// Blocks = partial rows the fold kernel reads: one tile per wave (= per SIMD) until the grid is one block per CU of the largest part,
// then the waves walk contiguous runs of tiles.
constexpr int mlp_bwd_tall64_blocks(int64_t n_rows) {
    const int64_t b = (gin64_n_tiles(n_rows) + kMlpBwd64Waves - 1) / kMlpBwd64Waves;
    return b < 1 ? 1 : (b > kMlpBwdMaxBlocks ? kMlpBwdMaxBlocks : (int)b);
}

// The tiles of wave `wave` of block `block` in a grid of `nblk` blocks: gin64_tile_share's order of the slots (grids of a multiple of
// 8 blocks: block b runs on XCD b & 7, and the blocks of one XCD take a contiguous run), one wave per slot.  Every tile of
// [0, gin64_n_tiles(n)) belongs to exactly one wave.
constexpr Gin64Tiles mlp_bwd_tall64_tile_share(int64_t n, int nblk, int block, int wave) {
    const int64_t n_tiles = gin64_n_tiles(n);
    int64_t blk = block;
    if (nblk >= 8 && (nblk & 7) == 0) blk = (int64_t)(block & 7) * (nblk >> 3) + (block >> 3);
    const int64_t slot = blk * kMlpBwd64Waves + wave, n_slots = (int64_t)nblk * kMlpBwd64Waves;
    return Gin64Tiles{n_tiles * slot / n_slots, n_tiles * (slot + 1) / n_slots};
}

// bytes of workspace tgnn_sigmoid_mlp_bwd_tall64 wants (0: the predicate refuses the shape)
constexpr size_t mlp_bwd_tall64_workspace_bytes(int64_t n_rows, int d0, int d1, int d2, int d3) {
    if (!mlp_bwd_tall64_ok(n_rows, d0, d1, d2, d3)) return 0;
    return ((size_t)mlp_bwd_tall64_blocks(n_rows) * kMlpBwd64RowFloats * sizeof(float) + 255) / 256 * 256;
}

}  // namespace tgnn
