// The fused adjoints of the 3-layer sigmoid MLP (mlp_bwd.hip): which form a call takes, the grid and tile share of the tall form and
// what both forms need of the workspace, as plain C++17: no HIP header, testable on the CPU (tests/host/mlp_bwd_plan_test.cpp).
//   tall (1): GINConv's MLP at width 32, (d0, d1, d2, d3) = (32, 32, 64, 32), any number of rows -- one persistent kernel of 16-row
//             tiles + one fold kernel over the blocks' partial rows;
//   wide (2): GraphConv's edge MLP, (fe, 32, 64, C C) on the T <= 63 distinct attribute rows, no input gradient -- one launch over
//             chunks of 64 output columns of layer 3, one 1-block launch for layers 2 and 1.
#pragma once
#include <stddef.h>
#include <stdint.h>

#include "gin64_plan.h"

namespace tgnn {

constexpr int kMlpBwdWaves = kGin64Waves;                  // the tall kernel's block: 8 waves, two per SIMD
constexpr int kMlpBwdThreads = kMlpBwdWaves * 64;
constexpr int kMlpBwdTileRows = kGin64TileRows;            // rows of a tile: the N of v_mfma_f32_16x16x4_f32
constexpr int kMlpBwdMaxBlocks = 256;                      // one block per CU of the largest part
// one partial row of a tall block / the fold's elements: [dW1 32x32 | db1 32 | dW2 64x32 | db2 64 | dW3 32x64 | db3 32]
constexpr int kMlpBwdOffW1 = 0, kMlpBwdOffB1 = 1024, kMlpBwdOffW2 = 1056, kMlpBwdOffB2 = 3104, kMlpBwdOffW3 = 3168,
              kMlpBwdOffB3 = 5216, kMlpBwdRowFloats = 5248;
constexpr int kMlpBwdWideChunk = 64;                       // output columns of layer 3 per block of the wide form's first launch
constexpr int kMlpBwdWideMaxRows = 63, kMlpBwdWideMaxIn = 64, kMlpBwdWideMaxOut = 65536;

// 0: not taken, 1: tall, 2: wide.  No row floor: both forms are taken from one row on (DESIGN section 30 has the times).
constexpr int mlp_bwd_form(int64_t n_rows, int d0, int d1, int d2, int d3, int want_dx) {
    if (n_rows < 0 || d1 != 32 || d2 != 64) return 0;
    if (d0 == 32 && d3 == 32) return 1;
    if (!want_dx && n_rows <= kMlpBwdWideMaxRows && d0 >= 1 && d0 <= kMlpBwdWideMaxIn && d3 >= kMlpBwdWideChunk &&
        d3 <= kMlpBwdWideMaxOut && d3 % kMlpBwdWideChunk == 0)
        return 2;
    return 0;
}

// Blocks of the tall kernel = partial rows the fold kernel reads.  Up to 16 384 rows a block gets four tiles, one per SIMD (a wave
// works alone on its SIMD: gin64_tile_share hands the tile of a slot to the slot's second wave): a 1 254-row call is 20 blocks, not
// the 10 that eight tiles per block would give, and a tile is then never queued behind another on its SIMD.  Beyond that the grid
// is one block per CU and the waves walk contiguous runs of tiles.
constexpr int mlp_bwd_tall_blocks(int64_t n_rows) {
    const int64_t b = (gin64_n_tiles(n_rows) + 3) / 4;
    return b < 1 ? 1 : (b > kMlpBwdMaxBlocks ? kMlpBwdMaxBlocks : (int)b);
}
constexpr Gin64Tiles mlp_bwd_tile_share(int64_t n, int nblk, int block, int wave) { return gin64_tile_share(n, nblk, block, wave); }

constexpr int mlp_bwd_wide_chunks(int d3) { return d3 / kMlpBwdWideChunk; }

// bytes of workspace tgnn_sigmoid_mlp_bwd_fused wants (0: the form predicate refuses the shape)
constexpr size_t mlp_bwd_fused_workspace_bytes(int64_t n_rows, int d0, int d1, int d2, int d3) {
    const int form = mlp_bwd_form(n_rows, d0, d1, d2, d3, 0);
    if (form == 1) return ((size_t)mlp_bwd_tall_blocks(n_rows) * kMlpBwdRowFloats * sizeof(float) + 255) / 256 * 256;
    if (form == 2)
        return ((size_t)mlp_bwd_wide_chunks(d3) * (size_t)(n_rows > 0 ? n_rows : 1) * 64 * sizeof(float) + 255) / 256 * 256;
    return 0;
}

}  // namespace tgnn
