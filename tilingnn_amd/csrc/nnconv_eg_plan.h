// NNConv on edge groups at width 32 (nnconv_eg.hip): how many blocks a launch gets, how the grid shares the 16-row tiles out over
// its waves, and the register footprint every kernel of the layer loop is pinned to, as plain C++17: no HIP header, testable on
// the CPU (tests/host/nnconv_eg_plan_test.cpp).
#pragma once
#include <stdint.h>

namespace tgnn {

constexpr int kEgTileRows = 16;                             // rows of a tile: the M of the matrix instructions
constexpr int kEgSimds = 4;                                 // SIMDs of a CU: waves w, w + 4, w + 8, .. of a block run on SIMD w & 3
constexpr int kEgTilesPerBlock = 4;                         // one tile per SIMD before a second block gets one
constexpr int kEgMaxBlocks = 1024;                          // (the 32-bit share arithmetic below: 4 096 slots, products below 2^24)

constexpr uint32_t nnconv_eg_n_tiles(int64_t n_nodes) { return (uint32_t)((n_nodes + kEgTileRows - 1) / kEgTileRows); }

// Blocks of a launch: one per four tiles, at most `cap` (the CUs left to this chain, or the debug cap); from 8 blocks on a
// multiple of 8, so that every XCD runs the same number (the swizzle below).
constexpr int nnconv_eg_blocks(int64_t n_nodes, int64_t cap) {
    const int64_t n_tiles = (n_nodes + kEgTileRows - 1) / kEgTileRows;
    int64_t blocks = (n_tiles + kEgTilesPerBlock - 1) / kEgTilesPerBlock;
    if (blocks > cap) blocks = cap;
    if (blocks > kEgMaxBlocks) blocks = kEgMaxBlocks;
    if (blocks >= 8) blocks &= ~int64_t(7);
    if (blocks < 1) blocks = 1;
    return (int)blocks;
}

struct EgTiles {
    uint32_t t0, t1;                                        // tiles [t0, t1)
};

// Grids of a multiple of 8 blocks: block b runs on XCD b & 7 -- the blocks of one XCD take a contiguous run of slots, so that the
// rows an XCD's L2 sees are contiguous.
constexpr uint32_t nnconv_eg_swizzled_block(uint32_t nblk, uint32_t block) {
    return nblk >= 8 && (nblk & 7) == 0 ? (block & 7) * (nblk >> 3) + (block >> 3) : block;
}

// The share of SIMD slot `simd` (0 .. 3) of block `block`: balanced to one tile, contiguous in the order (swizzled block, simd).
// (32-bit arithmetic: a 64-bit division is ~150 instructions and the kernel's prologue is a fifth of a wave's vector work;
//  n_tiles * slot / n_slots without the wide product.)
constexpr EgTiles nnconv_eg_slot_share(uint32_t n_tiles, uint32_t nblk, uint32_t block, uint32_t simd) {
    const uint32_t slot = nnconv_eg_swizzled_block(nblk, block) * kEgSimds + simd, n_slots = nblk * kEgSimds;
    const uint32_t tq = n_tiles / n_slots, tr = n_tiles % n_slots;
    return EgTiles{tq * slot + tr * slot / n_slots, tq * (slot + 1) + tr * (slot + 1) / n_slots};
}

// The share of wave `wave` of a block of `waves` waves (a multiple of 4): the waves/4 waves of a SIMD split its slot's run into
// contiguous parts, balanced to one tile.  Empty where a slot holds fewer tiles than waves.
constexpr EgTiles nnconv_eg_wave_share(uint32_t n_tiles, uint32_t nblk, uint32_t block, uint32_t wave, uint32_t waves) {
    const EgTiles q = nnconv_eg_slot_share(n_tiles, nblk, block, wave & (kEgSimds - 1));
    const uint32_t subs = waves / kEgSimds, sub = wave / kEgSimds;
    return EgTiles{q.t0 + (q.t1 - q.t0) * sub / subs, q.t0 + (q.t1 - q.t0) * (sub + 1) / subs};
}

// ---- the register footprint of the four kernels of a layer of the general schedule (forward.hip).  A SIMD has 512 vector
// registers per lane; a wave is allocated its kernel's count rounded up to 8.  `vgpr_cap` is what __launch_bounds__ pins the
// kernel to (the compiler may use fewer, never more); waves_per_simd is what ONE block puts on a SIMD.  Two kernels can be
// resident on one CU together when the sum of waves_per_simd x allocated registers of one block each is at most 512 (and their
// LDS fits 160 KB): tests/test_nnconv_eg_footprint.py checks the counts the runtime reports against this table.
enum LayerKernel : int {
    kLayerNnconvEg = 0,                                     // nnconv32_eg_kernel, LeakyReLU, the general forward's instantiation
    kLayerGinAggregate = 1,                                 // gin_aggregate_kernel<32>
    kLayerGinMlp = 2,                                       // gin32_mlp_kernel
    kLayerMerge = 3,                                        // merge_bn1_wide_kernel
    kLayerKernels = 4,
};

struct KernelFootprint {
    int waves_per_block, waves_per_simd, vgpr_cap;
};

constexpr int kSimdVgprs = 512, kCuLdsBytes = 160 * 1024;

// As built (gfx950): 125, 60, 230 and 120 registers.  The NNConv (4 x 128) and the aggregate (8 x 64 at full occupancy) fill a
// SIMD on their own; a 12-wave NNConv that leaves room for the aggregate was measured and is not faster (build switch
// TGNN_ABL_EGW12).  The dense pair is shaped to share a CU: one 4-wave block of the GIN MLP beside one 8-wave block of the merge
// (profiles/coresident_stage0.txt, profiles/coresident_ab.txt).
constexpr KernelFootprint kLayerFootprints[kLayerKernels] = {
    {16, 4, 128},                                           // nnconv32_eg_kernel<16, 4>: __launch_bounds__(1024, 4)
    {4, 1, 512},                                            // gin_aggregate_kernel<32>: __launch_bounds__(256), not pinned further
    {4, 1, 256},                                            // gin32_mlp_kernel<4>: __launch_bounds__(256, 2)
    {8, 2, 128},                                            // merge_bn1_wide_kernel<512>: __launch_bounds__(512, 4)
};

// one block of `a` beside one block of `b` on a CU: what the general schedule relies on
struct CoResidentPair {
    LayerKernel a, b;
};
constexpr CoResidentPair kCoResidentPairs[] = {{kLayerGinMlp, kLayerMerge}};

// VGPRs a wave is allocated for a kernel that uses `vgprs` of them
constexpr int vgprs_allocated(int vgprs) { return (vgprs + 7) / 8 * 8; }

}  // namespace tgnn
