// GINConv at width 32 (gin.hip): which of its three forms a call runs, how many blocks that form is launched with, and how the
// grid shares the 16-row tiles out over its waves (gin32_mlp_kernel, gin32_mlp16_kernel) or teams (gin32_fused_kernel), as plain
// C++17: no HIP header, testable on the CPU (tests/host/gin32_plan_test.cpp).
#pragma once
#include <stdint.h>

namespace tgnn {

// the three forms, also the `variant` of tgnn_gin32_fwd
enum Gin32Variant : int {
    kGin32Bf16x3 = 0,      // gin_aggregate_kernel<32> + gin32_mlp_kernel (every operand as three bf16 pieces)
    kGin32F16 = 1,         // gin_aggregate_kernel<32> + gin32_mlp16_kernel (layers 2 / 3 on fp16 pairs)
    kGin32Fused = 2,       // gin32_fused_kernel (one launch, the aggregate never leaves the chip)
};

constexpr int kGin32TileRows = 16;                          // rows of a tile: the N of v_mfma_f32_16x16x32_bf16
constexpr int kGin32BlockRows = 128;                        // rows per block every form's grid is sized by
constexpr int kGin32MaxPartials = 512;                      // TGNN_BN_MAX_PARTIALS: a block writes one BatchNorm partial row
constexpr int64_t kGinFusedMinNodes = 200000;               // tgnn_set_gin_fused(1): the fused form from this many nodes on
constexpr int kGin32ActLeakyRelu = 1;                       // TGNN_ACT_LEAKY_RELU

// rows whose byte offsets (128 per row) stay below 2^31: the fused kernel addresses rows with 32-bit buffer offsets
constexpr bool gin32_rows_addressable(int64_t n_nodes) { return n_nodes * 128 < (int64_t(1) << 31); }

// The form gin32_fwd_folded runs.  need_z: somebody reads the aggregate afterwards (the training forward); lda: floats between
// rows of the input; fused_mode: tgnn_set_gin_fused (0 never, 1 by size, 2 always); f16_switch: tgnn_set_gin_mlp_f16.
//   * fused: nobody needs z, packed rows, LeakyReLU, addressable rows, and the mode asks for it at this size;
//   * else fp16 pairs: nobody needs z (inference), LeakyReLU, the switch is on;
//   * else bf16 x 3.
constexpr Gin32Variant gin32_variant(bool need_z, int64_t lda, int act, int64_t n_nodes, int fused_mode, int f16_switch) {
    if (!need_z && lda == 32 && act == kGin32ActLeakyRelu && (fused_mode == 2 || (fused_mode == 1 && n_nodes >= kGinFusedMinNodes)) &&
        gin32_rows_addressable(n_nodes))
        return kGin32Fused;
    if (!need_z && act == kGin32ActLeakyRelu && f16_switch) return kGin32F16;
    return kGin32Bf16x3;
}

// Blocks of any of the three forms: one per 128 rows, at most `cap` (the CUs left to this chain, or the debug cap) and at most one
// per BatchNorm partial row; from 8 blocks on a multiple of 8, so that every XCD runs the same number (the swizzle below).
constexpr int gin32_blocks(int64_t n_nodes, int cap) {
    int64_t nb = (n_nodes + kGin32BlockRows - 1) / kGin32BlockRows;
    if (nb < 1) nb = 1;
    if (nb > kGin32MaxPartials) nb = kGin32MaxPartials;
    int blocks = (int)nb;
    if (blocks > cap) blocks = cap;
    if (blocks >= 8) blocks &= ~7;
    return blocks;
}

struct Gin32Tiles {
    int64_t t0, t1;                                         // tiles [t0, t1)
};

constexpr int64_t gin32_n_tiles(int64_t n) { return (n + kGin32TileRows - 1) / kGin32TileRows; }

// Grids of a multiple of 8 blocks: block b runs on XCD b & 7 -- the blocks of one XCD take a contiguous run of slots, so that the
// rows an XCD's L2 sees are contiguous.
constexpr int64_t gin32_swizzled_block(int nblk, int block) {
    return nblk >= 8 && (nblk & 7) == 0 ? (int64_t)(block & 7) * (nblk >> 3) + (block >> 3) : (int64_t)block;
}

// The share of SIMD slot `simd` (0 .. 3) of block `block`: what a team of the fused kernel walks, and what the waves simd and
// simd + 4 of the two-launch kernels split between them.  Balanced to one tile, contiguous in the order (swizzled block, simd).
constexpr Gin32Tiles gin32_slot_share(int64_t n, int nblk, int block, int simd) {
    const int64_t n_tiles = gin32_n_tiles(n);
    const int64_t slot = gin32_swizzled_block(nblk, block) * 4 + simd, n_slots = (int64_t)nblk * 4;
    return Gin32Tiles{n_tiles * slot / n_slots, n_tiles * (slot + 1) / n_slots};
}

// The share of wave `wave` (0 .. 7) of an 8-wave block: waves w and w + 4 run on SIMD w & 3 and split its slot's run in halves.
constexpr Gin32Tiles gin32_wave_share(int64_t n, int nblk, int block, int wave) {
    const Gin32Tiles q = gin32_slot_share(n, nblk, block, wave & 3);
    constexpr int kSubs = 2;
    const int sub = wave >> 2;
    return Gin32Tiles{q.t0 + (q.t1 - q.t0) * sub / kSubs, q.t0 + (q.t1 - q.t0) * (sub + 1) / kSubs};
}

}  // namespace tgnn
