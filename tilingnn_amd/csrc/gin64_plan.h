// The width-64 fp32 GIN MLP on the matrix cores (gin64_mlp.hip): how its grid shares the 16-row tiles out over its waves, and the
// predicate that sends a forward to it, as plain C++17: no HIP header, testable on the CPU (tests/host/gin64_plan_test.cpp).
#pragma once
#include <stdint.h>

namespace tgnn {

constexpr int kGin64Waves = 8;                             // waves of a block: two per SIMD
constexpr int kGin64Threads = kGin64Waves * 64;
constexpr int kGin64TileRows = 16;                         // rows of a tile: the N of v_mfma_f32_16x16x32_bf16
constexpr int kGin64BlockRows = kGin64TileRows * kGin64Waves;   // rows per block the grid is sized by

struct Gin64Tiles {
    int64_t t0, t1;                                        // this wave walks tiles [t0, t1)
};

constexpr int64_t gin64_n_tiles(int64_t n) { return (n + kGin64TileRows - 1) / kGin64TileRows; }

// The tile share of wave `wave` of block `block` in a grid of `nblk` blocks, as gin32_mlp_kernel shares its tiles out:
//   * grids of a multiple of 8 blocks: block b runs on XCD b & 7 -- the blocks of one XCD take a contiguous run of slots, so that
//     the rows an XCD's L2 sees are contiguous;
//   * waves w and w + 4 of a block run on SIMD w: the four SIMD slots of a block take contiguous, balanced runs of tiles, and the
//     two waves of a SIMD split their slot's run in halves.
// Every tile of [0, gin64_n_tiles(n)) belongs to exactly one wave; walked in the order (slot, sub) the ranges are contiguous.
constexpr Gin64Tiles gin64_tile_share(int64_t n, int nblk, int block, int wave) {
    const int64_t n_tiles = gin64_n_tiles(n);
    int64_t blk = block;
    if (nblk >= 8 && (nblk & 7) == 0) blk = (int64_t)(block & 7) * (nblk >> 3) + (block >> 3);
    const int64_t slot = blk * 4 + (wave & 3), n_slots = (int64_t)nblk * 4;
    const int64_t q0 = n_tiles * slot / n_slots, q1 = n_tiles * (slot + 1) / n_slots;
    constexpr int kSubs = kGin64Waves / 4;
    const int sub = wave >> 2;
    return Gin64Tiles{q0 + (q1 - q0) * sub / kSubs, q0 + (q1 - q0) * (sub + 1) / kSubs};
}

// tgnn_forward / tgnn_forward_train run their collision branch's MLP on gin64_mlp_kernel iff this holds.  It does not ask for the
// BatchNorm mode: the kernel needs no bound of its operand, so a forward on running statistics takes it too.
inline bool gin64_mfma_ok(int c, bool sharded, int switch_on) { return c == 64 && !sharded && switch_on == 1; }

}  // namespace tgnn
