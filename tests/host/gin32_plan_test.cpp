// Stand-alone check of the width-32 GINConv's plan (tilingnn_amd/csrc/gin32_plan.h): the tile share of the waves of
// gin32_mlp_kernel / gin32_mlp16_kernel and of the teams of gin32_fused_kernel, the block count, and the choice between the three
// forms against a table written out by hand.  No device, no HIP header:
//   g++ -std=c++17 -O1 -fsanitize=address,undefined -I include -I tilingnn_amd/csrc tests/host/gin32_plan_test.cpp
// (tests/test_gin32_plan_host.py builds and runs it).
#include <stdio.h>

#include <initializer_list>
#include <vector>

#include "gin32_plan.h"
#include "tgnn.h"

using namespace tgnn;

static long g_failures = 0;
#define EXPECT(cond)                                                              \
    do {                                                                          \
        if (!(cond) && ++g_failures <= 20) fprintf(stderr, "FAILED: %s (line %d)\n", #cond, __LINE__); \
    } while (0)

// the order the shares are contiguous in, written out once more: the XCD remap of the block, then the SIMD
static int64_t slot_rank(int nblk, int block, int simd) {
    int64_t blk = block;
    if (nblk >= 8 && nblk % 8 == 0) blk = (int64_t)(block % 8) * (nblk / 8) + block / 8;
    return blk * 4 + simd;
}

// every tile of [0, n_tiles) in exactly one share; the shares, in rank order, contiguous from 0 to n_tiles
static void check_cover(const std::vector<Gin32Tiles> &by_rank, int64_t n_tiles, int64_t max_spread) {
    std::vector<unsigned char> owners((size_t)n_tiles, 0);
    int64_t at = 0, longest = 0, shortest = n_tiles;
    for (const Gin32Tiles &t : by_rank) {
        EXPECT(0 <= t.t0 && t.t0 <= t.t1 && t.t1 <= n_tiles);
        EXPECT(t.t0 == at);
        at = t.t1;
        for (int64_t k = t.t0; k < t.t1 && k < n_tiles; ++k)
            if (k >= 0 && owners[(size_t)k] < 255) ++owners[(size_t)k];
        longest = t.t1 - t.t0 > longest ? t.t1 - t.t0 : longest;
        shortest = t.t1 - t.t0 < shortest ? t.t1 - t.t0 : shortest;
    }
    EXPECT(at == n_tiles);
    for (int64_t k = 0; k < n_tiles; ++k) EXPECT(owners[(size_t)k] == 1);
    EXPECT(longest - shortest <= max_spread);
}

struct Choice {
    bool need_z;
    int64_t lda;
    int act;
    int64_t n;
    int fused_mode, f16;
    Gin32Variant want;
};

int main() {
    static_assert(kGin32TileRows == 16 && kGin32BlockRows == 128, "the kernels' shape");
    static_assert(kGin32MaxPartials == TGNN_BN_MAX_PARTIALS && kGin32ActLeakyRelu == TGNN_ACT_LEAKY_RELU, "restated constants");
    static_assert(gin32_wave_share(17, 1, 0, 0).t0 == 0, "usable in constant expressions");

    // ---- tile shares
    long shares = 0;
    for (int64_t n : {int64_t(1), int64_t(15), int64_t(16), int64_t(17), int64_t(128), int64_t(129), int64_t(897), int64_t(1254),
                      int64_t(28672), int64_t(28673), int64_t(66003), int64_t(100000), int64_t(200003)})
        for (int nblk : {1, 2, 7, 8, 16, 24, 224}) {
            const int64_t n_tiles = (n + 15) / 16;
            EXPECT(gin32_n_tiles(n) == n_tiles);
            std::vector<Gin32Tiles> slots((size_t)nblk * 4, Gin32Tiles{-1, -1}), waves((size_t)nblk * 8, Gin32Tiles{-1, -1});
            for (int b = 0; b < nblk; ++b) {
                EXPECT(gin32_swizzled_block(nblk, b) == slot_rank(nblk, b, 0) / 4);
                for (int simd = 0; simd < 4; ++simd) {
                    const int64_t r = slot_rank(nblk, b, simd);
                    EXPECT(r >= 0 && r < (int64_t)slots.size() && slots[(size_t)r].t0 == -1);      // the remap is a permutation
                    const Gin32Tiles q = gin32_slot_share(n, nblk, b, simd);
                    if (r >= 0 && r < (int64_t)slots.size()) slots[(size_t)r] = q;
                    ++shares;
                    // the two waves of the SIMD split exactly the slot's run
                    const Gin32Tiles lo = gin32_wave_share(n, nblk, b, simd), hi = gin32_wave_share(n, nblk, b, simd + 4);
                    EXPECT(lo.t0 == q.t0 && lo.t1 == hi.t0 && hi.t1 == q.t1);
                    EXPECT((hi.t1 - hi.t0) - (lo.t1 - lo.t0) >= 0 && (hi.t1 - hi.t0) - (lo.t1 - lo.t0) <= 1);
                    if (r >= 0 && r < (int64_t)slots.size()) {
                        waves[(size_t)r * 2] = lo;
                        waves[(size_t)r * 2 + 1] = hi;
                    }
                    shares += 2;
                }
            }
            check_cover(slots, n_tiles, 1);                  // teams of the fused kernel: balanced to one tile
            check_cover(waves, n_tiles, 2);                  // waves: their halves to one more
        }
    // the fused kernel's hand-over ring (6 slots per team) wraps once a team holds more than 6 tiles: where the cases stand
    {
        auto longest_team = [](int64_t n, int nblk) {
            int64_t m = 0;
            for (int b = 0; b < nblk; ++b)
                for (int simd = 0; simd < 4; ++simd) {
                    const Gin32Tiles q = gin32_slot_share(n, nblk, b, simd);
                    m = q.t1 - q.t0 > m ? q.t1 - q.t0 : m;
                }
            return m;
        };
        EXPECT(longest_team(66003, 224) == 5);               // no wrap
        EXPECT(longest_team(100000, 224) == 7);              // wraps by one tile
        EXPECT(longest_team(200003, 224) == 14);             // every slot reused twice
    }

    // ---- block count
    EXPECT(gin32_blocks(1, 224) == 1 && gin32_blocks(128, 224) == 1 && gin32_blocks(129, 224) == 2);
    EXPECT(gin32_blocks(200, 224) == 2 && gin32_blocks(800, 224) == 7 && gin32_blocks(896, 224) == 7 && gin32_blocks(897, 224) == 8);
    EXPECT(gin32_blocks(1000, 224) == 8 && gin32_blocks(1254, 224) == 8);                     // 10 blocks -> a multiple of 8
    EXPECT(gin32_blocks(2000, 224) == 16 && gin32_blocks(3000, 224) == 24);
    EXPECT(gin32_blocks(28672, 224) == 224 && gin32_blocks(30000, 224) == 224 && gin32_blocks(200003, 224) == 224);
    EXPECT(gin32_blocks(30000, 7) == 7 && gin32_blocks(30000, 12) == 8 && gin32_blocks(30000, 1) == 1);
    EXPECT(gin32_blocks(1 << 24, 1 << 20) == 512);                                            // one partial row per block at most
    EXPECT(gin32_blocks(0, 224) == 1);

    // ---- the choice between the three forms, by hand
    const int L = TGNN_ACT_LEAKY_RELU, N = TGNN_ACT_NONE;
    const Choice table[] = {
        // need_z  lda  act  n        fused f16  -> form
        {false, 32, L, 1000, 1, 0, kGin32Bf16x3},            // the default below 200 000 nodes
        {false, 32, L, 199999, 1, 0, kGin32Bf16x3},
        {false, 32, L, 200000, 1, 0, kGin32Fused},           // the default from 200 000 nodes on
        {false, 32, L, 200003, 1, 0, kGin32Fused},
        {false, 32, L, 200003, 0, 0, kGin32Bf16x3},          // fused switched off
        {false, 32, L, 200003, 0, 1, kGin32F16},
        {false, 32, L, 17, 2, 0, kGin32Fused},               // fused at every size
        {false, 32, L, 17, 2, 1, kGin32Fused},               // ... which wins over the fp16 switch
        {false, 32, L, 1000, 1, 1, kGin32F16},               // the fp16 switch below the fused threshold
        {false, 32, L, 200000, 1, 1, kGin32Fused},
        {true, 32, L, 200003, 2, 1, kGin32Bf16x3},           // the training forward keeps z: always bf16 x 3
        {true, 32, L, 1000, 1, 1, kGin32Bf16x3},
        {false, 36, L, 200003, 2, 0, kGin32Bf16x3},          // strided rows: never fused
        {false, 36, L, 1000, 1, 1, kGin32F16},               // (the aggregate packs them: the fp16 MLP may follow)
        {false, 32, N, 200003, 2, 1, kGin32Bf16x3},          // no LeakyReLU: neither
        {false, 32, N, 1000, 0, 1, kGin32Bf16x3},
        {false, 32, L, (int64_t(1) << 24) - 1, 2, 0, kGin32Fused},     // the last row count with 32-bit byte offsets
        {false, 32, L, int64_t(1) << 24, 2, 0, kGin32Bf16x3},
        {false, 32, L, int64_t(1) << 24, 2, 1, kGin32F16},
    };
    long choices = 0;
    for (const Choice &c : table) {
        EXPECT(gin32_variant(c.need_z, c.lda, c.act, c.n, c.fused_mode, c.f16) == c.want);
        ++choices;
    }
    EXPECT(gin32_rows_addressable((int64_t(1) << 24) - 1) && !gin32_rows_addressable(int64_t(1) << 24));
    printf("gin32_plan_test: %ld tile shares, %ld choices, %ld failures\n", shares, choices, g_failures);
    return g_failures ? 1 : 0;
}
