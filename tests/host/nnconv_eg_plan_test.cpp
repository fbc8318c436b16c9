// Stand-alone check of the edge-group NNConv's plan (tilingnn_amd/csrc/nnconv_eg_plan.h): the tile share of every wave of
// nnconv32_eg_kernel for blocks of 8, 12 and 16 waves, the block count, and the footprint table's arithmetic.  No device, no HIP
// header:
//   g++ -std=c++17 -O1 -fsanitize=address,undefined -I include -I tilingnn_amd/csrc tests/host/nnconv_eg_plan_test.cpp
// (tests/test_nnconv_eg_plan_host.py builds and runs it).
#include <stdio.h>

#include <initializer_list>
#include <vector>

#include "nnconv_eg_plan.h"

using namespace tgnn;

static long g_failures = 0;
#define EXPECT(cond)                                                              \
    do {                                                                          \
        if (!(cond) && ++g_failures <= 20) fprintf(stderr, "FAILED: %s (line %d)\n", #cond, __LINE__); \
    } while (0)

// the order the shares are contiguous in, written out once more: the XCD remap of the block, then the SIMD, then the waves of
// that SIMD (wave = simd + 4 sub)
static int64_t wave_rank(int nblk, int block, int wave, int waves) {
    int64_t blk = block;
    if (nblk >= 8 && nblk % 8 == 0) blk = (int64_t)(block % 8) * (nblk / 8) + block / 8;
    const int subs = waves / 4;
    return (blk * 4 + wave % 4) * subs + wave / 4;
}

int main() {
    static_assert(kEgTileRows == 16 && kEgSimds == 4 && kEgTilesPerBlock == 4, "the kernel's shape");
    static_assert(nnconv_eg_wave_share(7, 1, 0, 0, 12).t0 == 0, "usable in constant expressions");
    static_assert(nnconv_eg_n_tiles(1) == 1 && nnconv_eg_n_tiles(16) == 1 && nnconv_eg_n_tiles(17) == 2 && nnconv_eg_n_tiles(100000) == 6250, "tiles");

    long shares = 0, empty = 0;
    std::vector<int> n_tiles_list;
    for (int t = 1; t <= 300; ++t) n_tiles_list.push_back(t);
    n_tiles_list.push_back(6250);
    for (int waves : {8, 12, 16})
        for (int nblk : {1, 7, 8, 9, 64, 224, 256})
            for (int n_tiles : n_tiles_list) {
                const int subs = waves / 4;
                std::vector<EgTiles> by_rank((size_t)nblk * waves, EgTiles{~0u, ~0u});
                std::vector<unsigned char> seen((size_t)nblk * waves, 0), owners((size_t)n_tiles, 0);
                for (int b = 0; b < nblk; ++b) {
                    EXPECT(nnconv_eg_swizzled_block((uint32_t)nblk, (uint32_t)b) == (uint32_t)(wave_rank(nblk, b, 0, waves) / (4 * subs)));
                    for (int w = 0; w < waves; ++w) {
                        const int64_t r = wave_rank(nblk, b, w, waves);
                        EXPECT(r >= 0 && r < (int64_t)by_rank.size());
                        if (r < 0 || r >= (int64_t)by_rank.size()) continue;
                        EXPECT(!seen[(size_t)r]);                                  // the remap is a permutation
                        seen[(size_t)r] = 1;
                        const EgTiles s = nnconv_eg_wave_share((uint32_t)n_tiles, (uint32_t)nblk, (uint32_t)b, (uint32_t)w, (uint32_t)waves);
                        by_rank[(size_t)r] = s;
                        ++shares;
                        // the waves of a SIMD split exactly its slot's run
                        const EgTiles q = nnconv_eg_slot_share((uint32_t)n_tiles, (uint32_t)nblk, (uint32_t)b, (uint32_t)(w % 4));
                        EXPECT(q.t0 <= s.t0 && s.t1 <= q.t1);
                        if (w / 4 == 0) EXPECT(s.t0 == q.t0);
                        if (w / 4 == subs - 1) EXPECT(s.t1 == q.t1);
                    }
                }
                // every tile in exactly one share; the shares, in rank order, contiguous from 0 to n_tiles; none past the last tile
                uint32_t at = 0, longest = 0, shortest = ~0u;
                for (const EgTiles &s : by_rank) {
                    EXPECT(s.t0 <= s.t1 && s.t1 <= (uint32_t)n_tiles);
                    EXPECT(s.t0 == at);
                    at = s.t1;
                    if (s.t0 == s.t1) ++empty;                                   // (allowed: fewer tiles than waves)
                    for (uint32_t k = s.t0; k < s.t1 && k < (uint32_t)n_tiles; ++k)
                        if (owners[k] < 255) ++owners[k];
                    const uint32_t len = s.t1 - s.t0;
                    longest = len > longest ? len : longest;
                    shortest = len < shortest ? len : shortest;
                }
                EXPECT(at == (uint32_t)n_tiles);
                for (int k = 0; k < n_tiles; ++k) EXPECT(owners[(size_t)k] == 1);
                EXPECT(longest - shortest <= 2);                                  // slots balanced to one tile, their parts to one more
            }
    // the benchmark layout: 6 250 tiles over 224 blocks of 12 or 16 waves
    {
        uint32_t longest12 = 0, longest16 = 0;
        for (uint32_t b = 0; b < 224; ++b) {
            for (uint32_t w = 0; w < 12; ++w) {
                const EgTiles s = nnconv_eg_wave_share(6250, 224, b, w, 12);
                longest12 = s.t1 - s.t0 > longest12 ? s.t1 - s.t0 : longest12;
            }
            for (uint32_t w = 0; w < 16; ++w) {
                const EgTiles s = nnconv_eg_wave_share(6250, 224, b, w, 16);
                longest16 = s.t1 - s.t0 > longest16 ? s.t1 - s.t0 : longest16;
            }
        }
        EXPECT(longest12 == 3 && longest16 == 2);                                 // 6.98 tiles per SIMD slot
    }

    // ---- block count
    EXPECT(nnconv_eg_blocks(1, 224) == 1 && nnconv_eg_blocks(64, 224) == 1 && nnconv_eg_blocks(65, 224) == 2);
    EXPECT(nnconv_eg_blocks(7 * 64, 224) == 7 && nnconv_eg_blocks(8 * 64, 224) == 8 && nnconv_eg_blocks(9 * 64, 224) == 8);
    EXPECT(nnconv_eg_blocks(1254, 224) == 16 && nnconv_eg_blocks(4099, 224) == 64);                // 20, 65 blocks -> multiples of 8
    EXPECT(nnconv_eg_blocks(100000, 224) == 224 && nnconv_eg_blocks(100000, 256) == 256 && nnconv_eg_blocks(100000, 230) == 224);
    EXPECT(nnconv_eg_blocks(4099, 1) == 1 && nnconv_eg_blocks(4099, 8) == 8 && nnconv_eg_blocks(4099, 9) == 8 && nnconv_eg_blocks(4099, 7) == 7);
    EXPECT(nnconv_eg_blocks(0, 224) == 1 && nnconv_eg_blocks(int64_t(1) << 30, 1 << 20) == kEgMaxBlocks);

    // ---- the footprint table: what the general schedule claims fits one SIMD's 512 registers
    static_assert(vgprs_allocated(125) == 128 && vgprs_allocated(60) == 64 && vgprs_allocated(230) == 232 && vgprs_allocated(128) == 128, "granule 8");
    for (int k = 0; k < kLayerKernels; ++k) {
        const KernelFootprint &f = kLayerFootprints[k];
        EXPECT(f.waves_per_block >= 1 && f.waves_per_block <= 16 && f.vgpr_cap >= 8 && f.vgpr_cap <= 512);
        EXPECT(f.waves_per_simd == (f.waves_per_block + kEgSimds - 1) / kEgSimds);
        EXPECT(f.waves_per_simd * vgprs_allocated(f.vgpr_cap) <= kSimdVgprs);     // a block fits a CU at its cap
    }
    // the pairs the schedule relies on: one block of each fits a SIMD's registers at the caps the kernels are pinned to
    int pairs = 0;
    for (const CoResidentPair &p : kCoResidentPairs) {
        const KernelFootprint &a = kLayerFootprints[p.a], &b = kLayerFootprints[p.b];
        ++pairs;
        EXPECT(p.a != p.b);
        // (the cap of the GIN MLP is 256 and it is built at 230: beside the merge the COUNT it is built with has to fit, which
        //  tests/test_nnconv_eg_footprint.py checks on the device; here: the merge's cap leaves the MLP at least its 232)
        EXPECT(a.waves_per_simd * vgprs_allocated(230) + b.waves_per_simd * vgprs_allocated(b.vgpr_cap) <= kSimdVgprs);
    }
    EXPECT(pairs == 1 && kCoResidentPairs[0].a == kLayerGinMlp && kCoResidentPairs[0].b == kLayerMerge);
    // ... and what does NOT fit, as built (125, 60, 230, 120 registers): the NNConv beside either kernel of the collision chain
    EXPECT(4 * vgprs_allocated(125) + 1 * vgprs_allocated(60) > kSimdVgprs && 4 * vgprs_allocated(125) + 1 * vgprs_allocated(230) > kSimdVgprs);
    printf("nnconv_eg_plan_test: %ld wave shares (%ld empty), %d footprints, %d pair, %ld failures\n", shares, empty, (int)kLayerKernels, pairs, g_failures);
    return g_failures ? 1 : 0;
}
