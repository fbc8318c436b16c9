// Stand-alone check of the width-64 tall adjoint's plan (tilingnn_amd/csrc/mlp_bwd64_plan.h): the tile share and the grid of
// mlp_bwd_tall64_kernel, its partial-row layout, the workspace it asks for and the predicate that admits a shape.  No device, no HIP
// header:
//   g++ -std=c++17 -O1 -fsanitize=address,undefined -I include -I tilingnn_amd/csrc tests/host/mlp_bwd64_plan_test.cpp
// (tests/test_mlp_bwd64_plan_host.py builds and runs it).
#include <stdio.h>

#include <initializer_list>
#include <vector>

#include "mlp_bwd64_plan.h"

using namespace tgnn;

static long g_failures = 0;
#define EXPECT(cond)                                                              \
    do {                                                                          \
        if (!(cond) && ++g_failures <= 20) fprintf(stderr, "FAILED: %s (line %d)\n", #cond, __LINE__); \
    } while (0)

int main() {
    static_assert(kMlpBwd64Waves == 4 && kMlpBwd64Threads == 256, "one wave per SIMD");
    static_assert(kMlpBwd64RowFloats == 32 * 64 + 32 + 64 * 32 + 64 + 64 * 64 + 64 && kMlpBwd64RowFloats == 8352, "the six gradients");
    static_assert(kMlpBwd64OffB1 == kMlpBwd64OffW1 + 32 * 64 && kMlpBwd64OffW2 == kMlpBwd64OffB1 + 32 &&
                      kMlpBwd64OffB2 == kMlpBwd64OffW2 + 64 * 32 && kMlpBwd64OffW3 == kMlpBwd64OffB2 + 64 &&
                      kMlpBwd64OffB3 == kMlpBwd64OffW3 + 64 * 64 && kMlpBwd64OffB3 + 64 == kMlpBwd64RowFloats,
                  "[dW1 | db1 | dW2 | db2 | dW3 | db3] without gaps");
    static_assert(mlp_bwd_tall64_ok(1254, 64, 32, 64, 64) && mlp_bwd_tall64_blocks(1254) == 20, "usable in constant expressions");
    const std::initializer_list<int64_t> sizes = {1, 15, 16, 17, 127, 128, 129, 1254, 4099, 66003, 100000, 2000000};

    // ---- tile share: every 16-row tile of [0, ceil(n / 16)) belongs to exactly one wave, at every block count and at the planned one
    long shares = 0;
    for (int64_t n : sizes)
        for (int nblk : {1, 7, 8, 16, 157, 224, 256, mlp_bwd_tall64_blocks(n)}) {
            const int64_t n_tiles = (n + 15) / 16;
            std::vector<unsigned char> owners((size_t)n_tiles, 0);
            for (int b = 0; b < nblk; ++b)
                for (int w = 0; w < kMlpBwd64Waves; ++w) {
                    const Gin64Tiles t = mlp_bwd_tall64_tile_share(n, nblk, b, w);
                    EXPECT(0 <= t.t0 && t.t0 <= t.t1 && t.t1 <= n_tiles);
                    for (int64_t k = t.t0; k < t.t1 && k < n_tiles; ++k)
                        if (k >= 0 && owners[(size_t)k] < 255) ++owners[(size_t)k];
                    ++shares;
                }
            for (int64_t k = 0; k < n_tiles; ++k) EXPECT(owners[(size_t)k] == 1);
        }

    // ---- grid and workspace: the planned grid never exceeds the partial rows the workspace query pays for
    long grids = 0;
    for (int64_t n : sizes) {
        const int nblk = mlp_bwd_tall64_blocks(n);
        const size_t bytes = mlp_bwd_tall64_workspace_bytes(n, 64, 32, 64, 64);
        EXPECT(nblk >= 1 && nblk <= kMlpBwdMaxBlocks);
        EXPECT((size_t)nblk * kMlpBwd64RowFloats * sizeof(float) <= bytes && bytes % 256 == 0);
        EXPECT(bytes < (size_t)(nblk + 1) * kMlpBwd64RowFloats * sizeof(float));          // ... and not for one more
        EXPECT((int64_t)nblk * 4 >= gin64_n_tiles(n) || nblk == kMlpBwdMaxBlocks);         // a tile per wave until the cap
        if (nblk < kMlpBwdMaxBlocks)                                                       // below the cap no wave gets two tiles
            for (int b = 0; b < nblk; ++b)
                for (int w = 0; w < kMlpBwd64Waves; ++w) {
                    const Gin64Tiles t = mlp_bwd_tall64_tile_share(n, nblk, b, w);
                    EXPECT(t.t1 - t.t0 <= 1);
                }
        ++grids;
    }
    EXPECT(mlp_bwd_tall64_blocks(0) == 1 && mlp_bwd_tall64_blocks(1) == 1 && mlp_bwd_tall64_blocks(64) == 1 && mlp_bwd_tall64_blocks(65) == 2);
    EXPECT(mlp_bwd_tall64_blocks(1254) == 20 && mlp_bwd_tall64_blocks(4099) == 65);
    EXPECT(mlp_bwd_tall64_blocks(16320) == 255 && mlp_bwd_tall64_blocks(16321) == 256 && mlp_bwd_tall64_blocks(100000) == 256);

    // ---- the predicate: (64, 32, 64, 64) and nothing else, from no rows on; the older predicate still refuses the shape
    long shapes = 0;
    for (int64_t n : {int64_t(-1), int64_t(0), int64_t(1), int64_t(13), int64_t(63), int64_t(64), int64_t(1254), int64_t(2000000)})
        for (int d0 : {1, 15, 32, 64, 65, 128})
            for (int d1 : {16, 32, 64})
                for (int d2 : {32, 64, 128})
                    for (int d3 : {32, 64, 96, 4096}) {
                        const bool want = n >= 0 && d0 == 64 && d1 == 32 && d2 == 64 && d3 == 64;
                        EXPECT(mlp_bwd_tall64_ok(n, d0, d1, d2, d3) == want);
                        EXPECT((mlp_bwd_tall64_workspace_bytes(n, d0, d1, d2, d3) != 0) == want);
                        ++shapes;
                    }
    EXPECT(mlp_bwd_tall64_ok(1, 64, 32, 64, 64) && mlp_bwd_tall64_ok(2000000, 64, 32, 64, 64));        // no row floor
    EXPECT(!mlp_bwd_tall64_ok(1254, 32, 32, 64, 32) && !mlp_bwd_tall64_ok(1254, 64, 32, 64, 32));
    EXPECT(!mlp_bwd_tall64_ok(1254, 64, 64, 64, 64) && !mlp_bwd_tall64_ok(-1, 64, 32, 64, 64));
    EXPECT(!mlp_bwd_tall64_ok(13, 15, 32, 64, 4096));
    EXPECT(mlp_bwd_form(1254, 64, 32, 64, 64, 1) == 0 && mlp_bwd_form(1254, 64, 32, 64, 64, 0) == 0);
    EXPECT(mlp_bwd_fused_workspace_bytes(1254, 64, 32, 64, 64) == 0);

    printf("mlp_bwd64_plan_test: %ld tile shares, %ld grids, %ld shapes, %ld failures\n", shares, grids, shapes, g_failures);
    return g_failures ? 1 : 0;
}
