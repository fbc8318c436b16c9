// Stand-alone check of the fused sigmoid-MLP adjoints' plan (tilingnn_amd/csrc/mlp_bwd_plan.h): the tall form's tile share and grid,
// the workspace both forms ask for, and the predicate that picks the form.  No device, no HIP header:
//   g++ -std=c++17 -O1 -fsanitize=address,undefined -I include -I tilingnn_amd/csrc tests/host/mlp_bwd_plan_test.cpp
// (tests/test_mlp_bwd_plan_host.py builds and runs it).
#include <stdio.h>

#include <initializer_list>
#include <vector>

#include "mlp_bwd_plan.h"

using namespace tgnn;

static long g_failures = 0;
#define EXPECT(cond)                                                              \
    do {                                                                          \
        if (!(cond) && ++g_failures <= 20) fprintf(stderr, "FAILED: %s (line %d)\n", #cond, __LINE__); \
    } while (0)

int main() {
    static_assert(kMlpBwdWaves == 8 && kMlpBwdTileRows == 16 && kMlpBwdThreads == 512, "the tall kernel's shape");
    static_assert(kMlpBwdRowFloats == 32 * 32 + 32 + 64 * 32 + 64 + 32 * 64 + 32 && kMlpBwdOffB3 + 32 == kMlpBwdRowFloats,
                  "a partial row holds the six gradients");
    static_assert(mlp_bwd_form(1254, 32, 32, 64, 32, 1) == 1 && mlp_bwd_tall_blocks(1254) == 20, "usable in constant expressions");
    const std::initializer_list<int64_t> sizes = {1, 15, 16, 17, 127, 128, 129, 1254, 4099, 66003, 100000, 2000000};

    // ---- tile share: every 16-row tile of [0, ceil(n / 16)) belongs to exactly one wave, at every block count and at the planned one
    long shares = 0;
    for (int64_t n : sizes)
        for (int nblk : {1, 7, 8, 16, 157, 224, 256, mlp_bwd_tall_blocks(n)}) {
            const int64_t n_tiles = (n + 15) / 16;
            std::vector<unsigned char> owners((size_t)n_tiles, 0);
            for (int b = 0; b < nblk; ++b)
                for (int w = 0; w < kMlpBwdWaves; ++w) {
                    const Gin64Tiles t = mlp_bwd_tile_share(n, nblk, b, w);
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
        const int nblk = mlp_bwd_tall_blocks(n);
        const size_t bytes = mlp_bwd_fused_workspace_bytes(n, 32, 32, 64, 32);
        EXPECT(nblk >= 1 && nblk <= kMlpBwdMaxBlocks);
        EXPECT((size_t)nblk * kMlpBwdRowFloats * sizeof(float) <= bytes && bytes % 256 == 0);
        EXPECT((int64_t)nblk * 4 >= gin64_n_tiles(n) || nblk == kMlpBwdMaxBlocks);     // four tiles per block until the cap
        // below the cap no SIMD gets two tiles: the longest run of a wave is one tile
        if (nblk < kMlpBwdMaxBlocks)
            for (int b = 0; b < nblk; ++b)
                for (int w = 0; w < kMlpBwdWaves; ++w) {
                    const Gin64Tiles t = mlp_bwd_tile_share(n, nblk, b, w);
                    EXPECT(t.t1 - t.t0 <= 1);
                    if (w < 4) EXPECT(mlp_bwd_tile_share(n, nblk, b, w + 4).t1 - t.t0 <= 1);      // (w, w + 4) share a SIMD
                }
        ++grids;
    }
    EXPECT(mlp_bwd_tall_blocks(1) == 1 && mlp_bwd_tall_blocks(64) == 1 && mlp_bwd_tall_blocks(65) == 2);
    EXPECT(mlp_bwd_tall_blocks(1254) == 20);                  // not the 10 blocks of eight tiles each
    EXPECT(mlp_bwd_tall_blocks(4099) == 65 && mlp_bwd_tall_blocks(16384) == 256 && mlp_bwd_tall_blocks(100000) == 256);
    for (int T : {1, 13, 63})
        for (int c : {32, 64}) {
            const size_t bytes = mlp_bwd_fused_workspace_bytes(T, 15, 32, 64, c * c);
            EXPECT(mlp_bwd_wide_chunks(c * c) == c * c / 64);
            EXPECT((size_t)mlp_bwd_wide_chunks(c * c) * T * 64 * sizeof(float) <= bytes && bytes % 256 == 0);
        }
    EXPECT(mlp_bwd_fused_workspace_bytes(300, 64, 32, 64, 64) == 0 && mlp_bwd_fused_workspace_bytes(64, 15, 32, 64, 1024) == 0);

    // ---- the form predicate over a table of shapes: tall only for (32, 32, 64, 32), wide only inside its limits
    long forms = 0;
    for (int64_t n : {int64_t(0), int64_t(1), int64_t(13), int64_t(63), int64_t(64), int64_t(1254), int64_t(100000)})
        for (int d0 : {1, 5, 15, 32, 64, 65})
            for (int d1 : {16, 32, 64})
                for (int d2 : {32, 64})
                    for (int d3 : {32, 64, 96, 1024, 4096})
                        for (int dx : {0, 1}) {
                            const bool tall = d0 == 32 && d1 == 32 && d2 == 64 && d3 == 32;
                            const bool wide = !tall && !dx && n <= 63 && d0 <= 64 && d1 == 32 && d2 == 64 && d3 % 64 == 0;
                            EXPECT(mlp_bwd_form(n, d0, d1, d2, d3, dx) == (tall ? 1 : wide ? 2 : 0));
                            EXPECT((mlp_bwd_fused_workspace_bytes(n, d0, d1, d2, d3) != 0) == (mlp_bwd_form(n, d0, d1, d2, d3, 0) != 0));
                            ++forms;
                        }
    EXPECT(mlp_bwd_form(1254, 64, 32, 64, 64, 1) == 0 && mlp_bwd_form(1254, 64, 32, 64, 64, 0) == 0);   // width 64's GIN MLP
    EXPECT(mlp_bwd_form(63, 15, 32, 64, 1024, 0) == 2 && mlp_bwd_form(64, 15, 32, 64, 1024, 0) == 0);   // T = 64
    EXPECT(mlp_bwd_form(13, 64, 32, 64, 4096, 0) == 2 && mlp_bwd_form(13, 65, 32, 64, 4096, 0) == 0);   // fe = 65
    EXPECT(mlp_bwd_form(13, 15, 32, 64, 1024, 1) == 0);                                                // the wide shape with dx
    EXPECT(mlp_bwd_form(-1, 32, 32, 64, 32, 1) == 0 && mlp_bwd_form(13, 0, 32, 64, 1024, 0) == 0);
    EXPECT(mlp_bwd_form(1, 32, 32, 64, 32, 0) == 1 && mlp_bwd_form(2000000, 32, 32, 64, 32, 1) == 1);  // no row floor

    printf("mlp_bwd_plan_test: %ld tile shares, %ld grids, %ld forms, %ld failures\n", shares, grids, forms, g_failures);
    return g_failures ? 1 : 0;
}
