// Stand-alone check of the width-64 matrix-core GIN MLP's tile share and of the predicate that routes a forward to it
// (tilingnn_amd/csrc/gin64_plan.h, forward_plan.h: ForwardPlan::gin64).  No device, no HIP header:
//   g++ -std=c++17 -O1 -fsanitize=address,undefined -I include -I tilingnn_amd/csrc tests/host/gin64_plan_test.cpp
// (tests/test_gin64_mfma_host.py builds and runs it).
#include <stdio.h>

#include <initializer_list>
#include <vector>

#include "forward_plan.h"

using namespace tgnn;

struct NoProbe {                                            // (width 64 asks the device nothing; width 32 gets "not eligible")
    int small_layout_teams() { return 0; }
    int mid_layout_tiles_per_block(int *) { return 0; }
    int mid_tail_tiles_per_block(int *) { return 0; }
};

static long g_failures = 0;
#define EXPECT(cond)                                                              \
    do {                                                                          \
        if (!(cond) && ++g_failures <= 20) fprintf(stderr, "FAILED: %s (line %d)\n", #cond, __LINE__); \
    } while (0)

// the slot order the kernel's ranges are contiguous in: the XCD remap of the block, then the SIMD, then the wave of the SIMD
static int64_t walk_rank(int nblk, int block, int wave) {
    int64_t blk = block;
    if (nblk >= 8 && (nblk & 7) == 0) blk = (int64_t)(block & 7) * (nblk >> 3) + (block >> 3);
    return (blk * 4 + (wave & 3)) * 2 + (wave >> 2);
}

int main() {
    static_assert(kGin64Waves == 8 && kGin64TileRows == 16 && kGin64BlockRows == 128 && kGin64Threads == 512, "the kernel's shape");
    static_assert(gin64_tile_share(17, 1, 0, 0).t0 == 0, "usable in constant expressions");
    // ---- tile share: every 16-row tile belongs to exactly one wave; ranges contiguous, in order, none past ceil(n / 16)
    long shares = 0;
    for (int64_t n : {int64_t(1), int64_t(15), int64_t(16), int64_t(17), int64_t(127), int64_t(128), int64_t(129), int64_t(1254),
                      int64_t(4099), int64_t(28672), int64_t(28673), int64_t(66003), int64_t(2000000)})
        for (int nblk : {1, 7, 8, 16, 157, 224, 256}) {
            const int64_t n_tiles = (n + 15) / 16;
            EXPECT(gin64_n_tiles(n) == n_tiles);
            std::vector<Gin64Tiles> by_rank((size_t)nblk * kGin64Waves, Gin64Tiles{-1, -1});
            std::vector<unsigned char> owners((size_t)n_tiles, 0);
            for (int b = 0; b < nblk; ++b)
                for (int w = 0; w < kGin64Waves; ++w) {
                    const Gin64Tiles t = gin64_tile_share(n, nblk, b, w);
                    EXPECT(0 <= t.t0 && t.t0 <= t.t1 && t.t1 <= n_tiles);
                    const int64_t r = walk_rank(nblk, b, w);
                    EXPECT(r >= 0 && r < (int64_t)by_rank.size() && by_rank[(size_t)r].t0 == -1);   // the remap is a permutation
                    if (r >= 0 && r < (int64_t)by_rank.size()) by_rank[(size_t)r] = t;
                    for (int64_t k = t.t0; k < t.t1 && k < n_tiles; ++k)
                        if (k >= 0 && owners[(size_t)k] < 255) ++owners[(size_t)k];
                    ++shares;
                }
            for (int64_t k = 0; k < n_tiles; ++k) EXPECT(owners[(size_t)k] == 1);
            int64_t at = 0;
            int64_t longest = 0, shortest = n_tiles;
            for (const Gin64Tiles &t : by_rank) {
                EXPECT(t.t0 == at);                                     // contiguous and in order
                at = t.t1;
                longest = t.t1 - t.t0 > longest ? t.t1 - t.t0 : longest;
                shortest = t.t1 - t.t0 < shortest ? t.t1 - t.t0 : shortest;
            }
            EXPECT(at == n_tiles);
            EXPECT(longest - shortest <= 2);                            // balanced: SIMD slots to one tile, their halves to one more
        }

    // ---- the predicate over the cross product of what it reads, and the plan around it
    long count = 0;
    for (int c : {32, 64, 66})
        for (int sharded : {0, 1})
            for (int sw : {0, 1})
                for (int urs : {0, 1})
                    for (int keep : {0, 1})
                        for (int eg64 : {0, 1})
                            for (int groups : {0, 1}) {
                                if ((sharded && (urs || keep)) || (urs && keep)) continue;       // (forward_impl refuses these)
                                ForwardFacts f;
                                f.c = c; f.D = 3; f.fx = 3; f.fe = 4;
                                f.nr = 5000; f.n = sharded ? 4000 : 5000; f.T = 13; f.max_in_degree = 40;
                                f.has_groups = groups != 0; f.has_cols = true;
                                f.sharded = sharded != 0; f.world = sharded ? 2 : 0;
                                f.use_running_stats = urs != 0; f.keep = keep != 0;
                                f.distinct_side_stream = true; f.device_cus = 256;
                                f.nnconv64_eg = eg64;
                                f.gin64_mfma = sw;
                                NoProbe probe;
                                const ForwardPlan p = plan_forward(f, probe);
                                const bool want = c == 64 && !sharded && sw == 1;
                                EXPECT(p.gin64 == want);
                                EXPECT(p.gin64 == gin64_mfma_ok(c, sharded != 0, sw));
                                // the route touches nothing else of the plan: with the switch at 0 the plan is today's
                                ForwardFacts f0 = f;
                                f0.gin64_mfma = 0;
                                NoProbe probe0;
                                const ForwardPlan p0 = plan_forward(f0, probe0);
                                EXPECT(!p0.gin64);
                                EXPECT(p0.side == p.side && p0.cols_ok == p.cols_ok && p0.groups_ok == p.groups_ok && p0.small_teams == p.small_teams &&
                                       p0.mid_k == p.mid_k && p0.mid_blocks == p.mid_blocks && p0.tail_k == p.tail_k && p0.tail_blocks == p.tail_blocks &&
                                       p0.mid_counter == p.mid_counter && p0.mid_init == p.mid_init && p0.verdict_refused == p.verdict_refused &&
                                       p0.f16 == p.f16 && p0.eg == p.eg && p0.tiled == p.tiled && p0.lean_head == p.lean_head && p0.eg64 == p.eg64 &&
                                       p0.init_fused_early == p.init_fused_early && p0.init_fused == p.init_fused && p0.head_used == p.head_used &&
                                       p0.weights_on_main == p.weights_on_main && p0.weights_queued == p.weights_queued &&
                                       p0.small_pre_used == p.small_pre_used && p0.weights_done == p.weights_done &&
                                       p0.weights_on_side == p.weights_on_side && p0.queue_weights == p.queue_weights && p0.nn_first == p.nn_first &&
                                       p0.fold_fin2 == p.fold_fin2 && p0.zero_fold_ctr == p.zero_fold_ctr && p0.fold_final == p.fold_final &&
                                       p0.fused_shard == p.fused_shard && p0.split == p.split && p0.pack_in_nnconv == p.pack_in_nnconv &&
                                       p0.fused_bn1_ok == p.fused_bn1_ok && p0.init_stats_written == p.init_stats_written && p0.scales == p.scales &&
                                       p0.final_operands == p.final_operands && p0.path == p.path);
                                if (p.gin64) EXPECT(p.path == ForwardPath::General && !p.fold_fin2);
                                ++count;
                            }
    EXPECT(!gin64_mfma_ok(64, false, 2) && !gin64_mfma_ok(64, false, -1));       // only the value the setter stores selects it
    ForwardFacts dflt;
    EXPECT(dflt.gin64_mfma == 0);                           // the switch is off unless somebody sets it
    printf("gin64_plan_test: %ld tile shares, %ld combinations, %ld failures\n", shares, count, g_failures);
    return g_failures ? 1 : 0;
}
