// Stand-alone check of the width-64 edge-group NNConv's limits and of the predicate that routes a forward to it
// (tilingnn_amd/csrc/nnconv64_eg_plan.h, forward_plan.h: ForwardPlan::eg64).  No device, no HIP header:
//   g++ -std=c++17 -O1 -fsanitize=address,undefined -I include -I tilingnn_amd/csrc tests/host/nnconv64_eg_plan_test.cpp
// (tests/test_nnconv64_eg_host.py builds and runs it).
#include <stdio.h>

#include <initializer_list>

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

int main() {
    // ---- LDS: 8 KiB per entry (types + root) and the selection table; T = limit fits, limit + 1 does not
    const int limit = nnconv64_eg_max_types();
    EXPECT(limit >= 18);
    EXPECT(nnconv64_eg_lds_bytes(limit) <= kEg64MaxLds);
    EXPECT(nnconv64_eg_lds_bytes(limit + 1) > kEg64MaxLds);
    EXPECT(nnconv64_eg_lds_bytes(13) == (size_t)14 * 8192 + 128);
    EXPECT(nnconv64_eg_lds_bytes(0) >= (size_t)kEg64Waves * 64 * 8 * sizeof(double));     // the BatchNorm reduction's floor
    for (int t = 0; t <= limit; ++t) EXPECT(nnconv64_eg_lds_bytes(t) <= kEg64MaxLds);
    EXPECT(kEg64TypeFloats * sizeof(float) == 16384 && kEg64HalfFloats * 2 == kEg64TypeFloats);

    // ---- the predicate over the cross product of what it reads
    const int64_t row_limit = (int64_t(1) << 31) / 256;      // nr * 256 < 2^31  <=>  nr < row_limit
    long count = 0;
    for (int c : {32, 64, 128})
        for (int T : {0, 1, limit, limit + 1})
            for (int64_t nr : {int64_t(2), row_limit - 1, row_limit, row_limit + 1})
                for (int deg : {0, 1, kEg64MaxInDegree, kEg64MaxInDegree + 1})
                    for (int sw : {0, 1})
                        for (int sharded : {0, 1})
                            for (int groups : {0, 1})
                                for (int urs : {0, 1})
                                    for (int keep : {0, 1}) {
                                        if ((sharded && (urs || keep)) || (urs && keep)) continue;   // (forward_impl refuses these)
                                        ForwardFacts f;
                                        f.c = c; f.D = 3; f.fx = 3; f.fe = 4;
                                        f.n = sharded ? (nr > 2 ? nr - 1 : nr) : nr; f.nr = nr; f.T = T; f.max_in_degree = deg;
                                        f.has_groups = groups != 0; f.has_cols = true;
                                        f.sharded = sharded != 0; f.world = sharded ? 2 : 0;
                                        f.use_running_stats = urs != 0; f.keep = keep != 0;
                                        f.distinct_side_stream = true; f.device_cus = 256;
                                        f.nnconv64_eg = sw;
                                        NoProbe probe;
                                        const ForwardPlan p = plan_forward(f, probe);
                                        const bool want = c == 64 && !sharded && groups && nr < row_limit && T >= 1 && T <= limit &&
                                                          deg >= 1 && deg <= kEg64MaxInDegree && !urs && sw;
                                        EXPECT(p.eg64 == want);
                                        EXPECT(p.eg64 == nnconv64_eg_ok(c, sharded != 0, groups != 0, nr, T, deg, urs != 0, sw));
                                        // the width-64 route touches nothing else of the plan
                                        ForwardFacts f0 = f;
                                        f0.nnconv64_eg = 0;
                                        NoProbe probe0;
                                        ForwardPlan p0 = plan_forward(f0, probe0);
                                        EXPECT(!p0.eg64);
                                        p0.eg64 = p.eg64;
                                        EXPECT(p0.path == p.path && p0.f16 == p.f16 && p0.eg == p.eg && p0.tiled == p.tiled && p0.side == p.side &&
                                               p0.queue_weights == p.queue_weights && p0.weights_on_side == p.weights_on_side &&
                                               p0.scales == p.scales && p0.final_operands == p.final_operands);
                                        if (p.eg64) EXPECT(p.path == ForwardPath::General && !p.f16 && !p.eg && p.queue_weights);
                                        ++count;
                                    }
    ForwardFacts dflt;
    EXPECT(dflt.nnconv64_eg == 0);                           // the switch is off unless somebody sets it
    printf("nnconv64_eg_plan_test: limit %d, %ld combinations, %ld failures\n", limit, count, g_failures);
    return g_failures ? 1 : 0;
}
