// Stand-alone check of the edge-group NNConv adjoint's plan (tilingnn_amd/csrc/nnconv_bwd_eg_plan.h): the predicate on either side of
// each limit, the grid of the dW kernel, the shares of the type-major group list, the partial-slot layout and the workspace.  No
// device, no HIP header:
//   g++ -std=c++17 -O1 -fsanitize=address,undefined -I include -I tilingnn_amd/csrc tests/host/nnconv_bwd_eg_plan_test.cpp
// (tests/test_nnconv_bwd_eg_plan_host.py builds and runs it).
#include <stdio.h>

#include <initializer_list>
#include <vector>

#include "nnconv_bwd_eg_plan.h"

using namespace tgnn;

static long g_failures = 0;
#define EXPECT(cond)                                                              \
    do {                                                                          \
        if (!(cond) && ++g_failures <= 20) fprintf(stderr, "FAILED: %s (line %d)\n", #cond, __LINE__); \
    } while (0)

int main() {
    static_assert(kBwdEgDwWaves == 4 && kBwdEgDwThreads == 256 && kBwdEgDwMaxBlocks == 512, "one wave per SIMD, two blocks per CU");
    static_assert(nnconv_bwd_eg_max_types(64) == 18 && nnconv_bwd_eg_max_types(32) == 22 && nnconv_bwd_eg_max_types(16) == 0, "limits");
    static_assert(nnconv_bwd_eg_ok(64, 1254, 13, 12, 12, true, true) && nnconv_bwd_eg_dw_blocks(1254) == 79, "constant expressions");
    const int grid = kBwdEgDwMaxBlocks * kBwdEgDwWaves * kBwdEgDwGroupsPerWave;      // the list length at which the grid reaches its cap
    const std::initializer_list<int64_t> lengths = {0, 1, 15, 16, 17, 511, 512, 513, grid - 1, grid, grid + 1, 200000};

    // ---- shares: every entry of the list belongs to exactly one block, at every grid the plan produces (the cap given or not)
    long shares = 0, grids = 0;
    for (int64_t L : lengths)
        for (int cap : {1, 7, 8, 9, 255, 511, 512, 100000}) {
            const int nblk = nnconv_bwd_eg_dw_blocks(L, cap);
            EXPECT(nblk >= 1 && nblk <= kBwdEgDwMaxBlocks && (nblk <= cap || cap < 1));
            EXPECT(nblk == 1 || (int64_t)(nblk - 1) * kBwdEgDwWaves * kBwdEgDwGroupsPerWave < L);      // no block without a group
            std::vector<unsigned char> owners((size_t)L, 0);
            int64_t prev_end = 0;
            for (int b = 0; b < nblk; ++b) {
                const BwdEgShare s = nnconv_bwd_eg_dw_share(L, nblk, b);
                EXPECT(s.begin == prev_end && s.begin <= s.end && s.end <= L);
                prev_end = s.end;
                for (int64_t k = s.begin; k < s.end; ++k)
                    if (owners[(size_t)k] < 255) ++owners[(size_t)k];
                ++shares;
            }
            EXPECT(prev_end == L);
            for (int64_t k = 0; k < L; ++k) EXPECT(owners[(size_t)k] == 1);
            ++grids;
        }
    EXPECT(nnconv_bwd_eg_dw_blocks(0) == 1 && nnconv_bwd_eg_dw_blocks(16) == 1 && nnconv_bwd_eg_dw_blocks(17) == 2);
    EXPECT(nnconv_bwd_eg_dw_blocks(grid - 16) == 511 && nnconv_bwd_eg_dw_blocks(grid - 15) == 512 && nnconv_bwd_eg_dw_blocks(200000) == 512);

    // ---- partial slots: with the list cut into T + 1 types (some empty), the slot of (block, type) over every pair that shares a
    // group is unique and inside the workspace; per type the blocks that meet it are a contiguous run (what the fold walks)
    long slots_checked = 0;
    for (int64_t L : lengths)
        for (int T : {1, 2, 13, 18, 22})
            for (int cap : {1, 8, 9, 512}) {
                const int nblk = nnconv_bwd_eg_dw_blocks(L, cap);
                std::vector<int64_t> off((size_t)T + 2, 0);
                for (int t = 0; t <= T; ++t) {                   // uneven types, every third one empty
                    const int64_t w = (t % 3 == 1) ? 0 : (int64_t)(t + 1) * (t + 2);
                    off[(size_t)t + 1] = off[(size_t)t] + w;
                }
                const int64_t total = off[(size_t)T + 1];
                for (int t = 0; t <= T + 1; ++t) off[(size_t)t] = total ? off[(size_t)t] * L / total : 0;
                off[(size_t)T + 1] = L;
                std::vector<unsigned char> used((size_t)nnconv_bwd_eg_dw_slots(T), 0);
                for (int t = 0; t <= T; ++t) {
                    int first = -1, last = -1, met = 0;
                    for (int b = 0; b < nblk; ++b) {
                        const BwdEgShare s = nnconv_bwd_eg_dw_share(L, nblk, b);
                        const int64_t lo = s.begin > off[(size_t)t] ? s.begin : off[(size_t)t];
                        const int64_t hi = s.end < off[(size_t)t + 1] ? s.end : off[(size_t)t + 1];
                        if (lo >= hi) continue;
                        const int slot = nnconv_bwd_eg_dw_slot(b, t);
                        EXPECT(slot >= 0 && slot < nnconv_bwd_eg_dw_slots(T));
                        if (slot >= 0 && slot < nnconv_bwd_eg_dw_slots(T)) {
                            EXPECT(used[(size_t)slot] == 0);     // never another (block, type)'s
                            used[(size_t)slot] = 1;
                        }
                        if (first < 0) first = b;
                        last = b;
                        ++met;
                        ++slots_checked;
                    }
                    EXPECT(met == 0 || met == last - first + 1);
                }
            }

    // ---- workspace: the layout's pieces in order, 256-byte aligned, the slots of the largest grid inside
    long spaces = 0;
    for (int c : {32, 64})
        for (int T = 1; T <= nnconv_bwd_eg_max_types(c); ++T) {
            const BwdEgWorkspace w = nnconv_bwd_eg_workspace(T, c);
            EXPECT(w.bounds == 0 && w.wt == 256 && w.wt % 256 == 0 && w.wimg % 256 == 0 && w.slots % 256 == 0 && w.total % 256 == 0);
            EXPECT(w.wimg - w.wt >= (size_t)(T + 1) * c * c * 4);
            EXPECT(w.slots - w.wimg >= (size_t)(T + 1) * (c == 64 ? 16384 : 4096));
            EXPECT(w.total - w.slots >= (size_t)(kBwdEgDwMaxBlocks + T + 1) * c * c * 4);
            EXPECT(w.total - w.slots < (size_t)(kBwdEgDwMaxBlocks + T + 2) * c * c * 4);               // ... and not one more
            EXPECT(nnconv_bwd_eg_workspace_bytes(1254, 2000, T, c) == w.total && nnconv_bwd_eg_workspace_bytes(100000, 200000, T, c) == w.total);
            ++spaces;
        }
    EXPECT(nnconv_bwd_eg_workspace_bytes(1254, 2000, 19, 64) == 0 && nnconv_bwd_eg_workspace_bytes(1254, 2000, 23, 32) == 0);
    EXPECT(nnconv_bwd_eg_workspace_bytes(1254, 2000, 13, 16) == 0 && nnconv_bwd_eg_workspace_bytes(1254, 2000, 13, 128) == 0);
    EXPECT(nnconv_bwd_eg_workspace_bytes(0, 2000, 13, 32) == 0 && nnconv_bwd_eg_workspace_bytes(1254, -1, 13, 32) == 0);
    EXPECT(nnconv_bwd_eg_list_ints(0) == 64 && nnconv_bwd_eg_list_ints(2000) == 64 + 4000);

    // ---- the predicate on either side of each limit
    long preds = 0;
    auto ok = [&](int c, int64_t n, int T, int din, int dout, bool f, bool b) {
        ++preds;
        const bool v = nnconv_bwd_eg_ok(c, n, T, din, dout, f, b);
        EXPECT(v == (nnconv_bwd_eg_why_not(c, n, T, din, dout, f, b) == nullptr));
        return v;
    };
    EXPECT(ok(64, 1254, 18, 12, 12, true, true) && !ok(64, 1254, 19, 12, 12, true, true));
    EXPECT(ok(32, 1254, 22, 12, 12, true, true) && !ok(32, 1254, 23, 12, 12, true, true));
    EXPECT(ok(32, 1254, 1, 12, 12, true, true) && !ok(32, 1254, 0, 12, 12, true, true) && !ok(64, 1254, 63, 12, 12, true, true));
    EXPECT(ok(32, 1254, 13, 2048, 12, true, true) && !ok(32, 1254, 13, 2049, 12, true, true) && !ok(32, 1254, 13, 0, 12, true, true));
    EXPECT(ok(64, 1254, 13, 12, 2048, true, true) && !ok(64, 1254, 13, 12, 2049, true, true) && !ok(64, 1254, 13, 12, 0, true, true));
    EXPECT(!ok(16, 1254, 13, 12, 12, true, true) && !ok(128, 1254, 13, 12, 12, true, true) && !ok(48, 1254, 13, 12, 12, true, true));
    EXPECT(!ok(32, 1254, 13, 12, 12, false, true) && !ok(32, 1254, 13, 12, 12, true, false) && !ok(64, 1254, 13, 12, 12, false, false));
    // rows within 2 GB: n c 4 < 2^31
    EXPECT(ok(64, (int64_t(1) << 23) - 1, 13, 12, 12, true, true) && !ok(64, int64_t(1) << 23, 13, 12, 12, true, true));
    EXPECT(ok(32, (int64_t(1) << 24) - 1, 13, 12, 12, true, true) && !ok(32, int64_t(1) << 24, 13, 12, 12, true, true));
    EXPECT(!ok(32, 0, 13, 12, 12, true, true));

    printf("nnconv_bwd_eg_plan_test: %ld shares, %ld grids, %ld slots, %ld workspaces, %ld predicates, %ld failures\n", shares, grids,
           slots_checked, spaces, preds, g_failures);
    return g_failures ? 1 : 0;
}
