// Stand-alone check of the fused Adam step's host plan (tilingnn_amd/csrc/adam_plan.h): the moment layout, the chunk list cut
// from a segment table and the checks a launch relies on.  No device, no HIP header:
//   g++ -std=c++17 -O1 -fsanitize=address,undefined -I include -I tilingnn_amd/csrc tests/host/adam_plan_test.cpp
// (tests/test_adam_plan_host.py builds and runs it, with and without the sanitizers).
#include <stdio.h>

#include <vector>

#include "adam_plan.h"

using namespace tgnn;

static long g_failures = 0;
#define EXPECT(cond)                                                              \
    do {                                                                          \
        if (!(cond) && ++g_failures <= 20) fprintf(stderr, "FAILED: %s (line %d)\n", #cond, __LINE__); \
    } while (0)

struct Plan {
    std::vector<AdamSegment> segs;
    std::vector<AdamChunk> chunks;
    int64_t moment_floats = 0;
};

// segments laid out as tilingnn_amd/optim.py lays them out: moments one slice after the other, gradients 64-float aligned in one
// buffer (the shape of tgnn_backward's), parameters anywhere (the plan never dereferences them)
static Plan make_plan(const std::vector<int64_t> &numel, float *fake_params) {
    Plan pl;
    int64_t moff = 0, goff = 0;
    for (int64_t n : numel) {
        pl.segs.push_back(AdamSegment{fake_params, goff * 4, moff, n});
        moff = adam_next_moment_off(moff, n);
        goff += (n + 63) / 64 * 64;
    }
    pl.moment_floats = moff;
    const int64_t want = adam_chunk_count(numel.data(), (int32_t)numel.size());
    pl.chunks.assign((size_t)(want > 0 ? want : 0), AdamChunk{-1, -1, -1});
    const int64_t cut = adam_cut_chunks(pl.segs.data(), (int32_t)pl.segs.size(), pl.chunks.data());
    EXPECT(cut == want);
    return pl;
}

static long check_plan(const Plan &pl, const std::vector<int64_t> &numel) {
    const int32_t ns = (int32_t)pl.segs.size();
    // the chunk count is the sum of ceil(numel / chunk)
    int64_t want = 0;
    for (int64_t n : numel) want += (n + kAdamChunk - 1) / kAdamChunk;
    EXPECT((int64_t)pl.chunks.size() == want);
    EXPECT(adam_check_segments(pl.segs.data(), ns, pl.moment_floats) == nullptr);
    EXPECT(adam_check_chunks(pl.segs.data(), ns, pl.chunks.data(), (int64_t)pl.chunks.size()) == nullptr);
    // the chunks tile every segment exactly once and none crosses a segment's end
    std::vector<std::vector<unsigned char>> owners;
    for (int64_t n : numel) owners.emplace_back((size_t)n, (unsigned char)0);
    for (const AdamChunk &c : pl.chunks) {
        EXPECT(c.segment >= 0 && c.segment < ns && c.reserved_ == 0);
        if (c.segment < 0 || c.segment >= ns) continue;
        const int64_t n = pl.segs[(size_t)c.segment].numel;
        EXPECT(c.start >= 0 && c.start < n && c.start % kAdamChunk == 0);
        const int64_t end = c.start + kAdamChunk < n ? c.start + kAdamChunk : n;     // what the kernel covers
        EXPECT(end - c.start >= 1 && end - c.start <= kAdamChunk && end <= n);
        for (int64_t e = c.start; e < end; ++e)
            if (e >= 0 && e < n && owners[(size_t)c.segment][(size_t)e] < 255) ++owners[(size_t)c.segment][(size_t)e];
    }
    for (size_t s = 0; s < owners.size(); ++s)
        for (unsigned char o : owners[s]) EXPECT(o == 1);
    // moment slices: 64-float aligned, inside the buffers, disjoint (ascending here: each starts at or behind the previous one's end)
    int64_t prev_end = 0;
    for (const AdamSegment &g : pl.segs) {
        EXPECT(g.moment_off % kAdamMomentAlign == 0);
        EXPECT(g.moment_off >= prev_end);
        EXPECT(g.moment_off + g.numel <= pl.moment_floats);
        prev_end = g.moment_off + g.numel;
    }
    return (long)pl.chunks.size();
}

int main() {
    static_assert(kAdamChunk % 4 == 0 && kAdamMomentAlign * sizeof(float) == 256, "the kernel's vector width, 256-byte slices");
    static_assert(adam_chunks_of(0) == 0 && adam_chunks_of(1) == 1 && adam_chunks_of(kAdamChunk) == 1 &&
                      adam_chunks_of(kAdamChunk + 1) == 2,
                  "usable in constant expressions");
    static float fake[4];
    const int64_t C_ = kAdamChunk;
    const std::vector<int64_t> sizes = {0, 1, 3, 4, 5, 63, 64, 65, C_ - 1, C_, C_ + 1, 2 * C_ + 7, (int64_t)256 * 672};
    long chunks = 0, plans = 0;
    // all sizes in one table, in this order and reversed; every size alone; every size between two vectors of 32
    {
        Plan pl = make_plan(sizes, fake);
        chunks += check_plan(pl, sizes);
        ++plans;
        std::vector<int64_t> rev(sizes.rbegin(), sizes.rend());
        Plan pr = make_plan(rev, fake);
        chunks += check_plan(pr, rev);
        ++plans;
    }
    for (int64_t n : sizes) {
        const std::vector<int64_t> one = {n}, mid = {32, n, 32};
        Plan a = make_plan(one, fake), b = make_plan(mid, fake);
        chunks += check_plan(a, one) + check_plan(b, mid);
        plans += 2;
    }
    // the shape of a real group: one 172 032-element matrix and 300 vectors of 32 balance as 42 + 300 blocks
    {
        std::vector<int64_t> net = {(int64_t)256 * 672};
        for (int i = 0; i < 300; ++i) net.push_back(32);
        Plan pl = make_plan(net, fake);
        EXPECT(check_plan(pl, net) == 42 + 300);
        chunks += 342;
        ++plans;
    }
    // the empty table
    {
        EXPECT(adam_chunk_count(nullptr, 0) == 0);
        EXPECT(adam_check_segments(nullptr, 0, 0) == nullptr && adam_check_chunks(nullptr, 0, nullptr, 0) == nullptr);
        EXPECT(adam_table_bytes(0, 0) == 0 && adam_table_bytes(3, 5) == 3 * 32 + 5 * 16);
    }

    // ---- what the checks refuse
    long refusals = 0;
    {
        const int64_t neg[2] = {4, -1};
        EXPECT(adam_chunk_count(neg, 2) == -1);
        EXPECT(adam_chunk_count(nullptr, 2) == -1 && adam_chunk_count(neg, -1) == -1);
        refusals += 3;
        const std::vector<int64_t> two = {100, 5000};
        Plan pl = make_plan(two, fake);
        const int32_t ns = 2;
        auto seg_bad = [&](AdamSegment s0) {
            std::vector<AdamSegment> segs = pl.segs;
            segs[0] = s0;
            ++refusals;
            return adam_check_segments(segs.data(), ns, pl.moment_floats) != nullptr;
        };
        const AdamSegment ok = pl.segs[0];
        EXPECT(seg_bad(AdamSegment{nullptr, ok.grad_off, ok.moment_off, ok.numel}));          // null parameter
        EXPECT(seg_bad(AdamSegment{ok.param, ok.grad_off, ok.moment_off, -1}));               // negative count
        EXPECT(seg_bad(AdamSegment{ok.param, ok.grad_off + 2, ok.moment_off, ok.numel}));     // gradient not on a float
        EXPECT(seg_bad(AdamSegment{ok.param, ok.grad_off, ok.moment_off + 1, ok.numel}));     // moment slice misaligned
        EXPECT(seg_bad(AdamSegment{ok.param, ok.grad_off, -64, ok.numel}));                   // ... before the buffers
        EXPECT(seg_bad(AdamSegment{ok.param, ok.grad_off, pl.moment_floats, ok.numel}));      // ... behind them
        EXPECT(seg_bad(AdamSegment{ok.param, ok.grad_off, ok.moment_off, pl.moment_floats + 1}));
        EXPECT(!seg_bad(AdamSegment{nullptr, ok.grad_off, ok.moment_off, 0}));                // (an empty tensor may have no address)
        EXPECT(!seg_bad(AdamSegment{ok.param, -4096, ok.moment_off, ok.numel}));              // (gradients may lie before the base)
        EXPECT(adam_check_segments(pl.segs.data(), ns, pl.segs[1].moment_off + pl.segs[1].numel) == nullptr);   // (the padding is not needed)
        EXPECT(adam_check_segments(pl.segs.data(), ns, pl.segs[1].moment_off + pl.segs[1].numel - 1) != nullptr);
        EXPECT(adam_check_segments(pl.segs.data(), ns, -1) != nullptr);
        refusals += 2;
        auto chunk_bad = [&](AdamChunk c) {
            std::vector<AdamChunk> ch = pl.chunks;
            ch.back() = c;
            ++refusals;
            return adam_check_chunks(pl.segs.data(), ns, ch.data(), (int64_t)ch.size()) != nullptr;
        };
        EXPECT(pl.chunks.size() == 3);
        EXPECT(chunk_bad(AdamChunk{0, 2, 0}));               // no such segment
        EXPECT(chunk_bad(AdamChunk{0, -1, 0}));
        EXPECT(chunk_bad(AdamChunk{kAdamChunk, 0, 0}));      // starts behind its segment's end (100 elements)
        EXPECT(chunk_bad(AdamChunk{2 * kAdamChunk, 1, 0}));  // ... (5000 elements)
        EXPECT(chunk_bad(AdamChunk{-kAdamChunk, 1, 0}));
        EXPECT(chunk_bad(AdamChunk{64, 1, 0}));              // not on a chunk boundary: would overlap its neighbour
        EXPECT(!chunk_bad(AdamChunk{kAdamChunk, 1, 0}));
        EXPECT(adam_check_chunks(pl.segs.data(), ns, pl.chunks.data(), -1) != nullptr);
        ++refusals;
    }
    printf("adam_plan_test: %ld plans, %ld chunks, %ld refusals, %ld failures\n", plans, chunks, refusals, g_failures);
    return g_failures ? 1 : 0;
}
