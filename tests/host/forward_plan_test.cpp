// Stand-alone check of tilingnn_amd/csrc/forward_plan.h: plan_forward over the cross product of its facts with a fake Probe, the
// plan's invariants asserted on every combination.  No device, no HIP header:
//   g++ -std=c++17 -O1 -fsanitize=address,undefined -I include -I tilingnn_amd/csrc tests/host/forward_plan_test.cpp
// (tests/test_abi_and_host.py builds and runs it).
#include <stdio.h>
#include <stdlib.h>

#include <initializer_list>

#include "forward_plan.h"

using namespace tgnn;

constexpr int64_t kSmallLimit = 4096, kMidLimit = 32768;     // the library's defaults (tgnn_get_small / mid_layout_limit)

// what the device would answer if asked; counts the questions
struct FakeProbe {
    int small = 0, mid_k = 0, mid_blocks = 0, tail_k = 0;
    int small_calls = 0, mid_calls = 0, tail_calls = 0;
    int small_layout_teams() { ++small_calls; return small; }
    int mid_layout_tiles_per_block(int *blocks) { ++mid_calls; if (mid_k) *blocks = mid_blocks; return mid_k; }
    int mid_tail_tiles_per_block(int *blocks) { ++tail_calls; if (tail_k) *blocks = 128; return tail_k; }
};

static long g_failures = 0;
static void fail(const char *what, const ForwardFacts &f, const FakeProbe &pr) {
    if (++g_failures > 20) return;
    fprintf(stderr,
            "FAILED: %s\n  c %d D %d fx %d fe %d n %lld nr %lld T %d deg %d cols %d groups %d verdict %d | sharded %d fused %d rows %d world %d keep %d "
            "urs %d init_done %d prof %d two %d head_done %d side %d | small_pre %d weights_early %d count_ok %d cus %d | f16 %d eg %d "
            "lean %d mid_init %d | probe small %d mid %d/%d tail %d\n",
            what, f.c, f.D, f.fx, f.fe, (long long)f.n, (long long)f.nr, f.T, f.max_in_degree, f.has_cols, f.has_groups, f.has_mid_verdict,
            f.sharded, f.shard_fused_tables, f.shard_send_rows, f.world, f.keep, f.use_running_stats, f.init_running_done,
            f.profiled, f.two_stream, f.head_done, f.distinct_side_stream, f.small_pre_match, f.weights_early, f.edge_table_device_count_ok,
            f.device_cus, f.split_f16, f.nnconv_eg, f.lean_head, f.mid_init_in_kernel, pr.small, pr.mid_k, pr.mid_blocks, pr.tail_k);
}
#define EXPECT(cond)                      \
    do {                                  \
        if (!(cond)) fail(#cond, f, pr);  \
    } while (0)
#define IMPLIES(a, b) EXPECT(!(a) || (b))

static void check(const ForwardFacts &f, const FakeProbe &pr, const ForwardPlan &p) {
    // one path, and it is what the team / tile counts say
    EXPECT((p.path == ForwardPath::Small) == (p.small_teams != 0));
    EXPECT((p.path == ForwardPath::Mid) == (p.mid_k != 0 && p.tail_k == 0));
    EXPECT((p.path == ForwardPath::MidTail) == (p.mid_k != 0 && p.tail_k != 0));
    EXPECT((p.path == ForwardPath::General) == (p.small_teams == 0 && p.mid_k == 0));
    IMPLIES(p.small_teams, !p.mid_k);
    // the chains of implications
    IMPLIES(p.weights_queued, p.weights_on_main);
    IMPLIES(p.weights_on_main, p.head_used);
    IMPLIES(p.head_used, p.lean_head);
    IMPLIES(p.lean_head, p.f16);
    IMPLIES(p.mid_init, p.mid_counter);
    IMPLIES(p.mid_counter, p.mid_k);
    IMPLIES(p.eg, !p.mid_k && f.has_groups);
    IMPLIES(p.tail_k, p.mid_k);
    IMPLIES(p.small_pre_used, p.small_teams);
    IMPLIES(f.sharded || f.keep || f.use_running_stats, !p.head_used && !p.weights_on_main && !p.weights_queued && !p.small_pre_used);
    // streams: the side stream is used only where there is one; the edge weights have one home
    IMPLIES(p.weights_on_side || p.weights_on_main || p.split || p.mid_counter || p.nn_first, p.side);
    IMPLIES(p.weights_on_side, !p.weights_on_main && !p.small_pre_used);
    IMPLIES(p.weights_queued || p.small_pre_used, !p.queue_weights);
    EXPECT((p.weights_done == WeightsDoneWord::MidBounds) == p.mid_counter);
    IMPLIES(p.weights_done == WeightsDoneWord::SmallCtr, p.small_teams == 2 && !p.small_pre_used);
    // schemes
    IMPLIES(p.split, p.fused_shard);
    IMPLIES(p.fused_shard, f.sharded);
    IMPLIES(p.pack_in_nnconv, p.split && p.eg && f.shard_send_rows);
    IMPLIES(p.fold_final, p.lean_head);
    IMPLIES(p.verdict_refused, p.mid_k && f.has_mid_verdict);
    EXPECT((p.scales == ScalesKernel::None) == !p.f16);
    EXPECT((p.scales == ScalesKernel::Begin) == p.head_used);
    EXPECT((p.final_operands == FinalOperands::Begin) == p.head_used);
    IMPLIES(p.init_fused, p.init_fused_early && !p.mid_init);
    // each probe at most once, and never outside its guard
    const bool cols = f.has_cols && f.c == 32 && f.nr * f.c * 4 < (int64_t(1) << 31);
    const bool single_plain = !f.sharded && !f.keep && !f.profiled && f.nr == f.n;
    EXPECT(pr.small_calls == ((cols && single_plain && !f.use_running_stats) ? 1 : 0));
    EXPECT(pr.mid_calls == ((p.f16 && single_plain) ? 1 : 0));
    EXPECT(pr.tail_calls == (p.mid_k ? 1 : 0));
    // the early entry points promise what the plan then does.  A forward that can follow them: tgnn_forward_resume (head_done) /
    // a plain tgnn_forward behind tgnn_forward_small_prepass -- single device, train-mode BatchNorm, not profiled
    const bool plain = !f.sharded && !f.keep && !f.use_running_stats && !f.profiled;
    const bool begin_ok = head_early_ok(f.c, f.D, f.fx, f.distinct_side_stream, f.split_f16, f.lean_head, f.n, kSmallLimit, kMidLimit);
    if (plain && f.head_done && begin_ok && p.f16 && p.path == ForwardPath::General) {
        EXPECT(p.head_used);
        EXPECT(p.weights_on_main);
        // (tgnn_forward_begin_weights checks the record's match itself; the rest of its condition:)
        if (f.weights_early && weights_early_ok(true, f.c, f.edge_table_device_count_ok, f.nnconv_eg, f.split_f16) && p.eg && f.T <= kCarveTypes)
            EXPECT(p.weights_queued);
    }
    IMPLIES(p.weights_queued, weights_early_ok(true, f.c, f.edge_table_device_count_ok, f.nnconv_eg, f.split_f16));
    IMPLIES(p.head_used, init_fused_model_ok(f.c, f.fx, f.lean_head) && f16_model_ok(f.c, f.D, f.split_f16));
    if (plain && !f.head_done && f.small_pre_match && small_prepass_ok(f.c, f.n, kSmallLimit, f.edge_table_device_count_ok) &&
        p.path == ForwardPath::Small && f.T <= kCarveTypes)
        EXPECT(p.small_pre_used);
    IMPLIES(p.small_pre_used, device_count_table_ok(f.c, f.edge_table_device_count_ok));
}

// Calls fn(facts, probe) -- fn runs plan_forward on them -- for every combination.  The probes' answers are varied only where the
// probe was asked (whether it is asked does not depend on its own answer).
template <class Fn>
static long enumerate(Fn fn) {
    long count = 0;
    struct Mode { bool sharded, fused, rows, keep, urs, profiled, two_stream, head_done, weights_early; };
    const Mode modes[] = {
        {0, 0, 0, 0, 0, 0, 0, 0, 0},   // tgnn_forward
        {0, 0, 0, 0, 0, 0, 0, 1, 0},   // tgnn_forward_resume
        {0, 0, 0, 0, 0, 0, 0, 1, 1},   //   behind tgnn_forward_begin_weights
        {0, 0, 0, 0, 1, 0, 0, 0, 0},   // eval mode
        {0, 0, 0, 0, 0, 1, 0, 0, 0},   // profiled
        {0, 0, 0, 0, 1, 1, 0, 0, 0},
        {0, 0, 0, 0, 0, 1, 1, 0, 0},   // profiled, two streams
        {0, 0, 0, 1, 0, 0, 0, 0, 0},   // training forward
        {1, 0, 0, 0, 0, 0, 0, 0, 0},   // sharded: all-reduce + all-to-all
        {1, 0, 1, 0, 0, 0, 0, 0, 0},
        {1, 1, 0, 0, 0, 0, 0, 0, 0},   // sharded: one all-to-all (fused / split)
        {1, 1, 1, 0, 0, 0, 0, 0, 0},
        // what no entry point passes today, but the plan must still answer consistently
        {0, 0, 0, 1, 0, 0, 0, 1, 1},
        {1, 1, 1, 0, 0, 0, 0, 1, 1},
        {0, 0, 0, 0, 1, 0, 0, 1, 1},
    };
    const int64_t ns[] = {300, 8192, 100000};
    const int cs[] = {32, 64}, fxs[] = {3, 9}, Ts[] = {0, 13, 17}, Ds[] = {4, 20, 65}, degs[] = {0, 8, 4096};
    const int smalls[] = {2, 1, 0}, tails[] = {3, 0};
    const int mids[][2] = {{2, 100}, {2, 250}, {0, 0}};   // (tiles per block, blocks): CUs to spare for the edge-weight kernel or not
    for (const Mode &m : modes)
    for (int bits = 0; bits < 128; ++bits)
    for (int c : cs) for (int fx : fxs) for (int T : Ts) for (int D : Ds) for (int deg : degs) for (int64_t n : ns)
    for (int sw = 0; sw < 16; ++sw) {
        ForwardFacts f;
        f.c = c; f.D = D; f.fx = fx; f.fe = 15; f.n = n; f.nr = m.sharded ? n + 100 : n; f.T = T; f.max_in_degree = deg;
        f.has_cols = bits & 1; f.has_groups = bits & 2; f.has_mid_verdict = bits & 4; f.distinct_side_stream = bits & 8;
        f.small_pre_match = bits & 16; f.edge_table_device_count_ok = bits & 32; f.init_running_done = bits & 64;
        f.sharded = m.sharded; f.shard_fused_tables = m.fused; f.shard_send_rows = m.rows; f.world = m.sharded ? 2 : 0;
        f.keep = m.keep; f.use_running_stats = m.urs; f.profiled = m.profiled; f.two_stream = m.two_stream;
        f.head_done = m.head_done; f.weights_early = m.weights_early;
        f.device_cus = 256;
        f.split_f16 = sw & 1; f.nnconv_eg = (sw >> 1) & 1; f.lean_head = (sw & 4) ? 3 : 0; f.mid_init_in_kernel = (sw & 8) != 0;
        for (int small : smalls) {
            bool small_asked = false;
            for (const int *mid : mids) {
                bool mid_asked = false;
                for (int tail : tails) {
                    FakeProbe pr;
                    pr.small = small; pr.mid_k = mid[0]; pr.mid_blocks = mid[1]; pr.tail_k = tail;
                    fn(f, pr);
                    ++count;
                    small_asked = pr.small_calls > 0; mid_asked = pr.mid_calls > 0;
                    if (!pr.tail_calls) break;
                }
                if (!mid_asked) break;
            }
            if (!small_asked) break;
        }
    }
    // the other values of tgnn_set_lean_head (1: lean head alone, 2: fused init MLP alone, 7: + the final MLP's folded records)
    for (int lean : {1, 2, 7})
    for (const Mode &m : modes)
    for (int bits = 0; bits < 64; ++bits)
    for (int64_t n : ns) for (int deg : degs) for (int T : Ts) {
        ForwardFacts f;
        f.c = 32; f.D = 20; f.fx = 3; f.fe = 15; f.n = n; f.nr = m.sharded ? n + 100 : n; f.T = T; f.max_in_degree = deg;
        f.has_cols = bits & 1; f.has_groups = bits & 2; f.has_mid_verdict = bits & 4; f.distinct_side_stream = bits & 8;
        f.small_pre_match = bits & 16; f.edge_table_device_count_ok = bits & 32;
        f.sharded = m.sharded; f.shard_fused_tables = m.fused; f.shard_send_rows = m.rows; f.world = m.sharded ? 2 : 0;
        f.keep = m.keep; f.use_running_stats = m.urs; f.profiled = m.profiled; f.two_stream = m.two_stream;
        f.head_done = m.head_done; f.weights_early = m.weights_early;
        f.device_cus = 256; f.lean_head = lean; f.mid_init_in_kernel = true;
        for (int small : {2, 0}) for (int mid : {2, 0}) {
            FakeProbe pr;
            pr.small = small; pr.mid_k = mid; pr.mid_blocks = 100; pr.tail_k = 3;
            fn(f, pr);
            ++count;
        }
    }
    return count;
}

#ifndef FORWARD_PLAN_TEST_NO_MAIN
int main() {
    const long count = enumerate([](const ForwardFacts &f, FakeProbe &pr) { check(f, pr, plan_forward(f, pr)); });
    printf("forward_plan_test: %ld combinations, %ld failures\n", count, g_failures);
    return g_failures ? 1 : 0;
}
#endif
