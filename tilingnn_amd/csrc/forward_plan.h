// Which schedule a forward takes, as a value: plain C++17, no HIP header, testable on the CPU (tests/host/forward_plan_test.cpp).
//
// forward.hip gathers ForwardFacts (model, layout, mode, hand-over records, the switches -- each read ONCE), plan_forward turns them
// into a ForwardPlan, and the phases of forward.hip only read the plan.  The three questions that need the device (the persistent
// kernels' capacity) stay behind a Probe; two of them count the fall-back window of forward_small.hip down, so every probe is
// called at most once and only under its guard.  The eligibility checks of tgnn_forward_begin / _begin_weights / _small_prepass --
// which run BEFORE the layout is known -- are the predicates at the end, built from the same sub-terms as the plan.
#pragma once
#include <stdint.h>

#include "gin64_plan.h"
#include "nnconv64_eg_plan.h"

namespace tgnn {

constexpr int kPlanMaxDepth = 64;      // == kMaxDepth (tgnn_common.h; forward.hip asserts it)
constexpr int kCarveTypes = 16;        // types the workspace's type-dependent pieces are carved for at least (forward.hip: carve); NOT
                                       // the matrix-core NNConv kernels' limit: tgnn_nnconv_cols_max_types() is 22
constexpr int kFinalWidth0 = 256;      // out width of the final MLP's first Linear (TilinGNN.py:46)

// bits of tgnn_set_lean_head
constexpr int kLeanHeadBit = 1, kLeanInitBit = 2, kLeanFoldFinalBit = 4;

struct ForwardFacts {
    // model
    int c = 0, D = 0, fx = 0, fe = 0;
    // layout
    int64_t n = 0, nr = 0;             // rows computed / rows of the gathered buffers (nr > n: halo rows of other shards)
    int T = 0, max_in_degree = 0;
    bool has_cols = false;             // nn_tile_col_ptr
    bool has_groups = false;           // nn_tile_grp_ptr && nn_grp
    bool has_mid_verdict = false;      // nn_mid_verdict
    // mode
    bool sharded = false;
    bool shard_fused_tables = false;   // send_idx_fused && recv_idx_fused
    bool shard_send_rows = false;      // send_row_ptr && send_row_slot
    int world = 0;
    bool keep = false;                 // training forward
    bool use_running_stats = false;
    bool init_running_done = false;    // bit 1 of update_running: the init MLP's running statistics have this forward's update already
    bool profiled = false, two_stream = false;
    bool head_done = false;            // tgnn_forward_resume
    bool distinct_side_stream = false; // the caller's second stream (the shard's side stream) exists and is not `stream`
    // hand-over records of this thread and device
    bool small_pre_match = false;      // tgnn_forward_small_prepass queued for this workspace and node count
    bool weights_early = false;        // tgnn_forward_begin_weights queued behind the matching tgnn_forward_begin
    bool edge_table_device_count_ok = false;   // edge_weight_table_device_count_ok(fe, c)
    int device_cus = 0;
    // switches
    int split_f16 = 1, nnconv_eg = 1, lean_head = 3;
    int nnconv64_eg = 0;               // tgnn_set_nnconv64_eg
    int gin64_mfma = 0;                // tgnn_set_gin64_mfma
    bool mid_init_in_kernel = false;
};

enum class ForwardPath { Small, Mid, MidTail, General };
enum class WeightsDoneWord { None, MidBounds, SmallCtr };   // the counter the persistent kernel polls instead of waiting for an event
enum class ScalesKernel { None, Begin, Lean, Full };        // Begin: tgnn_forward_begin has run it
enum class FinalOperands { None, Begin, Lean, Split };      // who takes the final MLP's bounds and builds its operand images

struct ForwardPlan {
    bool side = false;                 // the two-chain schedule: a side stream is used
    bool cols_ok = false, groups_ok = false;
    int small_teams = 0;
    int mid_k = 0, mid_blocks = 0, tail_k = 0, tail_blocks = 0;
    bool mid_counter = false, mid_init = false;
    bool verdict_refused = false;      // nn_mid_verdict given, but the forward is not the two persistent kernels alone
    bool f16 = false, eg = false, tiled = false, lean_head = false;
    bool eg64 = false;                 // width 64, fp32: the NNConv on edge groups (nnconv64_eg.hip) instead of the generic kernel
    bool gin64 = false;                // width 64, fp32: the GIN MLP on the matrix cores (gin64_mlp.hip) instead of the generic kernel
    bool init_fused_early = false, init_fused = false, head_used = false;
    bool weights_on_main = false, weights_queued = false, small_pre_used = false;
    WeightsDoneWord weights_done = WeightsDoneWord::None;
    bool weights_on_side = false;      // the edge weights (and the final MLP's operands) go on the side stream: sw == s2
    bool queue_weights = false;        // this forward launches the edge-weight kernel itself
    bool nn_first = false;             // layer 0: the NNConv's launch goes out before the collision chain's
    bool fold_fin2 = false, zero_fold_ctr = false, fold_final = false;
    bool fused_shard = false, split = false, pack_in_nnconv = false;
    bool fused_bn1_ok = false;         // merge derives the first BatchNorm's record itself where the partial rows are few enough
    bool init_stats_written = false;
    ScalesKernel scales = ScalesKernel::None;
    FinalOperands final_operands = FinalOperands::None;
    ForwardPath path = ForwardPath::General;
};

// ---- sub-terms shared by the plan and the early entry points ---------------------------------------------------------------
inline bool addr32_ok(int c, int64_t nr) { return c == 32 && nr * c * 4 < (int64_t(1) << 31); }   // buffer-addressed gathers
inline bool f16_model_ok(int c, int D, int split_f16) {
    return split_f16 && D <= kPlanMaxDepth && ((int64_t)c * (D + 1) * kFinalWidth0) % 4 == 0;
}
inline bool init_fused_model_ok(int c, int fx, int lean_bits) { return c == 32 && fx <= 8 && (lean_bits & kLeanInitBit); }
inline bool device_count_table_ok(int c, bool edge_table_device_count_ok) { return c == 32 && edge_table_device_count_ok; }
// the two-chain schedule: not in the one-stream profile, not for sharded widths other than 32 (forward.hip makes the chains' events
// from this alone, in front of the probes)
inline bool side_stream_used(const ForwardFacts &f) {
    return f.distinct_side_stream && !(f.profiled && !f.two_stream) && !(f.sharded && f.c != 32);
}

template <class Probe>
ForwardPlan plan_forward(const ForwardFacts &f, Probe &probe) {
    ForwardPlan p;
    const bool sh = f.sharded, keep = f.keep, urs = f.use_running_stats;
    const bool inference1 = !sh && !keep;                    // single device, nothing kept for a backward
    p.side = side_stream_used(f);
    const bool addr_ok = addr32_ok(f.c, f.nr);
    p.cols_ok = f.has_cols && addr_ok;
    p.groups_ok = f.has_groups && addr_ok && f.max_in_degree <= 2048 && f.nnconv_eg;
    // Small layouts: one persistent kernel (forward_small.hip) -- single device, inference, train-mode BatchNorm, not profiled
    const bool small_path_open = p.cols_ok && inference1 && !urs && !f.profiled && f.nr == f.n;
    p.small_teams = small_path_open ? probe.small_layout_teams() : 0;
    // fp16-pair operands wherever a bound of the operand is at hand: general schedule, train-mode BatchNorm, the layout's largest
    // in-degree known.  Sharded: only the one-all-to-all schemes (every shard merges its halo rows itself)
    p.fused_shard = sh && f.shard_fused_tables && f.world >= 1 && f.c == 32;
    p.f16 = f16_model_ok(f.c, f.D, f.split_f16) && (p.cols_ok || p.groups_ok) && (!sh || p.fused_shard) && !p.small_teams && !urs &&
            f.max_in_degree >= 1;
    // Mid-size layouts: the D layers as one persistent kernel (forward_mid.hip), the final MLP as one more (forward_tail.hip)
    p.mid_k = (p.f16 && inference1 && !f.profiled && f.nr == f.n) ? probe.mid_layout_tiles_per_block(&p.mid_blocks) : 0;
    p.tail_k = p.mid_k ? probe.mid_tail_tiles_per_block(&p.tail_blocks) : 0;
    p.path = p.small_teams ? ForwardPath::Small : !p.mid_k ? ForwardPath::General : p.tail_k ? ForwardPath::MidTail : ForwardPath::Mid;
    p.eg = p.f16 && p.groups_ok && !p.mid_k;
    p.tiled = p.cols_ok || p.eg;
    // width 64 (general schedule, nothing above applies): the NNConv alone changes kernels, everything else stays as it is
    p.eg64 = nnconv64_eg_ok(f.c, sh, f.has_groups, f.nr, f.T, f.max_in_degree, urs, f.nnconv64_eg);
    p.gin64 = gin64_mfma_ok(f.c, sh, f.gin64_mfma);           // (either BatchNorm mode: the kernel needs no bound of its operand)
    // the persistent kernels, with CUs to spare for the edge-weight kernel's blocks, wait for the edge weights on a counter of that
    // kernel's finished blocks instead of the host's event
    p.mid_counter = p.mid_k && p.mid_blocks + 16 <= f.device_cus && p.side;
    p.mid_init = p.mid_counter && f.mid_init_in_kernel && f.fx <= 8;
    p.verdict_refused = p.mid_k && f.has_mid_verdict && !(p.mid_init && p.tail_k);
    p.small_pre_used = f.small_pre_match && !f.head_done && inference1 && p.small_teams && f.T <= kCarveTypes && p.cols_ok &&
                       device_count_table_ok(f.c, f.edge_table_device_count_ok);
    p.weights_done = p.mid_counter                                      ? WeightsDoneWord::MidBounds
                     : (p.small_teams == 2 && p.side && !p.small_pre_used) ? WeightsDoneWord::SmallCtr
                                                                           : WeightsDoneWord::None;
    // the general schedule's head without memsets; the init MLP's fused form; tgnn_forward_begin's work is used iff both hold
    p.lean_head = p.f16 && !p.mid_k && !p.small_teams && (f.lean_head & kLeanHeadBit);
    p.init_fused_early = init_fused_model_ok(f.c, f.fx, f.lean_head) && inference1 && !urs;
    p.head_used = f.head_done && p.lean_head && p.init_fused_early;
    p.scales = !p.f16 ? ScalesKernel::None : p.head_used ? ScalesKernel::Begin : p.lean_head ? ScalesKernel::Lean : ScalesKernel::Full;
    // tgnn_forward_resume picking up tgnn_forward_begin's work: the edge weights go on the main stream, behind the preparation
    p.weights_on_main = p.head_used && p.side && inference1 && !p.mid_k && !p.small_teams;
    p.weights_on_side = !p.small_pre_used && !p.weights_on_main && p.side;
    p.weights_queued = f.weights_early && p.weights_on_main && p.eg && f.T <= kCarveTypes && p.weights_done == WeightsDoneWord::None &&
                       f.edge_table_device_count_ok;
    p.queue_weights = (f.T > 0 || p.tiled) && !p.weights_queued && !p.small_pre_used;
    p.nn_first = p.weights_on_main;
    p.final_operands = p.head_used                ? FinalOperands::Begin
                       : p.lean_head              ? FinalOperands::Lean
                       : (p.f16 && !p.tail_k)     ? FinalOperands::Split
                                                  : FinalOperands::None;
    p.init_fused = !p.mid_init && p.init_fused_early;
    p.init_stats_written = (f.head_done && !p.head_used) || (f.init_running_done && !urs);
    p.split = p.fused_shard && p.side;
#ifdef TGNN_ABL_NOFOLD
    p.fold_fin2 = false;
#else
    p.fold_fin2 = f.c == 32 && !sh && !urs;                  // the collision branch's BatchNorm record by the GIN MLP's last block
#endif
    p.zero_fold_ctr = p.fold_fin2 && !p.mid_k && !p.lean_head;
    p.pack_in_nnconv = p.eg && p.split && f.shard_send_rows && p.lean_head;
    p.fused_bn1_ok = f.c == 32 && !urs && !sh;
    p.fold_final = p.lean_head && !sh && !urs && f.c == 32 && (f.lean_head & kLeanFoldFinalBit);
    return p;
}

// ---- the early entry points: what can be known before the layout is prepared -----------------------------------------------
// tgnn_forward_begin: a forward that takes the lean head AND the fused init MLP if its layout then takes the fp16-pair general
// schedule (above both persistent kernels' limits; the edge groups / columns and the in-degree are tgnn_forward_resume's to check)
inline bool head_early_ok(int c, int D, int fx, bool distinct_side_stream, int split_f16, int lean_bits, int64_t n, int64_t small_limit,
                          int64_t mid_limit) {
    return distinct_side_stream && init_fused_model_ok(c, fx, lean_bits) && f16_model_ok(c, D, split_f16) && (lean_bits & kLeanHeadBit) &&
           n > mid_limit && n > small_limit;
}
// tgnn_forward_begin_weights: the device-counted edge weights with the edge-group kernel's images, behind a matching begin
inline bool weights_early_ok(bool head_match, int c, bool edge_table_device_count_ok, int nnconv_eg, int split_f16) {
    return head_match && device_count_table_ok(c, edge_table_device_count_ok) && nnconv_eg && split_f16;
}
// tgnn_forward_small_prepass: the device-counted edge weights with the column kernel's images, in front of the small-layout kernel
inline bool small_prepass_ok(int c, int64_t n, int64_t small_limit, bool edge_table_device_count_ok) {
    return device_count_table_ok(c, edge_table_device_count_ok) && n >= 2 && n <= small_limit;
}

}  // namespace tgnn
