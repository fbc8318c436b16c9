"""The operand bounds every forward path leaves in the workspace (include/tgnn.h: tgnn_forward_workspace_map documents the words).

The default forward is fp32-accurate on 16-bit matrix instructions because it runs fp16 PAIRS (csrc/tgnn_common.h: split2_f16), and
that holds only while every operand is scaled by a power of two taken from a bound of its magnitude.  The bounds are device words
written by a dozen producers (init_apply_kernel, bn_apply_kernel, the four merge kernels, absmax_kernel over halo rows, the two scales
kernels, dense_bounds_kernel, the mid-size persistent kernel's prologue and per-layer epilogue); the op-level tests of their consumers
compute the true maximum themselves, and a whole forward does not notice a word that is 2 x off.  Here the words are read back:
atomicMax over exact floats is exact whatever the order, so after a forward word k IS the bit pattern of max |slot k| of the same
workspace -- integer equality, no tolerance.

Where the maximum lies: tests/bounds_cases.py (one row far outside the others: row 0, the last row, the one before it, of an odd row
count; tests/test_forward_bounds_host.py shows with the fp64 oracle that slots 0 and 1 peak there).  A producer that skips its ragged
tail or its last block then leaves a word that is too small.  Reused workspace: a forward of a network whose slots are ~2^12 larger,
then the plain network on the SAME workspace -- a word that is only ever raised fails the second check.

Measured error columns of the consumers at those magnitudes (fp16 pairs against bf16 x 3): profiles/forward_bounds_errors.txt."""
import contextlib
import ctypes as C
import math

import pytest
import torch

from oracle import tilingnn_oracle as orc
from tests import bounds_cases as bc
from tests.test_hip_parity import make_net, run_thread_ranks

pytestmark = pytest.mark.gpu

D = bc.DEPTH
_ERROR_ROWS = []


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "GPU tests need a GPU"
    return torch.device("cuda:0")


@pytest.fixture(scope="module", autouse=True)
def error_table():
    yield
    if _ERROR_ROWS:
        print("\ncase                      slot   fp16 pairs   bf16 x 3    ratio    (max |slot - slot_fp64| / max |slot_fp64|, x 64 network)")
        for row in _ERROR_ROWS:
            print("%-25s %4d   %10.3e  %10.3e  %6.2f" % row)


@contextlib.contextmanager
def switch(setter, value):
    """A library switch (tgnn_set_*: returns the value before, -1 asks) for the length of the block."""
    from tilingnn_amd._lib import lib
    before = getattr(lib, setter)(value)
    try:
        yield
    finally:
        getattr(lib, setter)(before)


def _bits(v):
    return int(v.float().reshape(1).view(torch.int32))


def _word_float(word):
    return float(torch.tensor([word], dtype=torch.int32).view(torch.float32))


def _tensors(sg, dev):
    return sg.to_torch(dev)[:4]


def _net_from(sd, dev, depth=D, width=32):
    from tilingnn_amd import TilinGNN
    net = TilinGNN(adj_edge_features_dim=15, network_depth=depth, network_width=width, node_features_dim=3)
    net.load_state_dict(sd, strict=True)
    return net.to(dev).train()


def _prepared(net, inputs, n, dev, columns=False):
    """(graph, its C struct for this width, the workspace map, workspace bytes)"""
    from tilingnn_amd import _lib, ops
    _, adj, attr, col = inputs
    graph = ops.prepare_graph(n, adj, attr, col)
    if columns:
        graph.ensure_columns()
    g = ops.c_struct_for_width(graph, net.network_width)
    dims = net._dims()
    return graph, g, _lib.forward_workspace_map(dims, n, n, graph.n_types), int(_lib.lib.tgnn_forward_workspace_bytes(C.byref(dims), n, graph.n_types))


def _forward(net, inputs, n, dev, ws=None, columns=False, path=None):
    """tgnn_forward on `ws` (None: a fresh zeroed workspace -- the persistent kernels' counters are not this test's subject), synchronised.
    path: index into tgnn_forward_path_counts (0 general, 2 mid-size) this forward must take.  Returns (workspace, map, graph)."""
    from tilingnn_amd import _lib, ops
    graph, g, m, ws_bytes = _prepared(net, inputs, n, dev, columns)
    if ws is None:
        ws = torch.zeros(ws_bytes, dtype=torch.uint8, device=dev)
    assert ws.numel() == ws_bytes
    dims = net._dims()
    table, _ = net._param_table()
    probs = torch.empty(n, 1, device=dev)
    c0 = _lib.forward_path_counts()
    _lib.check(_lib.lib.tgnn_forward(C.byref(dims), table, ops.ptr(inputs[0]), ops.ptr(inputs[2]), C.byref(g), 0, 0, ops.ptr(probs), ops.ptr(ws),
                                    ws_bytes, _lib.current_stream(dev), _lib.side_stream(dev)))
    torch.cuda.synchronize()
    c1 = _lib.forward_path_counts()
    if path is not None:
        assert tuple(b - a for a, b in zip(c0, c1)) == tuple(int(k == path) for k in range(3)), (c0, c1)
    code = C.c_uint32(0)
    _lib.check(_lib.lib.tgnn_spin_error_poll(_lib.current_stream(dev), C.byref(code)))
    assert code.value == 0
    assert bool(torch.isfinite(probs).all())
    return ws, m, graph


def _slots(ws, m, nr, depth, c=32):
    return ws[m["mid"]: m["mid"] + (depth + 1) * nr * c * 4].view(torch.float32).view(depth + 1, nr, c)


def _words(ws, m, depth):
    return ws[m["bounds"]: m["bounds"] + (2 * depth + 100) * 4].view(torch.int32).cpu().tolist()


def assert_bounds(ws, m, net, n, nr, depth, inner=(1, 2), zero=(), n_total=None, populations=None):
    """Every bound word of `ws` behind a forward of `net` over n own rows of nr gathered ones, bit for bit against what it bounds.
    inner: the final MLP's layers whose (max |W_l|, bound of |BN(input)|) pair this path takes; zero: words the path clears and does
    not write; populations[l]: the rows of ALL shards the BatchNorm in front of layer l normalises with (None: this workspace's)."""
    sd = net.state_dict()
    w = _words(ws, m, depth)
    slots = _slots(ws, m, nr, depth)
    n_total = n_total or n
    for k in range(depth + 1):
        # every row a consumer gathers: the halo rows too, except those of the last slot (sharded: nobody reads or writes them)
        rows = nr if k < depth else n
        assert w[k] == _bits(slots[k, :rows].abs().max()), ("slot", k, _word_float(w[k]), float(slots[k, :rows].abs().max()))
    for i in range(depth):
        root = sd[f"brch_1_graph_conv_layers.{i}.nnConv.root"]
        assert root.numel() == 1024 and w[depth + 1 + i] == _bits(root.abs().max()), ("root", i)
    assert w[2 * depth + 1] == _bits(sd["final_mlp.0.mlp.0.linear.weight"].abs().max()), "max |W_0| of the final MLP"
    for l in inner:
        at = 2 * depth + 2 + 2 * (l - 1) if l <= 2 else 2 * depth + 8
        assert w[at] == _bits(sd[f"final_mlp.0.mlp.{l}.linear.weight"].abs().max()), ("max |W_l|", l)
        width = (256, 128, 64)[l - 1]
        f = ws[m[f"f{l}"]: m[f"f{l}"] + n * width * 4].view(torch.float32).view(n, width).double()
        pop = f if populations is None else populations[l]
        gamma = sd[f"final_mlp.0.mlp.{l - 1}.batch_norm.weight"].double()
        beta = sd[f"final_mlp.0.mlp.{l - 1}.batch_norm.bias"].double()
        mean, var = pop.mean(dim=0), pop.var(dim=0, unbiased=False)
        need = float(((f - mean) / torch.sqrt(var + 1e-5) * gamma + beta).abs().max())
        upper = float((gamma.abs() * math.sqrt(n_total) + beta.abs()).max()) * 1.001    # the formula dense_bounds_kernel states
        got = _word_float(w[at + 1])
        assert need <= got <= upper, ("bound of |BN(input of l)|", l, need, got, upper)
    for at in zero:
        assert w[at] == 0, ("cleared and unwritten", at, w[at])
    return w


def _fresh_f_population(ws, m, n, l):
    width = (256, 128, 64)[l - 1]
    return ws[m[f"f{l}"]: m[f"f{l}"] + n * width * 4].view(torch.float32).view(n, width).double()


def _lean_defaults():
    from tilingnn_amd._lib import lib
    assert (lib.tgnn_set_lean_head(-1), lib.tgnn_set_nnconv_eg(-1), lib.tgnn_set_split_precision(-1)) == (3, 1, 1)


def _assert_peak(slots, r_star, ks=(0, 1)):
    """The precondition of the peak layouts: the slot's largest magnitude lies in row r_star."""
    for k in ks:
        assert int(slots[k].abs().max(dim=1).values.argmax()) == r_star, ("the maximum of slot", k, "is not in row", r_star)


# ---- (a) general schedule, default switches: forward_scales_store_kernel, init_apply_kernel, merge_bn1_kernel ----------------------
@pytest.mark.parametrize("r_star", (None,) + bc.PEAK_ROWS)
def test_general_schedule_default_switches(dev, general_schedule, r_star):
    """Lean head, fused init MLP, NNConv on edge groups; n = 1 237 rows = 9 896 float4 + 1 block of 168: the last block of
    merge_bn1_kernel is ragged and the last tile has 5 rows.  r_star: the row the maxima of slots 0 and 1 lie in."""
    n = bc.N_PEAK
    _lean_defaults()
    inputs = _tensors(bc.plain_layout(n) if r_star is None else bc.peak_layout(r_star), dev)
    net, _ = make_net(dev, depth=D)
    ws, m, graph = _forward(net, inputs, n, dev, path=0)
    assert graph.groups is not None and 1 <= graph.max_in_degree <= 2048 and graph.n_types <= 16     # plan: eg, f16, lean head
    if r_star is not None:
        _assert_peak(_slots(ws, m, n, D), r_star)
    assert_bounds(ws, m, net, n, n, D, inner=(1, 2), zero=(2 * D + 6, 2 * D + 7, 2 * D + 8, 2 * D + 9))


def test_maximum_in_the_last_float4_of_a_blocks_stride(dev, general_schedule):
    """merge_bn1_kernel at 1 237 rows: 39 blocks of 256 threads, one float4 each.  A network whose slot 1 is zero outside channels
    28 .. 31 and a layout whose slot 1 peaks in row 31: the maximum is thread 255's of block 0."""
    n, r_star = bc.N_PEAK, bc.BLOCK_END_ROW
    _lean_defaults()
    inputs = _tensors(bc.peak_layout(r_star, column=0), dev)
    _, sd = make_net(dev, depth=D)
    net = _net_from(bc.last_float4_state_dict(sd), dev)
    ws, m, graph = _forward(net, inputs, n, dev, path=0)
    assert graph.groups is not None
    slot1 = _slots(ws, m, n, D)[1]
    _assert_peak(_slots(ws, m, n, D), r_star)
    assert float(slot1[:, :28].abs().max()) == 0.0 and (8 * r_star + 7) % 256 == 255
    assert_bounds(ws, m, net, n, n, D, inner=(1, 2), zero=(2 * D + 6, 2 * D + 7, 2 * D + 8, 2 * D + 9))


# ---- (b) the merge's two kernels on each side of 128 NNConv partial rows -----------------------------------------------------------
def _nnconv_eg_blocks(n, cus):
    """launch_nnconv_eg's block count (csrc/nnconv_eg.hip) = the NNConv's partial rows: 4 tiles of 16 rows per block, at most the
    device's compute units less 32, a multiple of 8 from 8 on."""
    blocks = min(((n + 15) // 16 + 3) // 4, cus - 32)
    return max(blocks & ~7 if blocks >= 8 else blocks, 1)


@pytest.mark.parametrize("n,wide", [(8640, False), (8641, True)])
def test_merge_kernels_on_each_side_of_the_partial_row_threshold(dev, general_schedule, n, wide):
    """launch_merge_bn1 takes merge_bn1_wide_kernel from 129 partial rows on: 8 640 rows are 135 -> 128 NNConv blocks, 8 641 rows 136."""
    _lean_defaults()
    cus = torch.cuda.get_device_properties(dev).multi_processor_count
    assert cus >= 168, "fewer compute units than the block counts this case is cut for"
    np1 = _nnconv_eg_blocks(n, cus)
    assert (np1 > 128) == wide and np1 in (128, 136)
    inputs = _tensors(bc.plain_layout(n), dev)
    net, _ = make_net(dev, depth=D)
    ws, m, graph = _forward(net, inputs, n, dev, path=0)
    assert graph.groups is not None
    assert_bounds(ws, m, net, n, n, D, inner=(1, 2), zero=(2 * D + 6, 2 * D + 7, 2 * D + 8, 2 * D + 9))


# ---- (c) tgnn_set_lean_head(0): memset + forward_scales_kernel (32 dense blocks), bn_apply_kernel for slot 0, FinalOperands::Split -
@pytest.mark.parametrize("r_star", (None, bc.N_PEAK - 1))
def test_launch_per_op_head(dev, general_schedule, r_star):
    n = bc.N_PEAK
    inputs = _tensors(bc.plain_layout(n) if r_star is None else bc.peak_layout(r_star), dev)
    net, _ = make_net(dev, depth=D)
    with switch("tgnn_set_lean_head", 0):
        ws, m, graph = _forward(net, inputs, n, dev, path=0)
    if r_star is not None:
        _assert_peak(_slots(ws, m, n, D), r_star)
    # plan: ScalesKernel::Full clears [0, 2 D + 7) and takes max |W_0| itself; Split takes the pairs of layers 1 and 2
    assert_bounds(ws, m, net, n, n, D, inner=(1, 2), zero=(2 * D + 6,))


# ---- (d) tgnn_set_nnconv_eg(0): the column NNConv is the consumer -------------------------------------------------------------------
def test_column_nnconv_as_the_consumer(dev, general_schedule):
    n = bc.N_PEAK
    inputs = _tensors(bc.peak_layout(n - 2), dev)
    net, _ = make_net(dev, depth=D)
    with switch("tgnn_set_nnconv_eg", 0):
        ws, m, graph = _forward(net, inputs, n, dev, columns=True, path=0)
    assert graph.cols is not None
    _assert_peak(_slots(ws, m, n, D), n - 2)
    assert_bounds(ws, m, net, n, n, D, inner=(1, 2), zero=(2 * D + 6, 2 * D + 7, 2 * D + 8, 2 * D + 9))


# ---- (e) rows-per-wave final MLP: nl == 4 from 49 152 rows on (words 2 D + 8, 2 D + 9) ---------------------------------------------
@pytest.mark.parametrize("n", [49152, 49151])
def test_resident_final_mlp_takes_the_fourth_pair(dev, general_schedule, n):
    depth = 2
    _lean_defaults()
    inputs = _tensors(bc.plain_layout(n), dev)
    net, _ = make_net(dev, depth=depth)
    ws, m, graph = _forward(net, inputs, n, dev, path=0)
    assert graph.groups is not None
    if n >= 49152:                                               # kDenseRowsKernelMin (csrc/tgnn_common.h)
        w = assert_bounds(ws, m, net, n, n, depth, inner=(1, 2, 3), zero=(2 * depth + 6, 2 * depth + 7))
        assert w[2 * depth + 8] != 0 and w[2 * depth + 9] != 0
    else:
        assert_bounds(ws, m, net, n, n, depth, inner=(1, 2), zero=(2 * depth + 6, 2 * depth + 7, 2 * depth + 8, 2 * depth + 9))


# ---- (f) tgnn_forward_begin + tgnn_forward_resume (ScalesKernel::Begin) ------------------------------------------------------------
def test_begin_and_resume_leave_the_plain_forwards_words(dev, general_schedule):
    from tilingnn_amd import _lib, ops
    n = bc.N_PEAK
    _lean_defaults()
    inputs = _tensors(bc.peak_layout(n - 1), dev)
    net, _ = make_net(dev, depth=D)
    ws_plain, m, _ = _forward(net, inputs, n, dev, path=0)
    want = assert_bounds(ws_plain, m, net, n, n, D, inner=(1, 2), zero=(2 * D + 6, 2 * D + 7, 2 * D + 8, 2 * D + 9))
    # the module's calling convention (TilinGNN._forward_one): the side stream behind the current one, begin on it with a workspace carved
    # for 0 types, the preparation, resume on the same workspace
    dims = net._dims()
    table, _ = net._param_table()
    assert net.network_width == 32 and net.node_features_dim <= 8          # plan: init_fused_early; with the lean head: head_used
    side = _lib.side_stream_torch(dev)
    assert side is not None, "no side stream: tgnn_forward_begin does not apply"
    ws_bytes = int(_lib.lib.tgnn_forward_workspace_bytes(C.byref(dims), n, 0))
    ws = torch.zeros(ws_bytes, dtype=torch.uint8, device=dev)
    side.wait_stream(torch.cuda.current_stream(dev))
    _lib.check(_lib.lib.tgnn_forward_begin(C.byref(dims), table, ops.ptr(inputs[0]), n, 0, ops.ptr(ws), ws_bytes, None, _lib.side_stream(dev)))
    graph = ops.prepare_graph(n, *inputs[1:])
    assert graph.n_types <= 16 and int(_lib.lib.tgnn_forward_workspace_bytes(C.byref(dims), n, graph.n_types)) == ws_bytes
    g = graph.c_struct()
    probs = torch.empty(n, 1, device=dev)
    c0 = _lib.forward_path_counts()
    _lib.check(_lib.lib.tgnn_forward_resume(C.byref(dims), table, ops.ptr(inputs[0]), ops.ptr(inputs[2]), C.byref(g), 0, ops.ptr(probs),
                                           ops.ptr(ws), ws_bytes, _lib.current_stream(dev), _lib.side_stream(dev)))
    torch.cuda.synchronize()
    assert _lib.forward_path_counts()[0] == c0[0] + 1
    got = assert_bounds(ws, m, net, n, n, D, inner=(1, 2), zero=(2 * D + 6, 2 * D + 7, 2 * D + 8, 2 * D + 9))
    assert got[: 2 * D + 10] == want[: 2 * D + 10]
    assert torch.equal(_slots(ws, m, n, D), _slots(ws_plain, m, n, D))


# ---- (g) mid-size path at the default limits: words 0 .. D from inside forward_layers_mid_kernel -----------------------------------
def _mid_expect(tail):
    # plan (csrc/forward_plan.h): ScalesKernel::Full clears [0, 2 D + 7) and takes max |W_0|; with the tail kernel nobody takes the inner
    # pairs (FinalOperands::None: words 2 D + 2 .. 2 D + 5 stay 0), without it FinalOperands::Split does
    return dict(inner=(), zero=(2 * D + 2, 2 * D + 3, 2 * D + 4, 2 * D + 5)) if tail else dict(inner=(1, 2), zero=())


@pytest.mark.parametrize("tail", [3, 0])
@pytest.mark.parametrize("n", [4097, 8191])
def test_mid_size_path(dev, n, tail):
    """4 097 rows: 257 tiles, the last one of ONE row; 8 191 rows: a last tile of 15.  The maximum of slots 0 and 1 lies in the last row."""
    from tilingnn_amd._lib import lib
    assert lib.tgnn_get_small_layout_limit() < n <= lib.tgnn_get_mid_layout_limit() and n <= 16384   # (16 384: the tail kernel's limit)
    inputs = _tensors(bc.peak_layout(n - 1, n=n, seed=bc.MID_SEED if n > bc.N_PEAK else 5), dev)
    net, _ = make_net(dev, depth=D)
    with switch("tgnn_set_mid_tail", tail):
        ws, m, graph = _forward(net, inputs, n, dev, path=2)
    assert graph.mid is not None
    _assert_peak(_slots(ws, m, n, D), n - 1)                     # (the last block's merge sets word 1, its prologue word 0)
    w = assert_bounds(ws, m, net, n, n, D, **_mid_expect(tail))
    assert (w[2 * D + 2] == 0) == bool(tail)                      # the path the switch asked for was taken


# ---- reused workspace: x 64 network first, then the plain one on the same words -----------------------------------------------------
REUSE_CASES = [("general", bc.N_PEAK, 3), ("mid", 4097, 3), ("mid", 8191, 3), ("mid", 8191, 0)]


def _reuse_setup(dev, kind, n, tail):
    from tilingnn_amd._lib import lib
    if kind == "general":
        lib.tgnn_set_small_layout_limit(0)
        lib.tgnn_set_mid_layout_limit(0)
    inputs = _tensors(bc.peak_layout(n - 1, n=n, seed=bc.MID_SEED if n > bc.N_PEAK else 5), dev)
    net, sd = make_net(dev, depth=D)
    big = _net_from(bc.scaled_state_dict(sd), dev)
    expect = dict(inner=(1, 2), zero=(2 * D + 6, 2 * D + 7, 2 * D + 8, 2 * D + 9)) if kind == "general" else _mid_expect(tail)
    return inputs, net, big, sd, expect, 0 if kind == "general" else 2


@pytest.fixture
def restore_limits():
    from tilingnn_amd._lib import lib
    before = lib.tgnn_get_small_layout_limit(), lib.tgnn_get_mid_layout_limit()
    yield
    lib.tgnn_set_small_layout_limit(before[0])
    lib.tgnn_set_mid_layout_limit(before[1])


@pytest.mark.parametrize("kind,n,tail", REUSE_CASES)
def test_every_forward_re_establishes_the_words_on_a_reused_workspace(dev, restore_limits, kind, n, tail):
    """What TilinGNN.forward's cached workspace sees.  The x 64 network's words are ~2^12 above the plain network's: a word that a
    forward only raises (an atomicMax into a word nobody cleared) still holds the first forward's value behind the second."""
    inputs, net, big, _, expect, path = _reuse_setup(dev, kind, n, tail)
    with switch("tgnn_set_mid_tail", tail):
        ws, m, _ = _forward(big, inputs, n, dev, path=path)
        first = assert_bounds(ws, m, big, n, n, D, **expect)
        ws2, m2, _ = _forward(net, inputs, n, dev, ws=ws, path=path)
        assert ws2 is ws and m2 == m
        second = assert_bounds(ws, m, net, n, n, D, **expect)
    assert all(_word_float(first[k]) > 256 * _word_float(second[k]) for k in range(1, D + 1)), "the x 64 network is not ~2^12 larger"


# ---- the consumers at those magnitudes: fp16 pairs (they need the bounds) against bf16 x 3 (it needs none) --------------------------
_ORACLE = {}


def _oracle_slots(sd_big, n):
    if n not in _ORACLE:
        sg = bc.peak_layout(n - 1, n=n, seed=bc.MID_SEED if n > bc.N_PEAK else 5)
        inputs64 = tuple(t.double() if t.is_floating_point() else t for t in sg.to_torch("cpu"))
        cap = {}
        with torch.no_grad():
            orc.tilingnn_forward(orc.cast_sd(sd_big, torch.float64), *inputs64, capture=cap)
        _ORACLE[n] = [cap["init"]] + [cap[f"mid.{k}"] for k in range(1, D + 1)]
    return _ORACLE[n]


@pytest.mark.parametrize("kind,n,tail", REUSE_CASES[:3])
def test_fp16_pairs_are_as_close_to_fp64_as_bf16x3_at_large_magnitudes(dev, restore_limits, kind, n, tail):
    """Every slot of the x 64 network against the fp64 oracle, max |error| / max |slot|: the fp16-pair forward (whose scales are the
    words above) at most 2 x the bf16 x 3 forward's figure -- the factor tests/test_small_layout.py allows between two rounding
    realisations of this network."""
    inputs, _, big, sd, _, path = _reuse_setup(dev, kind, n, tail)
    want = _oracle_slots(bc.scaled_state_dict(sd), n)
    errs = {}
    for name, mode in (("fp16", 1), ("bf16x3", 0)):
        with switch("tgnn_set_split_precision", mode):
            ws, m, _ = _forward(big, inputs, n, dev, columns=mode == 0, path=path if mode else 0)
        # (bf16 x 3 takes no bounds: nobody writes the slots' words of the zeroed workspace -- it IS the other path)
        assert all((v != 0) == bool(mode) for v in _words(ws, m, D)[: D + 1])
        got = _slots(ws, m, n, D).cpu().double()
        errs[name] = [float((got[k] - want[k]).abs().max() / want[k].abs().max()) for k in range(D + 1)]
    for k in range(D + 1):
        ratio = errs["fp16"][k] / errs["bf16x3"][k]
        print(f"{kind} n {n} slot {k}: fp16 pairs {errs['fp16'][k]:.3e}  bf16 x 3 {errs['bf16x3'][k]:.3e}  ratio {ratio:.2f}")
        _ERROR_ROWS.append((f"{kind} n={n}", k, errs["fp16"][k], errs["bf16x3"][k], ratio))
    for k in range(D + 1):
        assert errs["fp16"][k] <= 2 * errs["bf16x3"][k], (k, errs["fp16"][k], errs["bf16x3"][k])


# ---- (h) width 64 with tgnn_set_nnconv64_eg(1): bounds64 ----------------------------------------------------------------------------
def test_width_64_edge_group_bounds(dev, general_schedule):
    from tilingnn_amd import _lib
    n = bc.N_PEAK
    inputs = _tensors(bc.peak_layout(n - 1), dev)
    net, _ = make_net(dev, depth=D, width=64)
    with switch("tgnn_set_nnconv64_eg", 1):
        ws, m, graph = _forward(net, inputs, n, dev, path=0)
    assert m["bounds64"] > 0 and 1 <= graph.n_types <= int(_lib.lib.tgnn_nnconv64_eg_max_types())   # plan: eg64
    slots = _slots(ws, m, n, D, c=64)
    _assert_peak(slots, n - 1, ks=(0,))
    w = ws[m["bounds64"]: m["bounds64"] + 2 * D * 4].view(torch.int32).cpu().tolist()
    sd = net.state_dict()
    for i in range(D):
        assert w[i] == _bits(slots[i].abs().max()) and w[i] != 0, ("slot", i)
        assert w[D + i] == _bits(sd[f"brch_1_graph_conv_layers.{i}.nnConv.root"].abs().max()), ("root", i)


# ---- (i) sharded, one all-to-all per layer, world 2: merge_kernel over nr rows / shard_unpack1_merge_kernel -------------------------
@pytest.mark.parametrize("split", [False, True])
def test_sharded_words_cover_the_halo_rows(dev, general_schedule, split):
    """Each shard's word k is the maximum over ITS rows, halo rows included (the NNConv and the GIN gather them); word 0 includes the
    absmax_kernel over the halo rows of middle[0].  The outlying row is rank 1's first: a HALO row of rank 0, whose words 0 and 1 are
    therefore set by a row it does not own."""
    from tilingnn_amd import _lib
    from tilingnn_amd import dist as tdist
    world, n_total = 2, 2 * bc.N_PEAK
    _lean_defaults()
    sg = bc.plain_layout(n_total)
    shards = [tdist.make_shard(sg.node_feature, sg.align_edge_index, sg.align_edge_features, sg.collide_edge_index, r, world)
              for r in range(world)]
    peak = shards[1].lo
    sg.node_feature[peak, -1] = bc.PEAK_FEATURE
    shards = [tdist.make_shard(sg.node_feature, sg.align_edge_index, sg.align_edge_features, sg.collide_edge_index, r, world)
              for r in range(world)]
    tdist.LocalSimComm.setup(shards)
    nets = [make_net(dev, depth=D)[0] for _ in range(world)]
    hub = tdist.ThreadSimCollectives.Hub(world)
    runners = [tdist.FusedShardForward(nets[r], shards[r], dev, tdist.ThreadSimCollectives(hub, r), fused=True) for r in range(world)]
    if split:
        assert _lib.side_stream(dev).value, "no side stream: the split exchange is not taken"
    for rn in runners:
        rn.two_streams = split
    c0 = _lib.forward_path_counts()
    run_thread_ranks(dev, runners, hub)
    assert _lib.forward_path_counts()[0] == c0[0] + world
    dims = nets[0]._dims()
    maps = [_lib.forward_workspace_map(dims, s.n_own, s.n_rows, rn.n_types) for s, rn in zip(shards, runners)]
    assert all(s.n_rows > s.n_own for s in shards)
    populations = {l: torch.cat([_fresh_f_population(rn.workspace, m, s.n_own, l) for s, rn, m in zip(shards, runners, maps)]) for l in (1, 2)}
    slots0 = _slots(runners[0].workspace, maps[0], shards[0].n_rows, D)
    for k in (0, 1):                                             # the precondition: rank 0's maximum lies in a halo row
        assert int(slots0[k].abs().max(dim=1).values.argmax()) >= shards[0].n_own, k
    for s, rn, m in zip(shards, runners, maps):
        assert_bounds(rn.workspace, m, nets[s.rank], s.n_own, s.n_rows, D, inner=(1, 2), zero=(2 * D + 6, 2 * D + 7, 2 * D + 8, 2 * D + 9),
                      n_total=n_total, populations=populations)
