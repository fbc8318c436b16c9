"""The eval-mode forward (TilinGNN.eval(): tgnn_forward with use_running_stats, BatchNorm on the running buffers -- a path of its
own through csrc/forward_plan.h: no persistent kernel, no fp16 pairs, no lean head, no fused init MLP, every BatchNorm record from
launch_bn_finalize in mode 3) against the fp64 oracle through the WHOLE depth, free running: every skip slot, the final MLP's three
hidden activations and the probabilities, each within its gate.  Cases, statistics and the gate: tests/eval_cases.py; what makes the
gates meaningful: tests/test_eval_cases_host.py.  One measured run: profiles/eval_forward_errors.txt."""
import ctypes as C

import pytest
import torch

from tests import eval_cases as ec

pytestmark = pytest.mark.gpu

_TABLE = []


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "GPU tests need a GPU"
    return torch.device("cuda:0")


@pytest.fixture(scope="module", autouse=True)
def error_table():
    yield
    if _TABLE:
        print("\n# eval-mode forward against the fp64 oracle: worst tap of each group, its gate, error / gate")
        for line in _TABLE:
            print(line)


def make_net(case, dev, eval_mode=True):
    from tilingnn_amd import TilinGNN
    net = TilinGNN(adj_edge_features_dim=case.fe, network_depth=case.depth, network_width=case.width, output_dim=case.out_dim,
                   node_features_dim=case.fx)
    net.load_state_dict(case.state_dict(), strict=True)
    net = net.to(dev)
    return net.eval() if eval_mode else net.train()


def device_inputs(case, dev):
    x, adj, attr, col = case.inputs()
    return x.float().to(dev), adj.to(dev), attr.float().to(dev), col.to(dev)


def state_of(net):
    return {k: v.detach().clone() for k, v in net.state_dict().items()}


def assert_state_unchanged(net, before):
    after = net.state_dict()
    assert list(after) == list(before)
    for k in before:
        assert torch.equal(before[k], after[k]), k


def raw_forward(net, inputs, dev, graph=None, ws=None, use_running_stats=1):
    """tgnn_forward on a workspace of the caller's (default: a zeroed one) -> {tap: CPU tensor}, read through
    tgnn_forward_workspace_map.  The graph is handed over as TilinGNN.forward hands it over in eval mode."""
    from tilingnn_amd import _lib, ops
    x, adj, attr, col = inputs
    n, d, c = int(x.shape[0]), net.network_depth, net.network_width
    if graph is None:
        graph = ops.prepare_graph(n, adj, attr, col)
    if graph.cols is None and graph.groups is not None:
        graph.ensure_columns()
    dims = net._dims()
    table, _ = net._param_table()
    ws_bytes = int(_lib.lib.tgnn_forward_workspace_bytes(C.byref(dims), n, graph.n_types))
    if ws is None:
        ws = torch.zeros(ws_bytes, dtype=torch.uint8, device=dev)
    assert ws.numel() >= ws_bytes
    probs = torch.empty(n, net.output_dim, device=dev)
    g = ops.c_struct_for_width(graph, c)
    _lib.check(_lib.lib.tgnn_forward(C.byref(dims), table, ops.ptr(x), ops.ptr(attr), C.byref(g), 0, use_running_stats, ops.ptr(probs),
                                    ops.ptr(ws), ws_bytes, _lib.current_stream(dev), _lib.side_stream(dev)))
    torch.cuda.synchronize()
    m = _lib.forward_workspace_map(dims, n, n, graph.n_types)

    def piece(name, *shape):
        count = 1
        for s in shape:
            count *= s
        assert m[name] >= 0 and m[name] % 4 == 0 and m[name] + 4 * count <= ws_bytes
        return ws[m[name]: m[name] + 4 * count].view(torch.float32).view(*shape).clone().cpu()
    mid = piece("mid", d + 1, n, c)
    taps = {"mid.%d" % k: mid[k] for k in range(d + 1)}
    taps.update(f1=piece("f1", n, 256), f2=piece("f2", n, 128), f3=piece("f3", n, 64), probs=probs.cpu())
    return taps


def tap_groups(case):
    return (("skip slots", ["mid.%d" % k for k in range(case.depth + 1)]), ("final hidden", ["f1", "f2", "f3"]), ("probs", ["probs"]))


def measure(case, taps):
    """[(group, worst tap, error, gate, error / gate)]: the tap of every group that is closest to (or furthest beyond) its gate."""
    want = ec.reference(case)[0]
    out = []
    for group, names in tap_groups(case):
        ratio, tap = max((ec.tap_error(t, taps[t], want[t]) / ec.gate(case, t), t) for t in names)
        out.append((group, tap, ec.tap_error(tap, taps[tap], want[tap]), ec.gate(case, tap), ratio))
    return out


def assert_within_gates(case, taps, label=""):
    rows = measure(case, taps)
    _TABLE.append(f"{case.name}{label}: " + "; ".join(f"{g} {t} {e:.2e} gate {gt:.2e} ratio {r:.2f}" for g, t, e, gt, r in rows))
    want = ec.reference(case)[0]
    bad = [(t, ec.tap_error(t, taps[t], want[t]), ec.gate(case, t)) for t in case.taps()
           if not ec.tap_error(t, taps[t], want[t]) <= ec.gate(case, t)]
    assert not bad, (case.name, label, bad)


def assert_probs_within_gate(case, probs):
    want = ec.reference(case)[0]["probs"]
    assert probs.shape == want.shape
    err = ec.tap_error("probs", probs.cpu(), want)
    assert err <= ec.gate(case, "probs"), (case.name, err, ec.gate(case, "probs"))


# --------------------------------------------------------------------------------------------------- every case against its gates
@pytest.mark.parametrize("case", ec.LAYOUT_CASES + ec.MODEL_CASES, ids=lambda c: c.name)
def test_eval_forward_meets_the_gate(dev, case):
    """Every skip slot, F1 F2 F3 and the probabilities of tgnn_forward(use_running_stats = 1), and the module's own
    net.eval(); net(...), within the case's gates; no buffer or parameter moves; the forward is the general schedule's."""
    from tilingnn_amd import _lib, ops
    net, inputs = make_net(case, dev), device_inputs(case, dev)
    before = state_of(net)
    c0 = _lib.forward_path_counts()
    taps = raw_forward(net, inputs, dev)
    probs, passthrough = net(*inputs)
    torch.cuda.synchronize()
    assert _lib.forward_path_counts() == (c0[0] + 2, c0[1], c0[2])         # (300, 1 254, 4 097 rows included: neither persistent kernel)
    assert passthrough is inputs[2]
    assert_within_gates(case, taps)
    assert_probs_within_gate(case, probs)
    assert_state_unchanged(net, before)
    if case.n_types == 50:                                                  # above the column structure's limit: the CSR kernel
        graph = ops.prepare_graph(case.n, inputs[1], inputs[2], inputs[3])
        assert graph.n_types == 50 > int(_lib.lib.tgnn_nnconv_cols_max_types()) and graph.cols is None and graph.groups is None
    if case.n == 1:                                                         # only eval accepts one row
        with pytest.raises(ValueError, match="more than 1 value"):
            net.train()(*inputs)
        assert_state_unchanged(net, before)


def test_width_16_is_refused_loudly(dev):
    """The final MLP reads the slot-major skip buffer in blocks of 32 columns: a network_width of 16 is an error, not a result."""
    from tilingnn_amd import _lib
    case = ec.Case("width-16", "syn", 17, depth=1, width=16, stats="jittered", seed=7)
    net, inputs = make_net(case, dev), device_inputs(case, dev)
    before = state_of(net)
    with pytest.raises(_lib.TgnnError, match="multiple of 32"):
        net(*inputs)
    torch.cuda.synchronize()
    assert_state_unchanged(net, before)


# ------------------------------------------------------------------------------------------------------------------------ routing
def test_a_graph_with_edge_groups_only_gets_its_columns(dev, general_schedule):
    """3 000 rows on the general schedule are prepared with edge groups only; the eval forward (no fp16 pairs) builds the type
    columns on first use, keeps them on the cached graph, and meets the gates on them."""
    from tilingnn_amd import _lib
    from tilingnn_amd.graph_networks import _graph_cache
    case = ec.CASES["3000-rows"]
    net, inputs = make_net(case, dev), device_inputs(case, dev)
    _graph_cache.clear()
    graph = _graph_cache.get_full(case.n, inputs[1], inputs[2], inputs[3])
    assert graph.groups is not None and graph.cols is None
    c0 = _lib.forward_path_counts()
    probs, _ = net(*inputs)
    torch.cuda.synchronize()
    assert _lib.forward_path_counts() == (c0[0] + 1, c0[1], c0[2])
    assert _graph_cache.get_full(case.n, inputs[1], inputs[2], inputs[3]) is graph and graph.cols is not None
    assert_probs_within_gate(case, probs)
    taps = raw_forward(net, inputs, dev, graph=graph)
    assert torch.equal(taps["probs"], probs.cpu())
    assert_within_gates(case, taps, " (general_schedule, columns built on first use)")


def test_width_64_switches_in_eval(dev):
    """tgnn_set_nnconv64_eg: the plan refuses the edge-group NNConv on running statistics -- the bits of the switch-off forward.
    tgnn_set_gin64_mfma: taken in either BatchNorm mode -- other bits, the same gates."""
    from tilingnn_amd import ops
    case = ec.CASES["width-64"]
    net, inputs = make_net(case, dev), device_inputs(case, dev)
    off = raw_forward(net, inputs, dev)
    prev = ops.set_nnconv64_eg(1)
    try:
        eg = raw_forward(net, inputs, dev)
        p_eg = net(*inputs)[0].cpu()
    finally:
        ops.set_nnconv64_eg(prev)
    for tap in case.taps():
        assert torch.equal(eg[tap], off[tap]), tap
    assert torch.equal(p_eg, off["probs"])
    prev = ops.set_gin64_mfma(1)
    try:
        mfma = raw_forward(net, inputs, dev)
    finally:
        ops.set_gin64_mfma(prev)
    assert torch.equal(mfma["mid.0"], off["mid.0"]) and not torch.equal(mfma["mid.1"], off["mid.1"])
    assert not torch.equal(mfma["probs"], off["probs"])
    assert_within_gates(case, mfma, " (gin64_mfma on)")


def test_the_training_forward_refuses_an_eval_network(dev):
    """tgnn_forward_train has no running-statistics mode: an eval() network is an error in front of any launch, nothing moves."""
    from tilingnn_amd import train
    case = ec.CASES["17-rows"]
    net, inputs = make_net(case, dev), device_inputs(case, dev)
    before = state_of(net)
    with pytest.raises(ValueError, match="eval mode"):
        train.forward_train(net, *inputs)
    torch.cuda.synchronize()
    assert_state_unchanged(net, before)


def test_the_sharded_forward_refuses_an_eval_network(dev):
    from tests import shard_cases as sc
    from tilingnn_amd import dist as tdist
    kind = sc.CASE_TABLE[0][0]
    c = sc.case(kind)
    shard = c.shards[0]
    case = ec.Case("sharded", "syn", 17, depth=2, width=c.width)
    net = make_net(case, dev)
    before = state_of(net)
    runner = tdist.FusedShardForward(net, shard, dev, tdist.ThreadSimCollectives(tdist.ThreadSimCollectives.Hub(c.world), 0),
                                     inputs=tdist.HipBackend(dev).upload(shard))
    with pytest.raises(ValueError, match="eval mode"):
        runner.step()
    torch.cuda.synchronize()
    assert_state_unchanged(net, before)
    assert getattr(runner, "workspace", None) is None               # (no workspace was made, nothing was queued)


# -------------------------------------------------------------------------------------------------------------------------- state
def test_eval_forward_is_repeatable_and_ignores_what_the_workspace_held(dev):
    """Two calls: the same bits.  A workspace that a train-mode forward of ANOTHER layout has just filled: the bits of a zeroed one
    (every BatchNorm record, partial sum and bound the eval path reads is one it wrote)."""
    case, other = ec.CASES["labyrinth"], ec.CASES["many-900"]
    net, inputs = make_net(case, dev), device_inputs(case, dev)
    first, second = raw_forward(net, inputs, dev), raw_forward(net, inputs, dev)
    for tap in case.taps():
        assert torch.equal(first[tap], second[tap]), tap
    ws = torch.zeros(64 << 20, dtype=torch.uint8, device=dev)
    raw_forward(make_net(other, dev, eval_mode=False), device_inputs(other, dev), dev, ws=ws, use_running_stats=0)
    assert int(ws.count_nonzero()) > 0
    dirty = raw_forward(net, inputs, dev, ws=ws)
    for tap in case.taps():
        assert torch.equal(first[tap], dirty[tap]), tap


def _train_eval_train(case, dev):
    from tilingnn_amd.graph_networks import _graph_cache
    inputs = device_inputs(case, dev)
    _graph_cache.clear()
    fresh = make_net(case, dev, eval_mode=False)
    want = fresh(*inputs)[0].clone()
    _graph_cache.clear()
    net = make_net(case, dev, eval_mode=False)
    p1 = net(*inputs)[0].clone()
    graph = _graph_cache.get_full(case.n, inputs[1], inputs[2], inputs[3])
    had_cols = graph.cols is not None
    net.eval()
    buffers = state_of(net)
    p2 = net(*inputs)[0].clone()
    assert_state_unchanged(net, buffers)
    net.train()
    p3 = net(*inputs)[0].clone()
    torch.cuda.synchronize()
    assert _graph_cache.get_full(case.n, inputs[1], inputs[2], inputs[3]) is graph
    assert torch.equal(p1, want) and torch.equal(p3, want)
    assert not torch.equal(p2, want)
    return graph, had_cols


def test_train_eval_train_on_one_cached_graph(dev):
    _train_eval_train(ec.CASES["labyrinth"], dev)


def test_train_eval_train_where_eval_changes_the_cached_graph(dev, general_schedule):
    graph, had_cols = _train_eval_train(ec.CASES["3000-rows"], dev)
    assert not had_cols and graph.cols is not None and graph.groups is not None


def test_autograd_switch_in_eval_returns_plain_tensors(dev):
    case = ec.CASES["17-rows"]
    net, inputs = make_net(case, dev), device_inputs(case, dev)
    want = net(*inputs)[0].clone()
    net.autograd = True
    assert torch.is_grad_enabled()
    probs, _ = net(*inputs)
    assert not probs.requires_grad and probs.grad_fn is None and torch.equal(probs, want)
    assert_probs_within_gate(case, probs)


# ---------------------------------------------------------------------------------------------------------------- batched entries
@pytest.mark.parametrize("union", [False, True])
def test_forward_many_in_eval_is_the_solo_forwards(dev, union):
    """Five layouts, the one-row layout among them: every output the bits of its solo eval forward (and within its gate), nothing
    enters a union launch on running statistics, no buffer moves."""
    from tilingnn_amd import _lib
    cases = ec.MANY_CASES
    assert len({(c.fe, c.depth, c.width, c.out_dim, c.fx, c.seed) for c in cases}) == 1
    net = make_net(ec.CASES["many-640"], dev)                          # (one network: the default ridge's buffers)
    layouts = [device_inputs(c, dev) for c in cases]
    solo = [net(*l)[0].clone() for l in layouts]
    torch.cuda.synchronize()
    before, counts = state_of(net), _lib.forward_union_counts()
    outs = net.forward_many(layouts, union=union)
    torch.cuda.synchronize()
    assert _lib.forward_union_counts() == counts
    assert_state_unchanged(net, before)
    for c, got, want in zip(cases, outs, solo):
        assert torch.equal(got, want), c.name
        if c.ridge == ec.RIDGE:                                        # (the labyrinth case's own gate belongs to its own buffers)
            assert_probs_within_gate(c, got)
