"""The NNConv adjoint on edge groups (tilingnn_amd/csrc/nnconv_bwd_eg.hip behind tgnn_nnconv_bwd_eg, train.nnconv_backward(kernel="eg"))
as an op against fp64, and its opt-in route through tgnn_backward_groups / train.backward_train (tgnn_set_nnconv_bwd_eg,
train.set_nnconv_bwd_eg), widths 32 and 64.

Graphs: tests/train_graphs.directed_graph -- one direction per pair, a sink hub of one type, a source hub, rows without in-edges and
rows without out-edges: the transposed CSR is another graph and in-degree is not out-degree.  Gates: 1e-5 of each output's largest
magnitude against fp64 autograd (tests/test_training_sizes.py's gate for this adjoint); per edge type max(1e-5, 2 x the chain's error
on the same inputs): the two routes add the same fp32 products in another order.  Measured on an MI355X:
profiles/nnconv_bwd_eg_errors.txt.

"The same bits on either side of the dW grid cap" is read as: repeated calls give the same bits with the dW grid below its cap
(4 099 rows) and at it (66 003 rows) -- the plan's grid is asserted in both cases.  Two different grids add a type's partial tiles
in different groupings, so their fp32 sums are not comparable bit for bit."""
import functools
from types import SimpleNamespace

import numpy as np
import pytest
import torch

from oracle import tilingnn_oracle as orc
from tests import train_graphs as tgr
from tests.golden_util import graph_tensors, load_labyrinth_graph
from tests.test_training_sizes import FE, _gate, _net, _rel, _rng
from tests.train_graphs import N_BIG, N_MID

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
WIDTHS = [32, 64]
T_MAX = {32: 22, 64: 18}
EDGES = {200: (1500, 2000), 1254: (10000, 12000), N_MID: (30000, 25000), N_BIG: (tgr.EA_BIG, tgr.EC_BIG)}
P1 = "brch_1_graph_conv_layers.1"
GRAD_KEYS = {P1 + ".nnConv.root", P1 + ".nnConv.bias"} | {f"{P1}.mlp.mlp.{k}.linear.{w}" for k in range(3) for w in ("weight", "bias")}


class _switches:
    """eg = the new switch; the older opt-in switches travel together (`others`: the two adjoint switches set_mlp_bwd_fused and
    set_mlp_bwd_tall64, the two width-64 forward switches set_nnconv64_eg and set_gin64_mfma); all put back on exit."""

    def __init__(self, eg, others=0):
        self.want = (eg, others)

    def __enter__(self):
        from tilingnn_amd import ops, train
        o = self.want[1]
        self.prev = (train.set_nnconv_bwd_eg(self.want[0]), train.set_mlp_bwd_fused(o), train.set_mlp_bwd_tall64(o),
                     ops.set_nnconv64_eg(o), ops.set_gin64_mfma(o))

    def __exit__(self, *exc):
        from tilingnn_amd import ops, train
        train.set_nnconv_bwd_eg(self.prev[0])
        train.set_mlp_bwd_fused(self.prev[1])
        train.set_mlp_bwd_tall64(self.prev[2])
        ops.set_nnconv64_eg(self.prev[3])
        ops.set_gin64_mfma(self.prev[4])


@functools.lru_cache(maxsize=None)
def _graph(n, T):
    """The directed graph of (n, T) on the device, prepared both ways; built once, read only."""
    from tilingnn_amd import ops, train
    ea, ec = EDGES[n]
    cpu = tgr.directed_graph(n, ea, ec, T, FE, seed=2000 + T)
    x, adj, attr, col = (t.to(DEV) for t in cpu)
    graph = ops.prepare_graph(n, adj, attr, col)
    assert graph.n_types == T and graph.n_adj_edges == ea
    return SimpleNamespace(n=n, T=T, ea=ea, cpu=cpu, x=x, adj=adj, attr=attr, col=col, graph=graph, tg=train.TrainGraph(graph, adj, col))


@functools.lru_cache(maxsize=None)
def _case(n, T, width, mag=1.0):
    """Inputs of one NNConv adjoint and its fp64 expectations (autograd over the oracle's op, on the CPU); built once, read only."""
    from tilingnn_amd import ops
    torch.set_num_threads(8)
    p = _graph(n, T)
    _, adj_c, attr_c, _ = p.cpu
    net, sd = _net(FE, 2, 5, width)
    conv = net.brch_1_graph_conv_layers[1].nnConv
    r = _rng(31 + n + T + width)
    h, dz = r(n, width).to(DEV), (r(n, width) * mag).to(DEV)
    wtab = ops.edge_weight_table(p.attr, p.graph, *conv._edge_mlp_params(), width).contiguous()
    sd64 = orc.cast_sd(sd, torch.float64)
    leaf = {k: (v.clone().requires_grad_(True) if k.startswith(P1) and v.is_floating_point() else v) for k, v in sd64.items()}
    hh = h.double().cpu().requires_grad_(True)
    out = orc.nnconv_mean_dedup(hh, adj_c, attr_c.double(), leaf, P1)
    (out * dz.double().cpu()).sum().backward()
    want = {k: leaf[k].grad for k in GRAD_KEYS}
    want["dh"] = hh.grad
    return SimpleNamespace(p=p, conv=conv, h=h, dz=dz, g=dz * p.tg.inv_deg[:, None], wtab=wtab, want=want, sd64=sd64)


def _backward(c, kernel):
    from tilingnn_amd import train
    grads = {}
    dh = train.nnconv_backward(c.conv, P1, c.p.tg, c.wtab, c.h, c.dz, c.g, c.p.attr, grads, kernel=kernel)
    assert set(grads) == GRAD_KEYS
    grads["dh"] = dh
    return grads


def _gate_all(what, c, got):
    for k in sorted(got):
        assert torch.isfinite(got[k]).all(), (what, k)
        _gate(f"{what} {k}", got[k].reshape(c.want[k].shape), c.want[k], 1e-5)


def _dwcat(c, kernel):
    """[T + 1][C][C] ([in][out]; entry T: d root) of either route."""
    from tilingnn_amd import train
    tg, T, n = c.p.tg, c.p.T, c.p.n
    w = int(c.h.shape[1])
    if kernel == "chain":
        s = train.type_sum(c.g, c.g, tg.deg, tg.adjT_rowptr, tg.adjT_src, tg.adjT_type, n, T)
        return train.wgrad(c.h, s).view(w, T + 1, w).permute(1, 0, 2).contiguous()
    rc, dh, dwcat, _ = _op(c)
    assert rc == 0
    return dwcat.view(T + 1, w, w)


def _op(c, h=None, ld=None, poison=None, T=None, width=None):
    """tgnn_nnconv_bwd_eg through ctypes -> (return code, dh, dwcat, workspace)."""
    from tilingnn_amd import train
    from tilingnn_amd._lib import lib, ptr
    tg = c.p.tg
    gt = tg.ensure_groups_t()
    n = c.p.n
    T = c.p.T if T is None else T
    w = int(c.h.shape[1]) if width is None else width
    fill = (lambda *s: torch.full(s, poison, device=DEV)) if poison is not None else (lambda *s: torch.empty(*s, device=DEV))
    dh, dwcat = fill(n, w), fill((T + 1) * w, w)
    nb = max(int(lib.tgnn_nnconv_bwd_eg_workspace_bytes(n, gt.groups_cap, c.p.T, int(c.h.shape[1]))), 1 << 20)
    ws = torch.full((nb,), 7, dtype=torch.uint8, device=DEV)
    h = c.h if h is None else h
    rc = lib.tgnn_nnconv_bwd_eg(ptr(h), w if ld is None else ld, ptr(c.dz), ptr(c.g), ptr(gt.fwd.tile_grp_ptr), ptr(gt.fwd.grp),
                                ptr(gt.bwd.tile_grp_ptr), ptr(gt.bwd.grp), ptr(gt.type_major), gt.n_list, ptr(c.wtab),
                                ptr(c.conv.root), n, T, w, gt.max_in_degree, gt.max_out_degree, ptr(dh), ptr(dwcat), ptr(ws), nb,
                                train._s(c.h))
    return rc, dh, dwcat, ws


# ---------------------------------------------------------------------------------------------- 1. the op against fp64
SHAPES = [(200, 1), (1254, 13), (N_MID, "max"), (N_BIG, 2)]


@pytest.mark.parametrize("width", WIDTHS)
@pytest.mark.parametrize("n,T", SHAPES)
def test_op_against_fp64(n, T, width):
    """200 rows: 13 tiles, the last half-empty, one edge type; 1 254 rows / 13 types: the labyrinth layout's size and count; 4 099
    rows at the width's largest type count (22 | 18); 66 003 rows (past 65 536) with two types: 130 000 edges of one type in one
    accumulator chain.  dh, d root, d bias and the six edge-MLP gradients at 1e-5 of their largest magnitude."""
    from tilingnn_amd._lib import lib
    T = T_MAX[width] if T == "max" else T
    c = _case(n, T, width)
    gt = c.p.tg.ensure_groups_t()
    assert lib.tgnn_nnconv_bwd_eg_ok(width, n, T, gt.max_in_degree, gt.max_out_degree, 1, 1) == 1
    assert gt.max_in_degree >= tgr.hub_sizes(n)[0] and gt.max_out_degree >= tgr.hub_sizes(n)[0]
    _gate_all(f"eg n={n} T={T} width={width}", c, _backward(c, "eg"))


@pytest.mark.parametrize("width", WIDTHS)
@pytest.mark.parametrize("mag", [1e-6, 1e-3, 1e2])
@pytest.mark.parametrize("n", [1254, N_MID])
def test_op_against_fp64_over_gradient_magnitudes(n, mag, width):
    """dz of magnitude 1e-6 (what training produces), 1e-3 and 1e2 (1: the test above): the rows' power-of-two scale comes from
    their own bound, so the relative error does not move."""
    c = _case(n, 13, width, mag)
    _gate_all(f"eg n={n} width={width} |dz|~{mag:g}", c, _backward(c, "eg"))


# ---------------------------------------------------------------------------------------------- 2. what the max-norm hides
@pytest.mark.parametrize("width", WIDTHS)
@pytest.mark.parametrize("n,T", [(1254, 13), (N_MID, "max"), (N_BIG, 2)])
def test_every_edge_type_against_its_own_norm(n, T, width):
    """dW_t of every type (and d root) against ITS OWN largest magnitude: a type with few edges disappears under the table's largest
    entry.  Bound: max(1e-5, 2 x the chain's error for that type on the same inputs) -- another fp32 summation order, not another
    accuracy class."""
    T = T_MAX[width] if T == "max" else T
    c = _case(n, T, width)
    src, dst = c.p.adj[0], c.p.adj[1]
    et = c.p.graph.edge_type[:c.p.ea].long()
    h64, g64 = c.h.double(), c.dz.double() / c.p.tg.deg.double()[:, None]
    eg, chain = _dwcat(c, "eg"), _dwcat(c, "chain")
    rows = []
    for t in range(T + 1):
        if t < T:
            e = (et == t).nonzero().flatten()
            want = h64[src[e]].t() @ g64[dst[e]]
            count = int(e.numel())
        else:
            want, count = h64.t() @ c.dz.double(), n
        ee, ec = _rel(eg[t], want), _rel(chain[t], want)
        rows.append((t, count, ee, ec))
        print(f"n={n} width={width} T={T} type {t if t < T else 'root'} ({count} edges): eg {ee:.2e} chain {ec:.2e}")
    for t, count, ee, ec in rows:
        assert count > 0 and ee < max(1e-5, 2.0 * ec), (t, count, ee, ec)


# ---------------------------------------------------------------------------------------------- 3. dh on special rows
@pytest.mark.parametrize("width", WIDTHS)
def test_dh_on_rows_without_out_edges_on_the_source_hub_and_behind_n(width):
    n, T = N_MID, 13
    c = _case(n, T, width)
    rc, dh, _, _ = _op(c)
    assert rc == 0
    no_out = slice(*tgr.NO_OUT)
    root64 = c.conv.root.detach().double()
    _gate("rows without out-edges: the root term alone", dh[no_out], c.dz[no_out].double() @ root64.t(), 1e-5)
    hub = tgr.ADJ_SOURCE
    assert int(torch.bincount(c.p.adj[0], minlength=n)[hub]) >= 700
    _gate("the source hub row, against its own norm", dh[hub], c.want["dh"][hub], 1e-5)
    # a dh buffer with rows behind n: not written
    from tilingnn_amd import train
    from tilingnn_amd._lib import lib, ptr
    gt = c.p.tg.ensure_groups_t()
    big = torch.full((n + 40, width), 12345.0, device=DEV)
    dwcat = torch.empty((T + 1) * width, width, device=DEV)
    nb = int(lib.tgnn_nnconv_bwd_eg_workspace_bytes(n, gt.groups_cap, T, width))
    ws = torch.empty(nb, dtype=torch.uint8, device=DEV)
    assert lib.tgnn_nnconv_bwd_eg(ptr(c.h), width, ptr(c.dz), ptr(c.g), ptr(gt.fwd.tile_grp_ptr), ptr(gt.fwd.grp), ptr(gt.bwd.tile_grp_ptr),
                                  ptr(gt.bwd.grp), ptr(gt.type_major), gt.n_list, ptr(c.wtab), ptr(c.conv.root), n, T, width,
                                  gt.max_in_degree, gt.max_out_degree, ptr(big), ptr(dwcat), ptr(ws), nb, train._s(c.h)) == 0
    assert torch.equal(big[:n], dh) and bool((big[n:] == 12345.0).all())


# ---------------------------------------------------------------------------------------------- 4. the same bits
@pytest.mark.parametrize("width", WIDTHS)
@pytest.mark.parametrize("n,T", [(N_MID, 13), (N_BIG, 2)])
def test_same_bits_on_every_call_below_and_at_the_dw_grid_cap(n, T, width):
    """Three calls, the same bits in dh and in dwcat: no atomics, no order that depends on timing.  4 099 rows: the dW grid is below
    its cap of 512 blocks; 66 003 rows: at it."""
    from tilingnn_amd._lib import lib
    c = _case(n, T, width)
    gt = c.p.tg.ensure_groups_t()
    blocks = lib.tgnn_nnconv_bwd_eg_dw_blocks(gt.n_list)
    assert (1 < blocks < 512) if n == N_MID else blocks == 512
    _, dh0, dw0, _ = _op(c)
    for _ in range(2):
        rc, dh, dw, _ = _op(c)
        assert rc == 0 and torch.equal(dh, dh0) and torch.equal(dw, dw0)
    a, b = _backward(c, "eg"), _backward(c, "eg")
    for k in a:
        assert torch.equal(a[k], b[k]), k


def test_type_major_list_is_the_stable_sort_of_the_forward_groups():
    """The list against numpy: per type the groups in ascending order, every group once, the tile of each, the root groups as type T."""
    c = _case(N_MID, 13, 32)
    gt = c.p.tg.ensure_groups_t()
    T, n = 13, N_MID
    ptrs = gt.fwd.tile_grp_ptr.cpu().numpy()
    n_groups = int(ptrs[-1])
    meta = (gt.fwd.grp.view(-1, 16, 2)[:n_groups, 0, 1].cpu().numpy() >> 16) & 0xff
    tile_of = np.repeat(np.arange((n + 15) // 16), np.diff(ptrs))
    order = np.argsort(meta, kind="stable")
    lst = gt.type_major.cpu().numpy()
    assert gt.n_list == n_groups == int(lst[T + 1]) and lst[0] == 0
    assert np.array_equal(lst[:T + 2], np.concatenate([[0], np.cumsum(np.bincount(meta, minlength=T + 1))]))
    pairs = lst[64:64 + 2 * n_groups].reshape(-1, 2)
    assert np.array_equal(pairs[:, 0], order) and np.array_equal(pairs[:, 1], tile_of[order])
    assert int((meta == T).sum()) == (n + 15) // 16


# ---------------------------------------------------------------------------------------------- 5. refusals
@pytest.mark.parametrize("width,T,match", [(64, 19, "1 .. 18"), (32, 23, "1 .. 22"), (64, 63, "1 .. 18"), (32, 63, "1 .. 22")])
def test_kernel_eg_raises_naming_the_type_limit(width, T, match):
    from tilingnn_amd import ops, train
    p = _graph(N_MID, T)
    net, _ = _net(FE, 2, 5, width)
    conv = net.brch_1_graph_conv_layers[1].nnConv
    h = _rng(1)(N_MID, width).to(DEV)
    wtab = ops.edge_weight_table(p.attr, p.graph, *conv._edge_mlp_params(), width).contiguous()
    with pytest.raises(ValueError, match=match):
        train.nnconv_backward(conv, P1, p.tg, wtab, h, h, h * p.tg.inv_deg[:, None], p.attr, {}, kernel="eg")
    with _switches(1):                                       # kernel=None under the switch: the chain, as before
        grads = {}
        train.nnconv_backward(conv, P1, p.tg, wtab, h, h, h * p.tg.inv_deg[:, None], p.attr, grads)
    assert set(grads) == GRAD_KEYS


def test_kernel_eg_raises_at_width_16_and_on_an_unknown_name():
    from tilingnn_amd import train
    c = _case(200, 1, 32)
    h16 = c.h[:, :16].contiguous()
    with pytest.raises(ValueError, match="widths 32 and 64"):
        train.nnconv_backward(c.conv, P1, c.p.tg, c.wtab, h16, h16, h16, c.p.attr, {}, kernel="eg")
    with pytest.raises(ValueError, match="'chain' or 'eg'"):
        train.nnconv_backward(c.conv, P1, c.p.tg, c.wtab, c.h, c.dz, c.g, c.p.attr, {}, kernel="fast")


@pytest.mark.parametrize("width,T", [(64, 19), (32, 23), (16, 13)])
def test_op_refuses_and_leaves_the_buffers_untouched(width, T):
    from tilingnn_amd import _lib
    from tilingnn_amd._lib import lib
    c = _case(N_MID, 13, 32 if width == 16 else width)
    rc, dh, dwcat, ws = _op(c, poison=12345.0, T=T, width=width)
    assert rc == _lib.ERR_UNSUPPORTED
    msg = lib.tgnn_last_error()
    assert (b"width must be 32 or 64" in msg) if width == 16 else (b"edge types must lie in 1 .. " in msg), msg
    assert bool((dh == 12345.0).all()) and bool((dwcat == 12345.0).all()) and bool((ws == 7).all())


@pytest.mark.parametrize("width", WIDTHS)
@pytest.mark.parametrize("fault", ["h off by 4 bytes", "row stride 72"])
def test_argument_errors_write_nothing(fault, width):
    c = _case(N_MID, 13, width)
    h, ld = None, None
    if fault == "h off by 4 bytes":
        flat = torch.zeros(N_MID * width + 4, device=DEV)
        h = flat[1:1 + N_MID * width].view(N_MID, width)
        assert h.data_ptr() % 16 == 4
    else:
        ld = 72
    rc, dh, dwcat, ws = _op(c, h=h, ld=ld, poison=12345.0)
    assert rc == -1                                          # TGNN_ERR_INVALID_ARG (include/tgnn.h)
    assert bool((dh == 12345.0).all()) and bool((dwcat == 12345.0).all()) and bool((ws == 7).all())


# ---------------------------------------------------------------------------------------------- 6. the switch
def _forward(graph, depth, width, T=13):
    from tilingnn_amd import train
    if graph == "laby":
        x, adj, attr, col, _ = graph_tensors(load_labyrinth_graph(), torch.float32, DEV)
    else:
        p = _graph(N_MID, T)
        x, adj, attr, col = p.x, p.adj, p.attr, p.col
    net, _ = _net(int(attr.shape[1]), depth, 6, width)
    probs, sv = train.forward_train(net, x, adj, attr, col)
    dprobs = _rng(depth + width)(int(x.shape[0]), 1).to(DEV) * 1e-2
    return net, sv, dprobs


@pytest.mark.parametrize("width", WIDTHS)
def test_switch_off_is_the_code_as_it_stands(width):
    """One depth-3 step's gradients before the switch was touched, with it back at 0 after having been 1, and with it on at T = 63
    (the predicate is false): bit-equal, pair by pair.  A TrainGraph built with the switch off has no groups_t."""
    from tilingnn_amd import train
    assert train.set_nnconv_bwd_eg(-1) == 0                  # the default
    net, sv, dprobs = _forward("laby", 3, width)
    x, adj, attr, col, _ = graph_tensors(load_labyrinth_graph(), torch.float32, DEV)
    tg = train.TrainGraph(sv.tg.g, adj, col)
    assert tg.groups_t is None and "_groups_t_none" not in tg.__dict__
    had = sv.tg.groups_t
    before = train.backward_library(net, sv, dprobs)
    assert sv.tg.groups_t is had                             # a backward with the switch off builds nothing
    try:
        assert train.set_nnconv_bwd_eg(1) == 0 and train.set_nnconv_bwd_eg(-1) == 1 and train.set_nnconv_bwd_eg(7) == 1
        assert train.set_mlp_bwd_fused(-1) == 0 and train.set_mlp_bwd_tall64(-1) == 0       # a switch of its own
    finally:
        assert train.set_nnconv_bwd_eg(0) == 1
    after = train.backward_library(net, sv, dprobs)
    assert sorted(before) == sorted(after)
    for k in before:
        assert torch.equal(before[k], after[k]), k
    net63, sv63, dp63 = _forward("directed", 3, width, T=63)
    off = train.backward_library(net63, sv63, dp63)
    with _switches(1):
        on = train.backward_library(net63, sv63, dp63)
        on_py = train.backward_train(net63, sv63, dp63)
    for k in off:
        assert torch.equal(off[k], on[k]) and torch.equal(off[k].reshape(-1), on_py[k].reshape(-1)), k


@pytest.mark.parametrize("others", [0, 1])
@pytest.mark.parametrize("depth", [3, 20])
@pytest.mark.parametrize("graph", ["laby", "directed"])
@pytest.mark.parametrize("width", WIDTHS)
def test_switch_on_library_backward_equals_the_spelled_out_schedule(width, graph, depth, others):
    """tgnn_backward_groups and train.backward_train under the new switch, the four older switches off and on (the forward that
    fills the kept buffers runs under them too): the same kernels in the same order, the same bits -- and not the chain's bits: the
    kernel did run."""
    from tilingnn_amd import train
    with _switches(0, others):
        net, sv, dprobs = _forward(graph, depth, width)
        off = train.backward_library(net, sv, dprobs)
    with _switches(1, others):
        a = train.backward_library(net, sv, dprobs)
        b = train.backward_train(net, sv, dprobs)
    assert sv.tg.groups_t is not None
    assert sorted(a) == sorted(b) == sorted(k for k, _ in net.named_parameters())
    for k in a:
        assert torch.isfinite(a[k]).all(), k
        assert torch.equal(a[k].reshape(-1), b[k].reshape(-1)), k
    root = f"brch_1_graph_conv_layers.{depth - 1}.nnConv.root"     # the last layer's: nothing amplifies the difference
    assert _rel(a[root], off[root]) < 1e-4
    assert not torch.equal(a[root], off[root])


# ---------------------------------------------------------------------------------------------- 7. one whole training step
@pytest.mark.parametrize("width", WIDTHS)
def test_one_training_step_through_trainer_with_the_switch_on(width, tmp_path):
    """Forward, loss, backward and Adam through Trainer.train_step on the labyrinth layout with the switch on; the gradients against
    the fp64 oracle with the whole-step gate of tests/test_training_hip.py / tests/test_training_width64.py (its reasoning is
    above GRAD_SEEDS there): nine seeds, no seed's worst parameter beyond max(0.06, 2 x the float32 oracle's worst), and the third
    best seed within 4 x of the float32 oracle's own error (two rounding realisations, per parameter the larger)."""
    from tilingnn_amd.graph_networks.networks.TilinGNN import TilinGNN
    from tilingnn_amd.solver.ml_solver.trainer import Trainer
    from tilingnn_amd.weights import make_state_dict
    from tests.test_training_width64 import GRAD_SEEDS, _f32_oracle_err
    x, adj, attr, col, _ = graph_tensors(load_labyrinth_graph(), torch.float32, DEV)
    layout = SimpleNamespace(node_feature=x, align_edge_index=adj, align_edge_features=attr, collide_edge_index=col)
    fe, depth = 15, 3
    torch.set_num_threads(8)
    worst = []
    for seed in GRAD_SEEDS:
        net = TilinGNN(adj_edge_features_dim=fe, network_depth=depth, network_width=width, node_features_dim=3)
        sd = make_state_dict(fe, depth, width, 1, 3, seed=seed)
        net.load_state_dict(sd)
        net = net.to(DEV).train()
        net.autograd = True
        before = {k: p.detach().clone() for k, p in net.named_parameters()}
        opt = torch.optim.Adam(net.parameters(), lr=1e-3)
        with _switches(1):
            loss = Trainer(None, None, DEV, net, str(tmp_path)).train_step(layout, opt)
        _, ref_loss, _, ref_grads = orc.training_step_grads(orc.cast_sd(sd, torch.float64), x.double().cpu(), adj.cpu(),
                                                            attr.double().cpu(), col.cpu())
        assert abs(float(loss) - float(ref_loss)) < 1e-4 * float(ref_loss)
        err32 = _f32_oracle_err(sd, x.cpu(), adj.cpu(), attr.cpu(), col.cpu(), ref_grads)
        floor = float(np.median(list(err32.values())))
        errs = {k: _rel(p.grad, ref_grads[k]) for k, p in net.named_parameters()}
        assert set(errs) == set(err32)
        print(f"width {width} seed {seed}: worst parameter ours {max(errs.values()):.2e}, float32 oracle's worst "
              f"{max(err32.values()):.2e}, float32 oracle's median {floor:.2e}")
        assert max(errs.values()) < max(0.06, 2.0 * max(err32.values())), max(errs.items(), key=lambda kv: kv[1])
        worst.append(max(e / (max(err32[k], floor) + 2.5e-6) for k, e in errs.items()))
        for k, p in net.named_parameters():                  # Adam moved every parameter that has a gradient
            assert torch.isfinite(p).all() and (not bool(p.grad.abs().max() > 0) or not torch.equal(p.detach(), before[k])), k
    print("worst parameter, ours / float32 oracle, per seed:", [f"{w:.1f}" for w in worst])
    assert sorted(worst)[2] <= 4.0, worst
