"""The fused adjoints of the 3-layer sigmoid MLP (tilingnn_amd/csrc/mlp_bwd.hip: tgnn_sigmoid_mlp_bwd_fused, the tall form for
GINConv's MLP at width 32 and the wide form for GraphConv's edge MLP) as ops against fp64 autograd, and their opt-in route through
tgnn_backward / train.backward_train (tgnn_set_mlp_bwd_fused, train.set_mlp_bwd_fused).

Every op check has two gates: 1e-5 of the expectation's largest magnitude (what tests/test_training_sizes.py holds these adjoints
to), and the error of the chain of generic kernels (tgnn_sigmoid_mlp_bwd) on the same inputs times 4."""
import functools

import pytest
import torch

from oracle import tilingnn_oracle as orc
from tests.golden_util import graph_tensors, load_labyrinth_graph
from tests.test_training_sizes import FE, _gate, _net, _prepared, _rel, _rng
from tests.train_graphs import N_BIG, N_MID

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
GATE, RATIO = 1e-5, 4.0
NAMES = [f"mlp.{k}" for k in range(3)]
KEYS = [f"mlp.{k}.linear.{w}" for k in range(3) for w in ("weight", "bias")]


class _switched_on:
    def __enter__(self):
        from tilingnn_amd import train
        self.prev = train.set_mlp_bwd_fused(1)

    def __exit__(self, *exc):
        from tilingnn_amd import train
        train.set_mlp_bwd_fused(self.prev)


def _autograd64(x, w, d_out, want_dx):
    """fp64 autograd of three Linear + Sigmoid layers on the CPU -> (t3, {gradient name: expectation}, layer-1 pre-activations)."""
    xx = x.double().requires_grad_(want_dx)
    ww = [v.double().requires_grad_(True) for v in w]
    pre1 = xx @ ww[0].t() + ww[1]
    t3 = torch.sigmoid(torch.sigmoid(torch.sigmoid(pre1) @ ww[2].t() + ww[3]) @ ww[4].t() + ww[5])
    (t3 * d_out.double()).sum().backward()
    want = {KEYS[k]: ww[k].grad for k in range(6)}
    if want_dx:
        want["dx"] = xx.grad
    return t3.detach(), want, pre1.detach()


@functools.lru_cache(maxsize=None)
def _tall_inputs(n, mag):
    """Inputs of the tall form and their fp64 expectations; built once, read only.  x = randn mag, one row in a hundred (rows 37,
    137, ...) a further 50 times larger; W1 = randn 2 / (mag sqrt 32): layer-1 pre-activations of standard deviation about 2."""
    r = _rng(1000 + n + int(mag * 7))
    x = r(n, 32) * mag
    x[37::100] *= 50.0
    w = [r(32, 32) * (2.0 / (mag * 32 ** 0.5)), 0.5 * r(32), r(64, 32) * (2.0 / 32 ** 0.5), 0.5 * r(64),
         r(32, 64) * (2.0 / 64 ** 0.5), 0.5 * r(32)]
    d_out = r(n, 32)
    t3, want, pre1 = _autograd64(x, w, d_out, True)
    inside = float((pre1.abs() <= 4.0).double().mean())
    assert inside >= 0.90, inside                            # N(0, 2^2): 95.4 %, less the hub rows
    for k, v in want.items():
        assert float(v.abs().max()) > 0.0, k                 # saturated sigmoids would make every gate vacuous
    return x, w, t3.float(), d_out, want


@functools.lru_cache(maxsize=None)
def _tall_case(n, mag):
    x, w, t3, d_out, want = _tall_inputs(n, mag)
    return x.to(DEV), [v.to(DEV) for v in w], t3.to(DEV), d_out.to(DEV), want


@functools.lru_cache(maxsize=None)
def _wide_case(T, fe, c):
    """Inputs of the wide form as tgnn_backward holds them: T attribute rows in U(0, 1), d_out the first T matrices of a
    [(T + 1), c, c] buffer."""
    r = _rng(2000 + 100 * T + 10 * fe + c)
    g = torch.Generator().manual_seed(T + fe + c)
    x = torch.rand(T, fe, generator=g)
    w = [r(32, fe) * (2.0 / fe ** 0.5), 0.5 * r(32), r(64, 32) * (2.0 / 32 ** 0.5), 0.5 * r(64),
         r(c * c, 64) * (2.0 / 64 ** 0.5), 0.5 * r(c * c)]
    buf = r(T + 1, c, c)
    t3, want, _ = _autograd64(x, w, buf[:T].reshape(T, c * c), False)
    for k, v in want.items():
        assert float(v.abs().max()) > 0.0, k
    return x.to(DEV), [v.to(DEV) for v in w], t3.float().to(DEV), buf.to(DEV), want


def _run(kernel, x, w, t3, d_out, want_dx):
    from tilingnn_amd import train
    grads = {}
    dx = train.sigmoid_mlp_backward(w, x, t3, d_out, grads, NAMES, want_dx, kernel=kernel)
    if want_dx:
        grads["dx"] = dx
    else:
        assert dx is None
    return grads


def _both_gates(what, x, w, t3, d_out, want, want_dx):
    fused, chain = _run("fused", x, w, t3, d_out, want_dx), _run("chain", x, w, t3, d_out, want_dx)
    assert sorted(fused) == sorted(k for k in want if want_dx or k != "dx")
    worst = []
    for k in fused:
        ef, ec = _rel(fused[k], want[k]), _rel(chain[k], want[k])
        print(f"{what} {k}: fused {ef:.2e} chain {ec:.2e} ratio {ef / max(ec, 1e-30):.2f} (gates {GATE:.0e}, {RATIO:.0f})")
        worst.append((k, ef, ec))
    for k, ef, ec in worst:
        assert torch.isfinite(fused[k]).all(), (what, k)
        assert ef < GATE, (what, k, ef)
        assert ef < RATIO * ec, (what, k, ef, ec)
    return fused


# ---------------------------------------------------------------------------------------------- 1. the tall op
TALL = [(n, 1.0) for n in (1, 15, 16, 17, 127, 129, 1254, 4099, 66003)] + [(n, m) for n in (1254, 4099) for m in (1e-3, 1e2)]


@pytest.mark.parametrize("n,mag", TALL)
def test_tall_op_against_fp64(n, mag):
    """(32, 32, 64, 32) on n rows: one row, one short tile, one full tile, a tile and a row, short last tiles, the labyrinth's
    size (20 blocks, one tile per SIMD), 4 099 rows (65 blocks), 66 003 rows (256 persistent blocks, several tiles per wave)."""
    from tilingnn_amd._lib import lib
    assert lib.tgnn_sigmoid_mlp_bwd_fused_form(n, 32, 32, 64, 32, 1) == 1
    x, w, t3, d_out, want = _tall_case(n, mag)
    _both_gates(f"tall n={n} mag={mag:g}", x, w, t3, d_out, want, True)


@pytest.mark.parametrize("n", [129, 4099])
def test_tall_op_row_stride_and_no_input_gradient(n):
    """d_out as 32 columns of a buffer whose rows are 672 floats apart (the slot of a 21-slot concatenation); dx NULL."""
    x, w, t3, d_out, want = _tall_case(n, 1.0)
    wide = torch.full((n, 672), float("nan"), device=DEV)
    wide[:, 64:96] = d_out
    view = wide[:, 64:96]
    assert view.stride(0) == 672
    strided = _both_gates(f"tall n={n} ld 672", x, w, t3, view, want, True)
    dense = _run("fused", x, w, t3, d_out, True)
    no_dx = _both_gates(f"tall n={n} no dx", x, w, t3, d_out, want, False)
    for k in dense:
        assert torch.equal(dense[k], strided[k]), k
        assert k == "dx" or torch.equal(dense[k], no_dx[k]), k


# ---------------------------------------------------------------------------------------------- 2. the wide op
@pytest.mark.parametrize("c", [32, 64])
@pytest.mark.parametrize("fe", [1, 5, 64])
@pytest.mark.parametrize("T", [1, 2, 13, 18, 63])
def test_wide_op_against_fp64(T, fe, c):
    from tilingnn_amd._lib import lib
    assert lib.tgnn_sigmoid_mlp_bwd_fused_form(T, fe, 32, 64, c * c, 0) == 2
    x, w, t3, buf, want = _wide_case(T, fe, c)
    d_out = buf[:T].reshape(T, c * c)
    assert d_out.stride(0) == c * c and d_out.data_ptr() == buf.data_ptr()
    _both_gates(f"wide T={T} fe={fe} c={c}", x, w, t3, d_out, want, False)


# ---------------------------------------------------------------------------------------------- 3. repeatability
def test_both_forms_give_the_same_bits_on_every_call():
    x, w, t3, d_out, _ = _tall_case(4099, 1.0)
    a, b = _run("fused", x, w, t3, d_out, True), _run("fused", x, w, t3, d_out, True)
    for k in a:
        assert torch.equal(a[k], b[k]), k
    x, w, t3, buf, _ = _wide_case(13, 5, 32)
    d_out = buf[:13].reshape(13, 1024)
    a, b = _run("fused", x, w, t3, d_out, False), _run("fused", x, w, t3, d_out, False)
    for k in a:
        assert torch.equal(a[k], b[k]), k


# ---------------------------------------------------------------------------------------------- 4. refusals
@pytest.mark.parametrize("n,dims,want_dx", [(300, (64, 32, 64, 64), True), (64, (15, 32, 64, 1024), False),
                                            (13, (15, 32, 64, 1024), True)])
def test_refusals_launch_nothing_and_write_nothing(n, dims, want_dx):
    """Width 64's GIN MLP, 64 rows of the wide shape and the wide shape with an input gradient: TGNN_ERR_UNSUPPORTED with the
    message set, every output still the sentinel -- no fall-back to the chain."""
    from tilingnn_amd import _lib, train
    from tilingnn_amd._lib import lib, ptr
    d0, d1, d2, d3 = dims
    assert lib.tgnn_sigmoid_mlp_bwd_fused_form(n, d0, d1, d2, d3, int(want_dx)) == 0
    r = _rng(n + d0)
    x, t3, d_out = r(n, d0).to(DEV), torch.rand(n, d3).to(DEV), r(n, d3).to(DEV)
    w = [v.to(DEV) for v in (r(d1, d0), r(d1), r(d2, d1), r(d2), r(d3, d2), r(d3))]
    outs = [torch.full_like(v, 12345.0) for v in w] + [torch.full((n, d0), 12345.0, device=DEV)]
    ws = torch.full((1 << 20,), 7, dtype=torch.uint8, device=DEV)
    rc = lib.tgnn_sigmoid_mlp_bwd_fused(ptr(x), n, d0, d1, d2, d3, ptr(w[0]), ptr(w[1]), ptr(w[2]), ptr(w[3]), ptr(w[4]), ptr(t3),
                                        ptr(d_out), d3, *(ptr(v) for v in outs[:6]), ptr(outs[6] if want_dx else None), ptr(ws),
                                        ws.numel(), train._s(x))
    torch.cuda.synchronize()
    assert rc == _lib.ERR_UNSUPPORTED and b"no fused form" in lib.tgnn_last_error()
    for v in outs:
        assert bool((v == 12345.0).all())
    assert bool((ws == 7).all())
    with pytest.raises(_lib.TgnnError):
        train.sigmoid_mlp_backward(w, x, t3, d_out, {}, NAMES, want_dx, kernel="fused")


# ---------------------------------------------------------------------------------------------- 5 .. 8: the route
@functools.lru_cache(maxsize=None)
def _forward(graph, depth, width):
    """One training forward on the labyrinth layout (1 254 nodes, fe 15) or the 4 099-row directed graph; kept, read only."""
    from tilingnn_amd import train
    if graph == "laby":
        x, adj, attr, col, _ = graph_tensors(load_labyrinth_graph(), torch.float32, DEV)
    else:
        p = _prepared(N_MID, 13)
        x, adj, attr, col = p.x, p.adj, p.attr, p.col
    net, _ = _net(int(attr.shape[1]), depth, 6, width)
    probs, sv = train.forward_train(net, x, adj, attr, col)
    dprobs = _rng(depth + width)(int(x.shape[0]), 1).to(DEV) * 1e-2
    return net, sv, dprobs


def test_switch_off_is_the_code_as_it_stands():
    from tilingnn_amd import train
    assert train.set_mlp_bwd_fused(-1) == 0                  # the default
    net, sv, dprobs = _forward("laby", 3, 32)
    before = train.backward_library(net, sv, dprobs)
    try:
        assert train.set_mlp_bwd_fused(1) == 0 and train.set_mlp_bwd_fused(-1) == 1 and train.set_mlp_bwd_fused(7) == 1
    finally:
        assert train.set_mlp_bwd_fused(0) == 1
    after = train.backward_library(net, sv, dprobs)
    assert sorted(before) == sorted(after)
    for k in before:
        assert torch.equal(before[k], after[k]), k


@pytest.mark.parametrize("width", [32, 64])
@pytest.mark.parametrize("depth", [3, 20])
@pytest.mark.parametrize("graph", ["laby", "directed"])
def test_switch_on_library_backward_equals_the_spelled_out_schedule(graph, depth, width):
    """tgnn_backward and train.backward_train under the switch: the same kernels in the same order, the same bits.  Width 64 keeps
    the chain for GIN and takes the wide kernels for the edge MLP."""
    from tilingnn_amd import train
    from tilingnn_amd._lib import lib
    net, sv, dprobs = _forward(graph, depth, width)
    n, T = sv.n, sv.tg.g.n_types
    assert lib.tgnn_sigmoid_mlp_bwd_fused_form(n, width, 32, 64, width, 1) == (1 if width == 32 else 0)
    assert 1 <= T <= 63 and lib.tgnn_sigmoid_mlp_bwd_fused_form(T, FE, 32, 64, width * width, 0) == 2
    off = train.backward_library(net, sv, dprobs)
    with _switched_on():
        a = train.backward_library(net, sv, dprobs)
        b = train.backward_train(net, sv, dprobs)
    assert sorted(a) == sorted(b) == sorted(k for k, _ in net.named_parameters())
    for k in a:
        assert torch.isfinite(a[k]).all(), k
        assert torch.equal(a[k].reshape(-1), b[k].reshape(-1)), k
    # the two settings are two fp32 roundings of the same gradient (the last layer's: nothing amplifies the difference), each
    # within 1e-5 of fp64 by the op tests
    edge = "brch_1_graph_conv_layers.%d.mlp.mlp.2.linear.weight" % (depth - 1)
    assert _rel(a[edge], off[edge]) < 1e-4


@pytest.mark.parametrize("width", [32, 64])
@pytest.mark.parametrize("n,T", [(N_MID, 13), (N_MID, 63), (N_BIG, 13)])
def test_switch_on_adjoints_teacher_forced_on_the_directed_graph(n, T, width):
    """tests/test_training_sizes.py::test_nnconv_and_gin_adjoints_teacher_forced_on_the_directed_graph with the switch on: the
    composed NNConv and GIN adjoints against fp64 autograd over the oracle's ops, its 1e-5 gates."""
    from tilingnn_amd import ops, train
    torch.set_num_threads(8)
    p = _prepared(n, T)
    tg, attr = p.tg, p.attr
    _, adj_c, attr_c, col_c = p.cpu
    net, sd = _net(FE, 2, 5, width)
    sd64 = orc.cast_sd(sd, torch.float64)
    r = _rng(11 + width)
    h, dz = r(n, width).to(DEV), r(n, width).to(DEV)
    l1, l2 = net.brch_1_graph_conv_layers[1], net.brch_2_coll_conv_layers[1]
    p1, p2 = "brch_1_graph_conv_layers.1", "brch_2_coll_conv_layers.1"
    wtab = ops.edge_weight_table(attr, tg.g, *l1.nnConv._edge_mlp_params(), width).contiguous()
    u = train.gin_aggregate(h, tg.g.col_rowptr, tg.g.col_src, l2.ginConv.eps, n)
    gw = l2.ginConv._mlp_params()
    t1 = ops.dense_act(u, gw[0], gw[1], ops.ACT_SIGMOID)[0]
    t3 = ops.dense_act(ops.dense_act(t1, gw[2], gw[3], ops.ACT_SIGMOID)[0], gw[4], gw[5], ops.ACT_SIGMOID)[0]
    g1, g2 = {}, {}
    with _switched_on():
        dh = train.nnconv_backward(l1.nnConv, p1, tg, wtab, h, dz, dz * tg.inv_deg[:, None], attr, g1)
        dh2 = train.gin_backward(l2.ginConv, p2, tg, u, t3, dz, g2)

    leaf = {k: (v.clone().requires_grad_(True) if k.startswith(p1) and v.is_floating_point() else v) for k, v in sd64.items()}
    hh = h.double().cpu().requires_grad_(True)
    out = orc.nnconv_mean_dedup(hh, adj_c, attr_c.double(), leaf, p1)
    (out * dz.double().cpu()).sum().backward()
    _gate("NNConv dh", dh, hh.grad, 1e-5)
    for k, v in g1.items():
        _gate(k, v.reshape(leaf[k].shape), leaf[k].grad, 1e-5)
    assert set(g1) == {p1 + ".nnConv.root", p1 + ".nnConv.bias"} | {f"{p1}.mlp.mlp.{k}.linear.{w}" for k in range(3)
                                                                    for w in ("weight", "bias")}
    leaf = {k: (v.clone().requires_grad_(True) if k.startswith(p2) and v.is_floating_point() and not k.endswith(".eps")
                else v) for k, v in sd64.items()}
    out = orc.gin_conv(hh := h.double().cpu().requires_grad_(True), col_c, leaf, p2)
    (out * dz.double().cpu()).sum().backward()
    _gate("GIN dh", dh2, hh.grad, 1e-5)
    for k, v in g2.items():
        _gate(k, v.reshape(leaf[k].shape), leaf[k].grad, 1e-5)
    assert set(g2) == {f"{p2}.ginConv.nn.mlp.{k}.linear.{w}" for k in range(3) for w in ("weight", "bias")}


def test_one_training_step_with_the_switch_on():
    """Forward, loss, backward, Adam on the labyrinth layout: the loss is the switch-off step's bit for bit (the forward is
    untouched), BatchNorm's counter moves by one, the updated parameters are finite."""
    from tilingnn_amd.solver.ml_solver.losses import Losses
    x, adj, attr, col, _ = graph_tensors(load_labyrinth_graph(), torch.float32, DEV)

    def step():
        net, _ = _net(int(attr.shape[1]), 3, 9, 32)
        net.autograd = True
        bn = net.brch_2_coll_conv_layers[0].batch_norm
        start = int(bn.num_batches_tracked)
        opt = torch.optim.Adam(net.parameters(), lr=1e-3)
        opt.zero_grad()
        probs, _ = net(x, adj, attr, col)
        loss, _, _ = Losses.calculate_unsupervised_loss(probs, x, col, adj, attr)
        loss.backward()
        opt.step()
        return net, loss.detach().clone(), int(bn.num_batches_tracked) - start

    _, loss_off, _ = step()
    with _switched_on():
        net, loss_on, moved = step()
    assert moved == 1
    assert torch.equal(loss_on, loss_off)
    for k, p in net.named_parameters():
        assert p.grad is not None and torch.isfinite(p.grad).all() and torch.isfinite(p).all(), k
