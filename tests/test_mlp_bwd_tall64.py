"""The fused adjoint of GINConv's MLP at width 64 (tilingnn_amd/csrc/mlp_bwd.hip: mlp_bwd_tall64_kernel behind
tgnn_sigmoid_mlp_bwd_tall64, 64 -> 32 -> 64 -> 64) as an op against fp64 autograd, and its opt-in route through tgnn_backward /
train.backward_train (tgnn_set_mlp_bwd_tall64, train.set_mlp_bwd_tall64) under both settings of the older switch.

Every op check has the two gates of tests/test_mlp_bwd_fused.py: 1e-5 of the expectation's largest magnitude, and the error of the
chain of generic kernels (tgnn_sigmoid_mlp_bwd) on the same inputs times 4."""
import functools

import pytest
import torch

from oracle import tilingnn_oracle as orc
from tests.golden_util import graph_tensors, load_labyrinth_graph
from tests.test_mlp_bwd_fused import GATE, NAMES, RATIO, _autograd64, _forward, _run
from tests.test_training_sizes import FE, _gate, _net, _prepared, _rel, _rng
from tests.train_graphs import N_BIG, N_MID

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
DIMS = (64, 32, 64, 64)
ERR_INVALID_ARG = -1                                         # TGNN_ERR_INVALID_ARG (include/tgnn.h)
GIN_LAST = "brch_2_coll_conv_layers.%d.ginConv.nn.mlp.2.linear.weight"


class _switches:
    """tall64 = the new switch, fused = tgnn_set_mlp_bwd_fused; both put back on exit."""

    def __init__(self, tall64, fused=0):
        self.want = (tall64, fused)

    def __enter__(self):
        from tilingnn_amd import train
        self.prev = (train.set_mlp_bwd_tall64(self.want[0]), train.set_mlp_bwd_fused(self.want[1]))

    def __exit__(self, *exc):
        from tilingnn_amd import train
        train.set_mlp_bwd_tall64(self.prev[0])
        train.set_mlp_bwd_fused(self.prev[1])


def _blocks(n):
    """The grid the plan gives n rows, from the workspace query: blocks x one partial row, rounded up to 256 bytes."""
    from tilingnn_amd._lib import lib
    row = (32 * 64 + 32 + 64 * 32 + 64 + 64 * 64 + 64) * 4
    return int(lib.tgnn_sigmoid_mlp_bwd_tall64_workspace_bytes(n, *DIMS)) // row


@functools.lru_cache(maxsize=None)
def _first_n_at_the_cap():
    cap = _blocks(10 ** 7)
    lo, hi = 1, 10 ** 7                                      # blocks(lo) < cap <= blocks(hi); the grid never shrinks with n
    assert _blocks(lo) < cap
    while hi - lo > 1:
        mid = (lo + hi) // 2
        lo, hi = (lo, mid) if _blocks(mid) == cap else (mid, hi)
    return hi


@functools.lru_cache(maxsize=None)
def _inputs(n, mag):
    """Inputs at width 64 and their fp64 expectations; built once, read only.  x = randn mag, one row in a hundred (rows 37, 137,
    ...) a further 50 times larger; W1 = randn 2 / (mag sqrt 64): layer-1 pre-activations of standard deviation about 2."""
    r = _rng(3000 + n + int(mag * 7))
    x = r(n, 64) * mag
    x[37::100] *= 50.0
    w = [r(32, 64) * (2.0 / (mag * 64 ** 0.5)), 0.5 * r(32), r(64, 32) * (2.0 / 32 ** 0.5), 0.5 * r(64),
         r(64, 64) * (2.0 / 64 ** 0.5), 0.5 * r(64)]
    d_out = r(n, 64)
    t3, want, pre1 = _autograd64(x, w, d_out, True)
    inside = float((pre1.abs() <= 4.0).double().mean())
    assert inside >= 0.90, inside                            # N(0, 2^2): 95.4 %, less the hub rows
    for k, v in want.items():
        assert float(v.abs().max()) > 0.0, k                 # saturated sigmoids would make every gate vacuous
    return x, w, t3.float(), d_out, want


@functools.lru_cache(maxsize=None)
def _case(n, mag=1.0):
    x, w, t3, d_out, want = _inputs(n, mag)
    return x.to(DEV), [v.to(DEV) for v in w], t3.to(DEV), d_out.to(DEV), want


def _both_gates(what, x, w, t3, d_out, want, want_dx):
    new, chain = _run("tall64", x, w, t3, d_out, want_dx), _run("chain", x, w, t3, d_out, want_dx)
    assert sorted(new) == sorted(k for k in want if want_dx or k != "dx")
    worst = []
    for k in new:
        ef, ec = _rel(new[k], want[k]), _rel(chain[k], want[k])
        print(f"{what} {k}: tall64 {ef:.2e} chain {ec:.2e} ratio {ef / max(ec, 1e-30):.2f} (gates {GATE:.0e}, {RATIO:.0f})")
        worst.append((k, ef, ec))
    for k, ef, ec in worst:
        assert torch.isfinite(new[k]).all(), (what, k)
        assert ef < GATE, (what, k, ef)
        assert ef < RATIO * ec, (what, k, ef, ec)
    return new


# ---------------------------------------------------------------------------------------------- 1. the op
SIZES = [(n, 1.0) for n in (1, 15, 16, 17, 63, 65, 127, 129, 1254, 4099, 66003)] + [(n, m) for n in (1254, 4099) for m in (1e-3, 1e2)]


@pytest.mark.parametrize("n,mag", SIZES)
def test_op_against_fp64(n, mag):
    """(64, 32, 64, 64) on n rows: one row, one short tile, one full tile, a tile and a row, one block short of a row and one row
    into the second block, short last tiles, the labyrinth's size (20 blocks, a tile per wave), 4 099 rows (65 blocks), 66 003
    rows (256 persistent blocks, several tiles per wave)."""
    from tilingnn_amd._lib import lib
    assert lib.tgnn_sigmoid_mlp_bwd_tall64_ok(n, *DIMS) == 1
    _both_gates(f"tall64 n={n} mag={mag:g}", *_case(n, mag), True)


@pytest.mark.parametrize("side", ["below", "at"])
def test_op_against_fp64_on_either_side_of_the_grid_cap(side):
    """The last n whose grid is still a tile per wave and the first n at 256 blocks, where a wave gets its second tile."""
    first = _first_n_at_the_cap()
    n = first - 1 if side == "below" else first
    cap = _blocks(10 ** 7)
    assert cap == 256 and _blocks(first) == cap and _blocks(first - 1) == cap - 1
    _both_gates(f"tall64 n={n} ({side} the cap)", *_case(n), True)


# ---------------------------------------------------------------------------------------------- 2. stride, no dx
@pytest.mark.parametrize("n", [129, 4099])
def test_op_row_stride_and_no_input_gradient(n):
    """d_out as 64 columns of a buffer whose rows are 1 344 floats apart (a slot of the 21-slot concatenation); dx NULL."""
    x, w, t3, d_out, want = _case(n)
    wide = torch.full((n, 1344), float("nan"), device=DEV)
    wide[:, 128:192] = d_out
    view = wide[:, 128:192]
    assert view.stride(0) == 1344
    strided = _both_gates(f"tall64 n={n} ld 1344", x, w, t3, view, want, True)
    dense = _run("tall64", x, w, t3, d_out, True)
    no_dx = _both_gates(f"tall64 n={n} no dx", x, w, t3, d_out, want, False)
    assert len(dense) == 7
    for k in dense:
        assert torch.equal(dense[k], strided[k]), k
        assert k == "dx" or torch.equal(dense[k], no_dx[k]), k


# ---------------------------------------------------------------------------------------------- 3. repeatability
@pytest.mark.parametrize("n", [4099, 66003])
def test_same_bits_on_every_call(n):
    x, w, t3, d_out, _ = _case(n)
    a, b = _run("tall64", x, w, t3, d_out, True), _run("tall64", x, w, t3, d_out, True)
    assert len(a) == 7
    for k in a:
        assert torch.equal(a[k], b[k]), k


# ---------------------------------------------------------------------------------------------- 4. the dx tail
def _call(x, n, dims, w, t3, d_out, ld, outs, dx, ws):
    from tilingnn_amd import train
    from tilingnn_amd._lib import lib, ptr
    rc = lib.tgnn_sigmoid_mlp_bwd_tall64(ptr(x), n, *dims, ptr(w[0]), ptr(w[1]), ptr(w[2]), ptr(w[3]), ptr(w[4]), ptr(t3), ptr(d_out),
                                         ld, *(ptr(v) for v in outs), ptr(dx), ptr(ws), ws.numel(), train._s(w[0]))
    torch.cuda.synchronize()
    return rc


@pytest.mark.parametrize("n", [17, 1254])
def test_dx_rows_behind_n_are_not_written(n):
    """The last tile is short (n = 17: 15 rows of it, 1 254: 10): the clamped rows compute, the store is masked."""
    x, w, t3, d_out, want = _case(n)
    dx = torch.full((n + 16, 64), 12345.0, device=DEV)
    outs = [torch.empty_like(v) for v in w]
    ws = torch.empty(1 << 22, dtype=torch.uint8, device=DEV)
    assert _call(x, n, DIMS, w, t3, d_out, 64, outs, dx, ws) == 0
    assert bool((dx[n:] == 12345.0).all())
    assert _rel(dx[:n], want["dx"]) < GATE


# ---------------------------------------------------------------------------------------------- 5. refusals
@pytest.mark.parametrize("n,dims", [(300, (32, 32, 64, 32)), (300, (64, 32, 64, 32)), (13, (15, 32, 64, 4096))])
def test_refusals_launch_nothing_and_write_nothing(n, dims):
    """Width 32's GIN MLP, a narrower output and the edge MLP's shape: TGNN_ERR_UNSUPPORTED with the message set, every output and
    the workspace still the sentinel -- no fall-back to another kernel."""
    from tilingnn_amd import _lib, train
    from tilingnn_amd._lib import lib
    d0, d1, d2, d3 = dims
    assert lib.tgnn_sigmoid_mlp_bwd_tall64_ok(n, *dims) == 0 and lib.tgnn_sigmoid_mlp_bwd_tall64_workspace_bytes(n, *dims) == 0
    r = _rng(n + d0)
    x, t3, d_out = r(n, d0).to(DEV), torch.rand(n, d3).to(DEV), r(n, d3).to(DEV)
    w = [v.to(DEV) for v in (r(d1, d0), r(d1), r(d2, d1), r(d2), r(d3, d2), r(d3))]
    outs = [torch.full_like(v, 12345.0) for v in w]
    dx = torch.full((n, d0), 12345.0, device=DEV)
    ws = torch.full((1 << 20,), 7, dtype=torch.uint8, device=DEV)
    rc = _call(x, n, dims, w, t3, d_out, d3, outs, dx, ws)
    assert rc == _lib.ERR_UNSUPPORTED and b"no tall64 form" in lib.tgnn_last_error()
    for v in outs + [dx]:
        assert bool((v == 12345.0).all())
    assert bool((ws == 7).all())
    with pytest.raises(_lib.TgnnError):
        train.sigmoid_mlp_backward(w, x, t3, d_out, {}, NAMES, True, kernel="tall64")


@pytest.mark.parametrize("fault", ["ld_dout 66", "x off by 4 bytes"])
def test_argument_errors_write_nothing(fault):
    n = 129
    x, w, t3, d_out, _ = _case(n)
    ld = 64
    if fault == "ld_dout 66":
        buf = torch.zeros(n, 66, device=DEV)
        buf[:, :64] = d_out
        d_out, ld = buf, 66
    else:
        flat = torch.zeros(n * 64 + 4, device=DEV)
        x = flat[1:1 + n * 64].view(n, 64)
        assert x.data_ptr() % 16 == 4
    outs = [torch.full_like(v, 12345.0) for v in w]
    dx = torch.full((n, 64), 12345.0, device=DEV)
    ws = torch.full((1 << 20,), 7, dtype=torch.uint8, device=DEV)
    assert _call(x, n, DIMS, w, t3, d_out, ld, outs, dx, ws) == ERR_INVALID_ARG
    for v in outs + [dx]:
        assert bool((v == 12345.0).all())
    assert bool((ws == 7).all())


def test_no_rows_zero_the_six_gradients():
    _, w, _, _, _ = _case(129)
    empty = torch.empty(0, 64, device=DEV)
    outs = [torch.full_like(v, 12345.0) for v in w]
    ws = torch.full((1 << 20,), 7, dtype=torch.uint8, device=DEV)
    assert _call(empty, 0, DIMS, w, empty, empty, 64, outs, None, ws) == 0
    for v in outs:
        assert bool((v == 0.0).all())
    assert bool((ws == 7).all())
    grads = _run("tall64", empty, w, empty, empty, True)
    assert all(bool((v == 0.0).all()) for k, v in grads.items() if k != "dx") and grads["dx"].shape == (0, 64)


# ---------------------------------------------------------------------------------------------- 6. the switch
def test_switch_off_is_the_code_as_it_stands():
    from tilingnn_amd import train
    assert train.set_mlp_bwd_tall64(-1) == 0                 # the default
    net, sv, dprobs = _forward("laby", 3, 64)
    before = train.backward_library(net, sv, dprobs)
    try:
        assert train.set_mlp_bwd_tall64(1) == 0 and train.set_mlp_bwd_tall64(-1) == 1 and train.set_mlp_bwd_tall64(7) == 1
        assert train.set_mlp_bwd_fused(-1) == 0              # a switch of its own
    finally:
        assert train.set_mlp_bwd_tall64(0) == 1
    after = train.backward_library(net, sv, dprobs)
    assert sorted(before) == sorted(after)
    for k in before:
        assert torch.equal(before[k], after[k]), k


def test_switch_changes_no_bit_at_width_32():
    from tilingnn_amd import train
    net, sv, dprobs = _forward("laby", 3, 32)
    off = train.backward_library(net, sv, dprobs)
    with _switches(1):
        on = train.backward_library(net, sv, dprobs)
    assert sorted(off) == sorted(on)
    for k in off:
        assert torch.equal(off[k], on[k]), k


# ---------------------------------------------------------------------------------------------- 7. the route
@pytest.mark.parametrize("fused", [0, 1])
@pytest.mark.parametrize("depth", [3, 20])
@pytest.mark.parametrize("graph", ["laby", "directed"])
def test_switch_on_library_backward_equals_the_spelled_out_schedule(graph, depth, fused):
    """tgnn_backward and train.backward_train at width 64 under the new switch, the older one off and on: the same kernels in the
    same order, the same bits."""
    from tilingnn_amd import train
    from tilingnn_amd._lib import lib
    net, sv, dprobs = _forward(graph, depth, 64)
    assert lib.tgnn_sigmoid_mlp_bwd_tall64_ok(sv.n, 64, 32, 64, 64) == 1
    off = train.backward_library(net, sv, dprobs)
    with _switches(1, fused):
        a = train.backward_library(net, sv, dprobs)
        b = train.backward_train(net, sv, dprobs)
    assert sorted(a) == sorted(b) == sorted(k for k, _ in net.named_parameters())
    for k in a:
        assert torch.isfinite(a[k]).all(), k
        assert torch.equal(a[k].reshape(-1), b[k].reshape(-1)), k
    # two fp32 roundings of the same gradient (the last layer's: nothing amplifies the difference), each within 1e-5 of fp64 by
    # the op tests -- and not the same bits: the kernel did run
    gin = GIN_LAST % (depth - 1)
    assert _rel(a[gin], off[gin]) < 1e-4
    assert not torch.equal(a[gin], off[gin])


# ---------------------------------------------------------------------------------------------- 8. the composed GIN adjoint
@pytest.mark.parametrize("n", [N_MID, N_BIG])
def test_switch_on_gin_adjoint_teacher_forced_on_the_directed_graph(n):
    """tests/test_mlp_bwd_fused.py::test_switch_on_adjoints_teacher_forced_on_the_directed_graph, its GIN part at width 64 under the
    new switch: the composed adjoint against fp64 autograd over the oracle's ops, its 1e-5 gates."""
    from tilingnn_amd import ops, train
    torch.set_num_threads(8)
    width = 64
    p = _prepared(n, 13)
    tg = p.tg
    _, _, _, col_c = p.cpu
    net, sd = _net(FE, 2, 5, width)
    sd64 = orc.cast_sd(sd, torch.float64)
    r = _rng(11 + width)
    h, dz = r(n, width).to(DEV), r(n, width).to(DEV)
    l2, p2 = net.brch_2_coll_conv_layers[1], "brch_2_coll_conv_layers.1"
    u = train.gin_aggregate(h, tg.g.col_rowptr, tg.g.col_src, l2.ginConv.eps, n)
    gw = l2.ginConv._mlp_params()
    t1 = ops.dense_act(u, gw[0], gw[1], ops.ACT_SIGMOID)[0]
    t3 = ops.dense_act(ops.dense_act(t1, gw[2], gw[3], ops.ACT_SIGMOID)[0], gw[4], gw[5], ops.ACT_SIGMOID)[0]
    g2, g_off = {}, {}
    train.gin_backward(l2.ginConv, p2, tg, u, t3, dz, g_off)
    with _switches(1):
        dh2 = train.gin_backward(l2.ginConv, p2, tg, u, t3, dz, g2)
    leaf = {k: (v.clone().requires_grad_(True) if k.startswith(p2) and v.is_floating_point() and not k.endswith(".eps")
                else v) for k, v in sd64.items()}
    out = orc.gin_conv(hh := h.double().cpu().requires_grad_(True), col_c, leaf, p2)
    (out * dz.double().cpu()).sum().backward()
    _gate("GIN dh", dh2, hh.grad, 1e-5)
    for k, v in g2.items():
        _gate(k, v.reshape(leaf[k].shape), leaf[k].grad, 1e-5)
    assert set(g2) == {f"{p2}.ginConv.nn.mlp.{k}.linear.{w}" for k in range(3) for w in ("weight", "bias")}
    assert not torch.equal(g2[p2 + ".ginConv.nn.mlp.2.linear.weight"], g_off[p2 + ".ginConv.nn.mlp.2.linear.weight"])


# ---------------------------------------------------------------------------------------------- 9. a training step
def test_one_width_64_training_step_with_the_switch_on():
    """Forward, loss, backward, Adam on the labyrinth layout at width 64: the loss is the switch-off step's bit for bit (the forward
    is untouched), BatchNorm's counter moves by one, gradients and updated parameters are finite."""
    from tilingnn_amd.solver.ml_solver.losses import Losses
    x, adj, attr, col, _ = graph_tensors(load_labyrinth_graph(), torch.float32, DEV)

    def step():
        net, _ = _net(int(attr.shape[1]), 3, 9, 64)
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
    with _switches(1):
        net, loss_on, moved = step()
    assert moved == 1
    assert torch.equal(loss_on, loss_off)
    for k, p in net.named_parameters():
        assert p.grad is not None and torch.isfinite(p.grad).all() and torch.isfinite(p).all(), k
