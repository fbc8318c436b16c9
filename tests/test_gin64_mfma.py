"""GINConv's MLP at network_width 64, fp32, on the matrix cores (csrc/gin64_mlp.hip: gin64_mlp_kernel behind the gather kernel;
tgnn_gin64_fwd, ops.gin(kernel="mfma")) and its opt-in route through tgnn_forward / tgnn_forward_train (tgnn_set_gin64_mfma,
default off).  Reference semantics: CollConv.forward, graph_networks/layers/coll_conv.py:24-27 of the reference (the oracle's
gin_conv, LeakyReLU behind it).

* the op against the pinned fp64 oracle at 1 ... 66 003 nodes (66 003: past 224 blocks x 128 rows -- waves walk more than one
  tile), rows without collision edges, self loops, a hub row of 500 in-edges, with and without a folded BatchNorm record, with and
  without LeakyReLU, magnitudes 1e-3 ... 1e3, BatchNorm partial sums, bit-repeatability; the generic kernel's error beside it;
* the refusals of the entry points;
* the forward's routing (switch on: the kept buffers ARE the new op on the kept operands; switch off: the bits of before), eval
  mode, the kept buffers and one training step against the fp64 oracle with the switch on, a ragged general-schedule forward.
"""
import ctypes as C
import types

import pytest
import torch

from oracle import tilingnn_oracle as orc
from tests.golden_util import graph_tensors, load_labyrinth_graph

pytestmark = pytest.mark.gpu
W = 64
GATE = 1e-6          # of the output's max-norm: the project's gate for this op (tests/test_gin_fused.py)
PREFIX = "c"


@pytest.fixture(scope="module")
def dev():
    if not torch.cuda.is_available():
        pytest.skip("needs a GPU")
    return torch.device("cuda:0")


@pytest.fixture()
def switch_on():
    from tilingnn_amd import ops
    prev = ops.set_gin64_mfma(1)
    try:
        yield
    finally:
        ops.set_gin64_mfma(prev)


# ---------------------------------------------------------------------------------------------- the op
def collision_edges(n, seed):
    """[2, E] int64 on the CPU.  1 254: the labyrinth layout's collision edges.  Else 3 n random edges, the first few turned into
    self loops (the CSR drops them), rows n - 7 .. n - 1 without in-edges (n > 16), and from 1 254 nodes on 500 edges into row 5."""
    if n == 1254:
        return graph_tensors(load_labyrinth_graph(), torch.float32, "cpu")[3]
    g = torch.Generator().manual_seed(seed)
    e = 3 * n
    src = torch.randint(0, n, (e,), generator=g)
    dst = torch.randint(0, n - 7 if n > 16 else n, (e,), generator=g)
    k = min(4, e)
    src[:k] = dst[:k]                                        # self loops
    if n > 1254:
        src = torch.cat([src, torch.randint(0, n, (500,), generator=g)])
        dst = torch.cat([dst, torch.full((500,), 5)])
    return torch.stack([src, dst])


def gin_weights(ei, n, seed, in_scale=1.0):
    """State-dict entries of one GINConv (fp32, CPU) for rows of magnitude in_scale.  Scales: layer 1's pre-activations get a
    standard deviation of ~2 -- W1 ~ 0.25 / (in_scale sqrt(1 + mean in-degree)), 64 inputs of variance in_scale^2 ((1 + eps)^2 +
    degree) -- so the first sigmoid is not saturated; layers 2 / 3 see sigmoids in (0, 1).
    Why W1 follows the magnitude of the rows: the MLP reads the aggregate z as fp32, 2^-24 of |z| off the exact sum, and the
    output moves by up to a quarter of the error of a pre-activation, ~2^-24 sum_k |W1_k z_k|.  The gate of 1e-6 therefore says
    something about a KERNEL only where sum_k |W1_k z_k| is of order 1 - 10, which is also where the network runs it (rows
    behind a BatchNorm).  With W1 fixed and rows of 1e3 the terms are ~1e3 and every fp32 kernel is 1e-5 ... 4e-5 off in the few
    entries that cancel to an unsaturated value (measured on an MI355X: this kernel 7e-6 ... 4.0e-5, the generic kernel
    9e-7 ... 2.7e-5 on the same inputs); rows of 1e-3 would leave the output a function of the bias alone.  Scaled this way the
    three magnitudes exercise the split of operands whose exponents are 20 binary orders apart."""
    g = torch.Generator().manual_seed(seed)
    keep = ei[0] != ei[1]
    mean_deg = float(keep.sum()) / n
    s1 = 0.25 / (1.0 + mean_deg) ** 0.5 / in_scale
    return {f"{PREFIX}.ginConv.eps": torch.tensor([0.25]),
            f"{PREFIX}.ginConv.nn.mlp.0.linear.weight": torch.randn(32, W, generator=g) * s1,
            f"{PREFIX}.ginConv.nn.mlp.0.linear.bias": torch.randn(32, generator=g) * 0.3,
            f"{PREFIX}.ginConv.nn.mlp.1.linear.weight": torch.randn(64, 32, generator=g) * 0.4,
            f"{PREFIX}.ginConv.nn.mlp.1.linear.bias": torch.randn(64, generator=g) * 0.3,
            f"{PREFIX}.ginConv.nn.mlp.2.linear.weight": torch.randn(W, 64, generator=g) * 0.4,
            f"{PREFIX}.ginConv.nn.mlp.2.linear.bias": torch.randn(W, generator=g) * 0.3}


def layer1_unsaturated_share(x64, ei, sd64):
    """From the oracle's arithmetic alone: the share of layer 1's pre-activations with |v| < 4."""
    keep = ei[0] != ei[1]
    z = (1.0 + sd64[f"{PREFIX}.ginConv.eps"]) * x64 + torch.zeros_like(x64).index_add_(0, ei[1][keep], x64[ei[0][keep]])
    v = orc.linear(z, sd64, f"{PREFIX}.ginConv.nn.mlp.0.linear")
    return float((v.abs() < 4).double().mean())


def bn_record_on_cpu(a, seed):
    """A BatchNorm record [4][64] of `a` (mean hi, mean lo, gamma / sqrt(var + eps), beta) with random gamma / beta, as
    tests/test_training_width64.py builds it, and the fp64 BatchNorm it describes applied to `a`."""
    from tests.test_training_width64 import _bn, _bn_stat
    bn = _bn(W, seed)
    stat = _bn_stat(a, bn)
    s = stat.double().cpu().view(4, W)
    x64 = ((a.double().cpu() - s[0]) - s[1]) * s[2] + s[3]
    return stat, x64, bn


SIZES = [1, 16, 17, 37, 1254, 4099, 66003]


@pytest.mark.parametrize("n", SIZES)
def test_op_against_fp64(dev, n):
    """Gate: 1e-6 of the largest output, for every (BatchNorm record or none) x (magnitude 1e-3, 1, 1e3) x (LeakyReLU or none);
    one oracle evaluation serves both activations.  Three bf16 pieces per operand hold it to 2^-24; the sums are fp32."""
    from tests.test_training_width64 import _bn_ref
    from tilingnn_amd import ops
    ei = collision_edges(n, seed=n)
    rowptr, src, _, _ = ops.build_csr(ei.to(dev), n, True)
    graph = types.SimpleNamespace(n_nodes=n, col_rowptr=rowptr, col_src=src)
    gen = torch.Generator().manual_seed(n + 2)
    base = torch.randn(n, W, generator=gen)
    for with_stat in (False, True):
        for scale in (1e-3, 1.0, 1e3):
            # (behind a folded BatchNorm record the MLP sees normalised rows whatever the magnitude of `a`)
            sd = gin_weights(ei, n, seed=n + 1, in_scale=1.0 if with_stat else scale)
            sd64 = orc.cast_sd(sd, torch.float64)
            params = [sd[f"{PREFIX}.ginConv.eps"]] + [sd[f"{PREFIX}.ginConv.nn.mlp.{i}.linear.{k}"] for i in range(3) for k in ("weight", "bias")]
            params = [p.to(dev) for p in params]
            a = (base * scale + (0.3 * scale if with_stat else 0.0)).to(dev)
            stat = None
            x64 = a.double().cpu()
            if with_stat:
                stat, x64, bn = bn_record_on_cpu(a, seed=4)
                if n > 1:                                     # the record describes the BatchNorm of `a` (one row: variance 0)
                    assert orc.rel_max_err(x64, _bn_ref(a.double(), bn, False).cpu()) < 1e-5
            with torch.no_grad():
                want_lin = orc.gin_conv(x64, ei, sd64, PREFIX)
            if scale == 1.0 or not with_stat:
                share = layer1_unsaturated_share(x64, ei, sd64)
                assert share >= 0.5, f"layer 1 saturated: only {share:.2f} of its pre-activations within (-4, 4)"
            for leaky in (False, True):
                want = orc.leaky_relu(want_lin) if leaky else want_lin
                act = ops.ACT_LEAKY_RELU if leaky else ops.ACT_NONE
                part = ops.new_partials(W, dev)
                out, npart = ops.gin(a, graph, *params, act=act, in_stat=stat, partials=part, kernel="mfma")
                out_gen, _ = ops.gin(a, graph, *params, act=act, in_stat=stat, partials=ops.new_partials(W, dev))
                err, err_gen = orc.rel_max_err(out.cpu(), want), orc.rel_max_err(out_gen.cpu(), want)
                worst = int((out.cpu().double() - want).abs().max(1).values.argmax())
                print(f"gin64 mfma n {n} stat {int(with_stat)} scale {scale:g} leaky {int(leaky)}: rel_max_err {err:.3e}, "
                      f"generic kernel {err_gen:.3e}, ratio {err / max(err_gen, 1e-30):.2f} (worst row {worst}, in-degree "
                      f"{int(rowptr[worst + 1] - rowptr[worst])})")
                assert out.shape == (n, W) and bool(torch.isfinite(out).all())
                assert err < GATE
                # BatchNorm partial rows: [blocks][sum 64 | sum of squares 64] in fp64 (tolerances of tests/test_nnconv64_eg.py)
                assert 1 <= npart <= 512
                p = part[:npart * 2 * W].view(npart, 2 * W).sum(0).cpu()
                assert torch.allclose(p[:W], want.sum(0), rtol=1e-6, atol=1e-6 * float(want.abs().max()) * n)
                assert torch.allclose(p[W:], (want * want).sum(0), rtol=1e-5, atol=1e-6 * float(want.abs().max()) ** 2 * n)
                # the same bits on a second call, output and partial rows
                part2 = ops.new_partials(W, dev)
                out2, npart2 = ops.gin(a, graph, *params, act=act, in_stat=stat, partials=part2, kernel="mfma")
                assert npart2 == npart and torch.equal(out, out2) and torch.equal(part[:npart * 2 * W], part2[:npart * 2 * W])


# ---------------------------------------------------------------------------------------------- refusals
def test_refusals_and_the_empty_layout(dev):
    from tilingnn_amd import ops
    from tilingnn_amd._lib import lib, ptr
    n = 37
    ei = collision_edges(n, seed=3)
    rowptr, src, _, _ = ops.build_csr(ei.to(dev), n, True)
    graph = types.SimpleNamespace(n_nodes=n, col_rowptr=rowptr, col_src=src)
    gen = torch.Generator().manual_seed(1)
    eps = torch.tensor([0.0], device=dev)
    # width 32 is not this kernel's
    w32 = [torch.randn(32, 32, generator=gen), torch.randn(32, generator=gen), torch.randn(64, 32, generator=gen),
           torch.randn(64, generator=gen), torch.randn(32, 64, generator=gen), torch.randn(32, generator=gen)]
    with pytest.raises(ValueError, match="64"):
        ops.gin(torch.randn(n, 32, generator=gen).to(dev), graph, eps, *[p.to(dev) for p in w32], kernel="mfma")
    with pytest.raises(ValueError):
        ops.gin(torch.randn(n, 32, generator=gen).to(dev), graph, eps, *[p.to(dev) for p in w32], kernel="no such kernel")
    # the library's own entry point
    w64 = [torch.randn(32, W, generator=gen), torch.randn(32, generator=gen), torch.randn(64, 32, generator=gen),
           torch.randn(64, generator=gen), torch.randn(W, 64, generator=gen), torch.randn(W, generator=gen)]
    w64 = [p.to(dev) for p in w64]
    a = torch.randn(n, W, generator=gen).to(dev)
    out = torch.empty(n, W, device=dev)
    z = torch.empty(n * W + 4, device=dev)
    npart = C.c_int32(7)

    def call(a_, lda, z_, rows):
        return lib.tgnn_gin64_fwd(ptr(a_), lda, None, ptr(rowptr), ptr(src), ptr(eps), *[ptr(p) for p in w64], rows, ops.ACT_NONE,
                                  ptr(out), ptr(z_), None, C.byref(npart), None)

    assert call(a, W, z[1:], n) == -4 and b"aligned" in lib.tgnn_last_error()          # z_scratch 4 bytes off
    assert call(torch.randn(n, 66, generator=gen).to(dev), 66, z, n) == -4 and b"66" in lib.tgnn_last_error()
    assert call(a, 32, z, n) == -1 and b"lda" in lib.tgnn_last_error()                 # rows shorter than the width
    assert npart.value == 7                                                           # (nothing ran)
    assert call(a, W, z, 0) == 0 and npart.value == 0                                 # no rows: OK, 0 partial rows
    assert call(a, W, z, n) == 0 and npart.value == 1
    torch.cuda.synchronize()
    want, _ = ops.gin(a, graph, eps, *w64, kernel="mfma")
    assert torch.equal(out, want)


# ---------------------------------------------------------------------------------------------- the forward
def _net(fe, depth, seed, dev):
    from tilingnn_amd.graph_networks.networks.TilinGNN import TilinGNN
    from tilingnn_amd.weights import make_state_dict
    net = TilinGNN(adj_edge_features_dim=fe, network_depth=depth, network_width=W, node_features_dim=3)
    sd = make_state_dict(fe, depth, W, 1, 3, seed=seed)
    net.load_state_dict(sd)
    net = net.to(dev).train()
    net.cache_graph = False
    return net, sd


def _both_forwards(net, x, adj, attr, col):
    from tilingnn_amd import train
    with torch.no_grad():
        p_inf = net(x=x, adj_e_index=adj, adj_e_features=attr, col_e_idx=col)[0].clone()
    p_train, sv = train.forward_train(net, x, adj, attr, col)
    return p_inf, p_train.clone(), sv


@pytest.mark.parametrize("nnconv64_eg", [0, 1])
def test_forward_routing(dev, nnconv64_eg):
    """Width 64, depth 3, the labyrinth layout.  Switch off: the bits of a run before the switch was ever touched.  Switch on:
    every layer's kept CollConv output IS the new op on the kept operands, the kept aggregate IS the gather kernel's; inference
    and the training forward give the same probabilities bit for bit.  Once more with the edge-group NNConv's switch on as well."""
    from tilingnn_amd import ops, train
    net, _ = _net(15, 3, 4, dev)
    x, adj, attr, col, _ = graph_tensors(load_labyrinth_graph(), torch.float32, dev)
    n = int(x.shape[0])
    part = ops.new_partials(W, dev)
    assert ops.set_gin64_mfma(-1) == 0                       # the default
    prev_eg = ops.set_nnconv64_eg(nnconv64_eg)
    try:
        p_inf_0, p_0, sv_0 = _both_forwards(net, x, adj, attr, col)            # before the switch is touched
        prev = ops.set_gin64_mfma(1)
        try:
            assert prev == 0 and ops.set_gin64_mfma(-1) == 1 and ops.set_gin64_mfma(7) == 1
            p_inf_on, p_on, sv_on = _both_forwards(net, x, adj, attr, col)
        finally:
            ops.set_gin64_mfma(prev)
        assert ops.set_gin64_mfma(-1) == 0
        p_inf_off, p_off, sv_off = _both_forwards(net, x, adj, attr, col)      # switched off again
    finally:
        ops.set_nnconv64_eg(prev_eg)
    # off: nothing changed
    assert torch.equal(p_inf_off, p_inf_0) and torch.equal(p_off, p_0) and torch.equal(p_inf_off, p_off)
    for i in range(3):
        assert torch.equal(sv_off.a2[i], sv_0.a2[i]) and torch.equal(sv_off.u[i], sv_0.u[i]), i
    # on: the kernel ran on the right operands
    g = sv_on.tg.g
    for i in range(3):
        gin = net.brch_2_coll_conv_layers[i].ginConv
        h_in, h_stat = (sv_on.skip[0], None) if i == 0 else (sv_on.a2[i - 1], sv_on.stat2[i - 1])
        mlp = [p.detach() for p in gin._mlp_params()]
        want, _ = ops.gin(h_in, g, gin.eps, *mlp, act=ops.ACT_LEAKY_RELU, in_stat=h_stat, partials=part, kernel="mfma")
        assert torch.equal(sv_on.a2[i], want), i
        assert torch.equal(sv_on.u[i], train.gin_aggregate(h_in, g.col_rowptr, g.col_src, gin.eps, n, in_stat=h_stat)), i
    assert not torch.equal(sv_on.a2[0], sv_off.a2[0])        # (it IS the other kernel)
    assert torch.equal(sv_on.skip[0], sv_off.skip[0])        # (the init MLP is untouched)
    assert torch.equal(p_inf_on, p_on)
    assert float((p_on - p_off).abs().max()) < 2e-3


def test_eval_mode(dev):
    """A forward on running statistics takes the kernel too: within the eval gate of the fp64 oracle (tests/eval_cases.py), within
    2e-3 of the generic kernel's, statistics untouched."""
    from tilingnn_amd import ops
    net, _ = _net(15, 3, 4, dev)
    x, adj, attr, col, _ = graph_tensors(load_labyrinth_graph(), torch.float32, dev)
    with torch.no_grad():
        net(x=x, adj_e_index=adj, adj_e_features=attr, col_e_idx=col)         # one train-mode forward: statistics worth using
    net.eval()
    before = {k: v.detach().clone() for k, v in net.state_dict().items()}
    with torch.no_grad():
        p_off = net(x=x, adj_e_index=adj, adj_e_features=attr, col_e_idx=col)[0].clone()
    prev = ops.set_gin64_mfma(1)
    try:
        with torch.no_grad():
            p_on = net(x=x, adj_e_index=adj, adj_e_features=attr, col_e_idx=col)[0].clone()
    finally:
        ops.set_gin64_mfma(prev)
    from tests import eval_cases
    want, gate = eval_cases.probs_gate(before, (x, adj, attr, col))   # the fp64 oracle's eval forward of the same buffers
    err = float((p_on.cpu().double() - want).abs().max())
    print(f"eval forward with gin64_mfma: max |p - p_fp64| {err:.2e}, gate {gate:.2e}")
    assert err <= gate and float((p_on - p_off).abs().max()) < 2e-3
    assert not torch.equal(p_on, p_off)                      # (the switch reached this forward)
    after = net.state_dict()
    assert all(torch.equal(before[k], after[k]) for k in before)


def test_kept_buffers_meet_the_oracle_gate_with_the_switch_on(dev, switch_on):
    """Every buffer tgnn_forward_train keeps and the probabilities, against the fp64 oracle's intermediates with the gate of
    tests/test_training_width64.py::test_forward_train_keeps_what_the_backward_reads, run as it stands."""
    from tests.test_training_width64 import test_forward_train_keeps_what_the_backward_reads as keeps_gate
    keeps_gate()


@pytest.mark.parametrize("seed", [1, 2, 3])
def test_training_step_with_the_switch_on(dev, switch_on, seed):
    """One width-64 step on the labyrinth layout, depth 3: the loss within 1e-4 of the fp64 oracle's, every parameter gradient
    within max(0.06, 2 x the float32 oracle's worst error) -- the gates of
    tests/test_nnconv64_eg.py::test_training_step_with_the_switch_on."""
    from tests.test_training_width64 import _f32_oracle_err, _rel
    from tilingnn_amd.solver.ml_solver.losses import Losses
    x, adj, attr, col, _ = graph_tensors(load_labyrinth_graph(), torch.float32, dev)
    torch.set_num_threads(8)
    net, sd = _net(15, 3, seed, dev)
    net.autograd = True
    probs, _ = net(x, adj, attr, col)
    loss, _, _ = Losses.calculate_unsupervised_loss(probs, x, col, adj, attr)
    loss.backward()
    _, ref_loss, _, ref_grads = orc.training_step_grads(orc.cast_sd(sd, torch.float64), x.double().cpu(), adj.cpu(), attr.double().cpu(),
                                                        col.cpu())
    err32 = _f32_oracle_err(sd, x.cpu(), adj.cpu(), attr.cpu(), col.cpu(), ref_grads)
    errs = {k: _rel(p.grad, ref_grads[k]) for k, p in net.named_parameters()}
    print(f"gin64 mfma on, seed {seed}: loss {float(loss.detach()):.8f} oracle {float(ref_loss):.8f}; worst parameter ours "
          f"{max(errs.values()):.2e}, float32 oracle's worst {max(err32.values()):.2e}")
    assert abs(float(loss.detach()) - float(ref_loss)) < 1e-4 * float(ref_loss)
    assert set(errs) == set(err32)
    assert max(errs.values()) < max(0.06, 2.0 * max(err32.values())), max(errs.items(), key=lambda kv: kv[1])


def test_ragged_general_schedule_forward(dev, switch_on):
    """4 099 nodes (no multiple of any tile), depth 2: the probabilities against the fp64 oracle within the 4e-4 the width-32 GIN
    tests use (tests/test_gin_fused.py)."""
    from tests.test_mid_layout import _layout
    n = 4099
    (x, adj, attr, col), inputs64 = _layout(n, dev, seed=6)
    net, sd = _net(int(attr.shape[1]), 2, 2, dev)
    with torch.no_grad():
        probs = net(x=x, adj_e_index=adj, adj_e_features=attr, col_e_idx=col)[0]
        want = orc.tilingnn_forward(orc.cast_sd(sd, torch.float64), *inputs64)[0]
    gap = float((probs.cpu().double() - want).abs().max())
    print(f"gin64 mfma on, n {n}, depth 2: max |p - p_fp64| {gap:.2e}")
    assert probs.shape == (n, 1) and gap < 4e-4
