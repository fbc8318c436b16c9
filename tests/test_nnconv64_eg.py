"""NNConv at network_width 64, fp32, over edge groups on the matrix cores (csrc/nnconv64_eg.hip: nnconv64_eg_kernel) and its
opt-in route through tgnn_forward / tgnn_forward_train (tgnn_set_nnconv64_eg, default off).  Reference semantics:
GraphConv.forward, graph_networks/layers/edge_conv.py:24-27 of the reference (PyG NNConv, aggr="mean", root weight, bias).

* the op against the pinned fp64 oracle (oracle.nnconv_mean_dedup, edge MLP 4 -> 32 -> 64 -> 4096) at 37 ... 20 000 nodes,
  1 ... 18 edge types (18 = the kernel's limit), rows with more than 16 in-edges of one type and rows with none, magnitudes
  1e-3 ... 1e3, with and without LeakyReLU, BatchNorm partial sums included; the generic kernel's error printed beside it;
* halo rows behind the destinations; the refusals (edge types, in-degree) of the op and what the forward does with them;
* the forward's routing (the kernel ran on the right operands; switch off = the bits of before), one training step against the
  fp64 oracle with the switch on.
"""
import pytest
import torch

from oracle import tilingnn_oracle as orc
from tests.golden_util import graph_tensors, load_labyrinth_graph

pytestmark = pytest.mark.gpu
W = 64
GATE = 2e-6          # of the output's max-norm: the bound the project's fp32-accurate NNConv kernels are held to


@pytest.fixture(scope="module")
def dev():
    if not torch.cuda.is_available():
        pytest.skip("needs a GPU")
    return torch.device("cuda:0")


@pytest.fixture()
def switch_on():
    from tilingnn_amd import ops
    prev = ops.set_nnconv64_eg(1)
    try:
        yield
    finally:
        ops.set_nnconv64_eg(prev)


def _limit():
    from tilingnn_amd._lib import lib
    return int(lib.tgnn_nnconv64_eg_max_types())


def random_layout(n, ea, n_types, seed, max_type_run=0):
    """adjacency [2, ea] (int64), attribute rows with n_types distinct values; max_type_run > 0: node 3 receives that many
    in-edges of ONE type (more than a group holds); node 5 none at all."""
    g = torch.Generator().manual_seed(seed)
    src = torch.randint(0, n, (ea,), generator=g)
    dst = torch.randint(0, n, (ea,), generator=g)
    typ = torch.randint(0, n_types, (ea,), generator=g)
    if n > 8:
        dst[dst == 5] = 6
        if max_type_run:
            dst[:max_type_run] = 3
            typ[:max_type_run] = typ[0]
    table = torch.rand(n_types, 4, generator=g)
    return torch.stack([src, dst]), table[typ].contiguous()


def fp64_nnconv(h, adj, edge_type, wtab, root, bias, n, leaky):
    """oracle/tilingnn_oracle.py: nnconv_mean in fp64 on the device, on a given table (edge_conv.py:25; LeakyReLU behind it)."""
    src, dst = adj[0], adj[1]
    msg = torch.einsum("ek,eko->eo", h.double()[src], wtab.double()[edge_type])
    agg = torch.zeros(n, W, dtype=torch.float64, device=h.device).index_add_(0, dst, msg)
    deg = torch.zeros(n, dtype=torch.float64, device=h.device).index_add_(0, dst, torch.ones_like(dst, dtype=torch.float64))
    out = agg / deg.clamp(min=1).unsqueeze(1) + h.double()[:n] @ root.double() + bias.double()
    return torch.where(out >= 0, out, out * 0.01) if leaky else out


CASES = [(37, 200, 3, 0, 1.0), (1254, 9000, 13, 0, 1.0), (1000, 12000, 1, 40, 1.0), (4097, 30000, "limit", 0, 1.0),
         (20000, 200000, 13, 20, 1.0), (5000, 40000, 13, 0, 1e-3), (5000, 40000, 13, 0, 8.0), (5000, 40000, 13, 0, 1e3)]


@pytest.mark.parametrize("n,ea,n_types,run,scale", CASES)
def test_op_against_fp64(dev, n, ea, n_types, run, scale):
    """Gate: 2e-6 of the largest output, with and without LeakyReLU (one oracle evaluation serves both).  Three fp16-pair splits
    of 2^-22 each (rows, weights, messages) and fp32 sums.  The generic kernel's error on the same inputs is printed beside the
    new kernel's.  Magnitudes 1e-3, 1 and 1e3 take the scaled branch of the row split, 8 the unscaled one."""
    from tilingnn_amd import ops
    if n_types == "limit":
        n_types = _limit()
    adj, attr = random_layout(n, ea, n_types, seed=n + n_types, max_type_run=run)
    adj, attr = adj.to(dev), attr.to(dev)
    g = ops.prepare_graph(n, adj, attr, torch.zeros(2, 0, dtype=torch.int64, device=dev), groups=True)
    assert g.n_types == n_types
    gen = torch.Generator().manual_seed(1)
    h = (torch.randn(n, W, generator=gen) * torch.randn(n, W, generator=gen) * scale).to(dev)
    prefix = "g"
    sd = {f"{prefix}.mlp.mlp.0.linear.weight": torch.randn(32, 4, generator=gen) * 0.5, f"{prefix}.mlp.mlp.0.linear.bias": torch.randn(32, generator=gen) * 0.1,
          f"{prefix}.mlp.mlp.1.linear.weight": torch.randn(64, 32, generator=gen) * 0.2, f"{prefix}.mlp.mlp.1.linear.bias": torch.randn(64, generator=gen) * 0.1,
          f"{prefix}.mlp.mlp.2.linear.weight": torch.randn(W * W, 64, generator=gen) * 0.2, f"{prefix}.mlp.mlp.2.linear.bias": torch.randn(W * W, generator=gen) * 0.1,
          f"{prefix}.nnConv.root": torch.randn(W, W, generator=gen) * 0.3, f"{prefix}.nnConv.bias": torch.randn(W, generator=gen) * scale}
    mlp = [sd[f"{prefix}.mlp.mlp.{i}.linear.{k}"].to(dev) for i in range(3) for k in ("weight", "bias")]
    wtab = ops.edge_weight_table(attr, g, *mlp, W)
    root, bias = sd[f"{prefix}.nnConv.root"].to(dev), sd[f"{prefix}.nnConv.bias"].to(dev)
    with torch.no_grad():
        want_lin = orc.nnconv_mean_dedup(h.double().cpu(), adj.cpu(), attr.double().cpu(), orc.cast_sd(sd, torch.float64), prefix)
    assert g.max_in_degree >= (run if n > 8 else 1)
    for leaky in (False, True):
        want = orc.leaky_relu(want_lin) if leaky else want_lin
        act = ops.ACT_LEAKY_RELU if leaky else ops.ACT_NONE
        # (this file's own restatement, on the device's table: the two expectations agree to the table's fp32 rounding)
        assert orc.rel_max_err(fp64_nnconv(h, adj, g.edge_type[:ea].long(), wtab, root, bias, n, leaky).cpu(), want) < 1e-6
        part = ops.new_partials(W, dev)
        out, npart = ops.nnconv_mean(h, g, wtab, root, bias, act, part, kernel="eg")
        out_gen, _ = ops.nnconv_mean(h, g, wtab, root, bias, act, ops.new_partials(W, dev))         # width 64, kernel=None: generic
        err, err_gen = orc.rel_max_err(out.cpu(), want), orc.rel_max_err(out_gen.cpu(), want)
        print(f"nnconv64_eg n {n} ea {ea} T {n_types} run {run} scale {scale:g} leaky {int(leaky)}: rel_max_err {err:.3e}, "
              f"generic kernel {err_gen:.3e}, ratio {err / max(err_gen, 1e-30):.2f}")
        assert out.shape == (n, W) and bool(torch.isfinite(out).all())
        assert err < GATE
        # BatchNorm partial rows: [blocks][sum 64 | sum of squares 64] in fp64 (tolerances of tests/test_nnconv_eg.py)
        p = part[:npart * 2 * W].view(npart, 2 * W).sum(0).cpu()
        assert 1 <= npart <= 512
        assert torch.allclose(p[:W], want.sum(0), rtol=1e-6, atol=1e-6 * float(want.abs().max()) * n)
        assert torch.allclose(p[W:], (want * want).sum(0), rtol=1e-5, atol=1e-6 * float(want.abs().max()) ** 2 * n)


def test_halo_rows_behind_the_destinations(dev):
    """A shard's layout: sources index rows behind the n destination rows (n_src_nodes > n_nodes); a random table."""
    from tilingnn_amd import ops
    n, n_src, ea = 3000, 3700, 30000
    gen = torch.Generator().manual_seed(4)
    adj = torch.stack([torch.randint(0, n_src, (ea,), generator=gen), torch.randint(0, n, (ea,), generator=gen)]).to(dev)
    table = torch.rand(7, 3, generator=gen)
    attr = table[torch.randint(0, 7, (ea,), generator=gen)].contiguous().to(dev)
    g = ops.prepare_graph(n, adj, attr, torch.zeros(2, 0, dtype=torch.int64, device=dev), n_src_nodes=n_src)
    assert g.n_types == 7
    h = torch.randn(n_src, W, generator=gen).to(dev)
    wtab = torch.rand(g.n_types, W, W, generator=gen).to(dev)
    root = (torch.randn(W, W, generator=gen) * 0.3).to(dev)
    bias = torch.randn(W, generator=gen).to(dev)
    want = fp64_nnconv(h, adj, g.edge_type[:ea].long(), wtab, root, bias, n, False)
    out, _ = ops.nnconv_mean(h, g, wtab, root, bias, ops.ACT_NONE, ops.new_partials(W, dev), kernel="eg")
    err = orc.rel_max_err(out.cpu(), want.cpu())
    print(f"nnconv64_eg halo rows: rel_max_err {err:.3e}")
    assert bool(torch.isfinite(out).all()) and err < GATE


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


def test_more_edge_types_than_the_kernel_takes(dev):
    """T = limit + 1: the op refuses (ValueError naming the limit), kernel=None gives the generic kernel's bits."""
    from tilingnn_amd import ops
    from tilingnn_amd._lib import check, lib, ptr
    import ctypes as C
    n, ea, T = 700, 6000, _limit() + 1
    adj, attr = random_layout(n, ea, T, seed=11)
    adj, attr = adj.to(dev), attr.to(dev)
    g = ops.prepare_graph(n, adj, attr, torch.zeros(2, 0, dtype=torch.int64, device=dev), groups=True)
    assert g.n_types == T
    gen = torch.Generator().manual_seed(2)
    h = torch.randn(n, W, generator=gen).to(dev)
    wtab = torch.rand(T, W, W, generator=gen).to(dev)
    root, bias = (torch.randn(W, W, generator=gen) * 0.3).to(dev), torch.randn(W, generator=gen).to(dev)
    with pytest.raises(ValueError, match=str(_limit())):
        ops.nnconv_mean(h, g, wtab, root, bias, ops.ACT_NONE, ops.new_partials(W, dev), kernel="eg")
    out, _ = ops.nnconv_mean(h, g, wtab, root, bias, ops.ACT_NONE, ops.new_partials(W, dev))
    out_gen = torch.empty_like(out)
    npart = C.c_int32(0)
    check(lib.tgnn_nnconv_mean_fwd(ptr(h), W, ptr(g.adj_rowptr), ptr(g.adj_src), ptr(g.adj_type), ptr(wtab), T, ptr(root), ptr(bias), n, W,
                                   ops.ACT_NONE, ptr(out_gen), None, C.byref(npart), None))
    assert torch.equal(out, out_gen)
    # ... and the library's own entry point refuses with TGNN_ERR_UNSUPPORTED and a message
    grp = ops.graph_groups(g)
    assert grp is not None
    wimg = torch.empty(lib.tgnn_nnconv64_eg_image_floats(T), dtype=torch.float32, device=dev)
    bounds = torch.empty(2, dtype=torch.int32, device=dev)
    rc = lib.tgnn_nnconv64_mean_eg_fwd(ptr(h), W, n, ptr(grp.tile_grp_ptr), ptr(grp.grp), ptr(wtab), T, ptr(root), ptr(bias), n, ops.ACT_NONE,
                                       ptr(out_gen), ptr(wimg), ptr(bounds), None, C.byref(npart), None)
    assert rc == -4 and b"edge types" in lib.tgnn_last_error()


def test_in_degree_beyond_the_limit(dev):
    """A hub with limit + 1 in-edges at 5 000 nodes: refused by the op, left to the generic kernel by the forward."""
    from tilingnn_amd import ops
    from tilingnn_amd.synth import make_super_graph
    n = 5000
    sg = make_super_graph(n, 10 * n, 12 * n, tile_count=2, n_edge_types=13, seed=4)
    x, adj, attr, col, _ = sg.to_torch(dev)
    adj = adj.clone()
    adj[1, :ops.NNCONV64_EG_MAX_IN_DEGREE + 1] = 123
    g = ops.prepare_graph(n, adj, attr, col)
    assert g.max_in_degree >= ops.NNCONV64_EG_MAX_IN_DEGREE + 1
    gen = torch.Generator().manual_seed(5)
    h = torch.randn(n, W, generator=gen).to(dev)
    wtab = torch.rand(g.n_types, W, W, generator=gen).to(dev)
    root, bias = (torch.randn(W, W, generator=gen) * 0.3).to(dev), torch.randn(W, generator=gen).to(dev)
    with pytest.raises(ValueError, match=str(ops.NNCONV64_EG_MAX_IN_DEGREE)):
        ops.nnconv_mean(h, g, wtab, root, bias, ops.ACT_NONE, ops.new_partials(W, dev), kernel="eg")
    net, _ = _net(int(attr.shape[1]), 2, 1, dev)
    off = _both_forwards(net, x, adj, attr, col)
    prev = ops.set_nnconv64_eg(1)
    try:
        on = _both_forwards(net, x, adj, attr, col)
    finally:
        ops.set_nnconv64_eg(prev)
    assert torch.equal(on[0], off[0]) and torch.equal(on[1], off[1])
    assert all(torch.equal(a, b) for a, b in zip(on[2].a1, off[2].a1))


def test_layout_with_more_types_than_the_limit_keeps_its_bits(dev):
    from tilingnn_amd import ops
    from tilingnn_amd.synth import make_super_graph
    sg = make_super_graph(600, 6000, 7500, tile_count=2, n_edge_types=25, seed=9)
    x, adj, attr, col, _ = sg.to_torch(dev)
    net, _ = _net(2 + 25, 2, 3, dev)
    off = _both_forwards(net, x, adj, attr, col)
    assert off[2].tg.g.n_types > _limit()
    prev = ops.set_nnconv64_eg(1)
    try:
        on = _both_forwards(net, x, adj, attr, col)
    finally:
        ops.set_nnconv64_eg(prev)
    assert torch.equal(on[0], off[0]) and torch.equal(on[1], off[1])
    assert all(torch.equal(a, b) for a, b in zip(on[2].a1, off[2].a1))


def test_forward_routing(dev):
    """Width 64, depth 3, the labyrinth layout.  Switch on: every layer's kept NNConv output IS the new op on the kept operands
    (the forward ran the kernel on the right rows, table, root and bias); switch off: it is the generic op (nothing changed).
    Inference and the training forward give the same probabilities bit for bit in either setting."""
    from tilingnn_amd import ops, train
    net, _ = _net(15, 3, 4, dev)
    x, adj, attr, col, _ = graph_tensors(load_labyrinth_graph(), torch.float32, dev)
    params = dict(net.named_parameters())
    part = ops.new_partials(W, dev)
    assert ops.set_nnconv64_eg(-1) == 0                      # the default
    p_inf_off, p_off, sv_off = _both_forwards(net, x, adj, attr, col)
    g = sv_off.tg.g
    assert 1 <= g.n_types <= _limit() and 1 <= g.max_in_degree <= ops.NNCONV64_EG_MAX_IN_DEGREE
    prev = ops.set_nnconv64_eg(1)
    try:
        assert prev == 0 and ops.set_nnconv64_eg(-1) == 1
        p_inf_on, p_on, sv_on = _both_forwards(net, x, adj, attr, col)
        for i in range(3):
            root, bias = params[f"brch_1_graph_conv_layers.{i}.nnConv.root"], params[f"brch_1_graph_conv_layers.{i}.nnConv.bias"]
            eg, _ = ops.nnconv_mean(sv_on.skip[i], sv_on.tg.g, sv_on.wtab[i], root.detach(), bias.detach(), ops.ACT_LEAKY_RELU, part, kernel="eg")
            assert torch.equal(sv_on.a1[i], eg), i
            gen, _ = ops.nnconv_mean(sv_off.skip[i], g, sv_off.wtab[i], root.detach(), bias.detach(), ops.ACT_LEAKY_RELU, part)
            assert torch.equal(sv_off.a1[i], gen), i
        assert not torch.equal(sv_on.a1[0], sv_off.a1[0])    # two kernels, two roundings
        assert torch.equal(sv_on.skip[0], sv_off.skip[0])    # (the init MLP is untouched)
        assert float((p_on - p_off).abs().max()) < 2e-3
    finally:
        ops.set_nnconv64_eg(prev)
    assert torch.equal(p_inf_off, p_off)
    assert torch.equal(p_inf_on, p_on)


def test_kept_buffers_meet_the_oracle_gate_with_the_switch_on(dev, switch_on):
    """Every buffer tgnn_forward_train keeps and the probabilities, against the fp64 oracle's intermediates with the gate of
    tests/test_training_width64.py::test_forward_train_keeps_what_the_backward_reads (tol = 2e-3), run as it stands."""
    from tests.test_training_width64 import test_forward_train_keeps_what_the_backward_reads as keeps_gate
    keeps_gate()


@pytest.mark.parametrize("seed", [1, 2, 3])
def test_training_step_with_the_switch_on(dev, switch_on, seed):
    """One width-64 step on the labyrinth layout, depth 3: the loss within 1e-4 of the fp64 oracle's, every parameter gradient
    within max(0.06, 2 x the float32 oracle's worst error) -- the "none may be off by more" gate of
    tests/test_training_width64.py::test_training_step_width64_against_the_oracle."""
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
    print(f"switch on, seed {seed}: loss {float(loss.detach()):.8f} oracle {float(ref_loss):.8f}; worst parameter ours "
          f"{max(errs.values()):.2e}, float32 oracle's worst {max(err32.values()):.2e}")
    assert abs(float(loss.detach()) - float(ref_loss)) < 1e-4 * float(ref_loss)
    assert set(errs) == set(err32)
    assert max(errs.values()) < max(0.06, 2.0 * max(err32.values())), max(errs.items(), key=lambda kv: kv[1])
