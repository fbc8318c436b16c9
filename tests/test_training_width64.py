"""Training at network_width 64 (BASELINE config 3's width) on the GPU: the width-64 adjoint kernels against float64
restatements, the buffers the training forward keeps against the oracle's intermediates, the whole step against the fp64
oracle, the library backward against the spelled-out schedule, and Trainer.train end to end."""
import numpy as np
import pytest
import torch

from oracle import tilingnn_oracle as orc
from tests.golden_util import graph_tensors, load_labyrinth_graph

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
W = 64


def _rel(got, want):
    got, want = got.detach().double().cpu(), want.detach().double().cpu()
    return float((got - want).abs().max() / want.abs().max().clamp(min=1e-30))


def _rng(seed):
    g = torch.Generator().manual_seed(seed)
    return lambda *shape: torch.randn(*shape, generator=g)


def _net(fe, depth, seed, width=W, fx=3):
    from tilingnn_amd.graph_networks.networks.TilinGNN import TilinGNN
    from tilingnn_amd.weights import make_state_dict
    net = TilinGNN(adj_edge_features_dim=fe, network_depth=depth, network_width=width, node_features_dim=fx)
    sd = make_state_dict(fe, depth, width, 1, fx, seed=seed)
    net.load_state_dict(sd)
    return net.to(DEV).train(), sd


def _bn(f, seed):
    bn = torch.nn.BatchNorm1d(f)
    r = _rng(seed)
    with torch.no_grad():
        bn.weight.copy_(1 + 0.3 * r(f))
        bn.bias.copy_(0.2 * r(f))
    return bn.to(DEV)


def _bn_stat(a, bn):
    from tilingnn_amd import ops
    sums = torch.stack([a.double().sum(0), (a.double() ** 2).sum(0)]).contiguous()
    return ops.bn_stat_from_sums(sums, int(a.shape[0]), bn, update_running=False)


def _bn_ref(z, bn, leaky):
    a = torch.where(z > 0, z, 0.01 * z) if leaky else z
    mean, var = a.mean(0), a.var(0, unbiased=False)
    return (a - mean) / torch.sqrt(var + bn.eps) * bn.weight.detach().double() + bn.bias.detach().double()


# ---------------------------------------------------------------------------------------------- single kernels
def _edges_with_a_hub(n, e, hub, hub_in, seed):
    """Random directed edges (destination = row 1) plus `hub_in` edges into row `hub`; rows n - 7 .. n - 1 get no in-edges."""
    rng = np.random.default_rng(seed)
    src = rng.integers(0, n, e)
    dst = rng.integers(0, n - 7, e)
    src = np.concatenate([src, rng.integers(0, n, hub_in)])
    dst = np.concatenate([dst, np.full(hub_in, hub)])
    return torch.tensor(np.stack([src, dst]), dtype=torch.int64)


@pytest.mark.parametrize("T", [0, 1, 13, 63])
def test_type_sum_width64(T):
    """Per-type sums over a CSR at width 64: zero-in-degree rows, a hub row with 700 in-edges, many same-type edges on a row,
    a node count that is not a multiple of the kernel's rows per block, a row stride wider than 64."""
    from tilingnn_amd import ops, train
    n = 4099
    ei = _edges_with_a_hub(n, 30000, 17, 700, seed=T).to(DEV)
    rowptr, src, eid, _ = ops.build_csr(ei, n, False)
    e = int(ei.shape[1])
    rng = np.random.default_rng(100 + T)
    edge_type = torch.tensor(rng.integers(0, max(T, 1), e) if T else np.zeros(e, dtype=np.int64), device=DEV)
    if T:
        edge_type[ei[1] == 17] = int(rng.integers(0, T))     # the hub: hundreds of edges of one type
    typ = edge_type[eid[:e].long()].int().contiguous() if e else torch.zeros(1, dtype=torch.int32, device=DEV)
    r = _rng(T)
    wide = r(n, W + 16).to(DEV)
    rows = wide[:, :W]                                       # ld_rows = 80
    own = r(n, W).to(DEV)
    scale = (r(n).abs() + 0.5).to(DEV)
    got = train.type_sum(rows, own, scale, rowptr, src, typ, n, T).view(n, T + 1, W)
    want = torch.zeros(n, T + 1, W, dtype=torch.float64, device=DEV)
    if T:
        want.view(n * (T + 1), W).index_add_(0, ei[1] * (T + 1) + edge_type, rows.double()[ei[0]])
    want[:, T] = own.double() * scale.double()[:, None]
    assert _rel(got, want) < 1e-6
    if T:
        assert float(got[n - 7:, :T].abs().max()) == 0.0                 # rows without in-edges: zero type slots


@pytest.mark.parametrize("n,with_resid,with_carry", [(1000, True, True), (4099, False, False), (37, True, False)])
def test_merge_backward_width64(n, with_resid, with_carry):
    from tilingnn_amd import ops, train
    from tilingnn_amd._lib import check, lib, ptr
    r = _rng(n)
    z1, z2 = (r(n, W) + 0.2).to(DEV), (r(n, W) + 0.2).to(DEV)
    a1, a2 = torch.where(z1 > 0, z1, 0.01 * z1), torch.where(z2 > 0, z2, 0.01 * z2)
    bn1, bn2 = _bn(W, 1), _bn(W, 2)
    st1, st2 = _bn_stat(a1, bn1), _bn_stat(a2, bn2)
    dcat = r(n, 3 * W).to(DEV)                                           # dh lives in slot 2, the residual in slot 0
    before = dcat.clone()
    carry = r(n, W).to(DEV) if with_carry else None
    q1, q2 = z1.double().requires_grad_(True), z2.double().requires_grad_(True)
    y1, y2 = _bn_ref(q1, bn1, True), _bn_ref(q2, bn2, True)
    obj = (y1 * y2 * before[:, 2 * W:].double()).sum()
    if with_carry:
        obj = obj + (y2 * carry.double()).sum()
    obj.backward()
    dy1, dy2 = torch.empty(n, W, device=DEV), torch.empty(n, W, device=DEV)
    coef, dgb = torch.empty(2, 2, W, device=DEV), torch.empty(4, W, device=DEV)
    nb = lib.tgnn_reduce_workspace_bytes(W)
    ws = torch.empty(nb, dtype=torch.uint8, device=DEV)
    check(lib.tgnn_merge_bwd_reduce(ptr(dcat[:, 2 * W:]), 3 * W, ptr(a1), ptr(st1), ptr(a2), ptr(st2), ptr(carry), n, W,
                                    bn1.eps, bn2.eps, ptr(dy1), ptr(dy2), ptr(dcat) if with_resid else None, 3 * W,
                                    ptr(coef[0]), ptr(dgb[0]), ptr(dgb[1]), ptr(coef[1]), ptr(dgb[2]), ptr(dgb[3]), ptr(ws),
                                    nb, train._s(dy1)))
    dz1, _ = train.bn_bwd_apply(dy1, a1, st1, coef[0], ops.ACT_LEAKY_RELU)
    dz2, _ = train.bn_bwd_apply(dy2, a2, st2, coef[1], ops.ACT_LEAKY_RELU)
    assert _rel(dz1, q1.grad) < 1e-5 and _rel(dz2, q2.grad) < 1e-5
    # the BatchNorm parameter gradients from the same sweep: d gamma = sum dy xhat, d beta = sum dy
    dy1_ref = before[:, 2 * W:].double() * _bn_ref(z2.double(), bn2, True)
    dy2_ref = before[:, 2 * W:].double() * _bn_ref(z1.double(), bn1, True) + (carry.double() if with_carry else 0.0)
    for dy_ref, z, bn, k in ((dy1_ref, z1, bn1, 0), (dy2_ref, z2, bn2, 2)):
        xhat = (_bn_ref(z.double(), bn, True) - bn.bias.detach().double()) / bn.weight.detach().double()
        assert _rel(dgb[k], (dy_ref * xhat).sum(0)) < 1e-5 and _rel(dgb[k + 1], dy_ref.sum(0)) < 1e-5
    want_slot0 = before[:, :W] + before[:, 2 * W:] if with_resid else before[:, :W]
    assert torch.equal(dcat[:, :W], want_slot0) and torch.equal(dcat[:, W:], before[:, W:])


@pytest.mark.parametrize("with_stat", [False, True])
def test_gin_aggregate_width64(with_stat):
    from tilingnn_amd import ops, train
    n = 3001
    ei = _edges_with_a_hub(n, 25000, 5, 400, seed=7).to(DEV)
    rowptr, src, _, _ = ops.build_csr(ei, n, True)                      # GIN drops self loops (coll_conv.py)
    r = _rng(9)
    a = (r(n, W) + 0.3).to(DEV)
    eps = torch.tensor([0.25], device=DEV)
    bn = _bn(W, 4)
    stat = _bn_stat(a, bn) if with_stat else None
    got = train.gin_aggregate(a, rowptr, src, eps, n, in_stat=stat)
    x = _bn_ref(a.double(), bn, False) if with_stat else a.double()
    keep = ei[0] != ei[1]
    want = 1.25 * x + torch.zeros_like(x).index_add_(0, ei[1][keep], x[ei[0][keep]])
    assert _rel(got, want) < 1e-5


def test_wgrad_slot_major_width64_is_the_concatenation():
    from tilingnn_amd import train
    r = _rng(3)
    skip, dz = r(4, 3001, W).to(DEV), r(3001, 256).to(DEV)
    cat = torch.cat(list(skip), dim=1)                                   # TilinGNN.py:74
    got, gb = train.wgrad(dz, skip, slot_major=True, with_bias=True)
    want, wb = train.wgrad(dz, cat, with_bias=True)
    assert _rel(got, dz.double().t() @ cat.double()) < 2e-6 and _rel(gb, dz.double().sum(0)) < 2e-6
    assert torch.equal(got, want) and torch.equal(gb, wb)               # the same kernel, the same sums: the same bits
    small = r(21, 700, W).to(DEV)                                        # few rows: one row range, written directly
    dz2 = r(700, 64).to(DEV)
    assert _rel(train.wgrad(dz2, small, slot_major=True), dz2.double().t() @ torch.cat(list(small), 1).double()) < 2e-6


# ---------------------------------------------------------------------------------------------- the training forward keeps
def test_forward_train_keeps_what_the_backward_reads():
    """Width 64, depth 3, the labyrinth layout: every buffer tgnn_forward_train keeps, against the fp64 oracle's intermediates
    (orc.tilingnn_forward(capture=...)); u must be the GIN aggregate its MLP read."""
    from tilingnn_amd import train
    g = load_labyrinth_graph()
    net, sd = _net(15, 3, 4)
    x, adj, attr, col, _ = graph_tensors(g, torch.float32, DEV)
    n = int(x.shape[0])
    probs, sv = train.forward_train(net, x, adj, attr, col)
    sd64 = orc.cast_sd(sd, torch.float64)
    xc, adjc, attrc, colc, _ = graph_tensors(g, torch.float64)
    cap = {}
    with torch.no_grad():
        want_p, _ = orc.tilingnn_forward(sd64, xc, adjc, attrc, colc, capture=cap)
    tol = 2e-3            # fp32 against fp64 through up to 5 train-mode BatchNorms

    def stat_ok(stat, a_ref, prefix):
        mean = a_ref.mean(0)
        ginv = sd64[prefix + ".weight"] / torch.sqrt(((a_ref - mean) ** 2).mean(0) + 1e-5)
        assert _rel(stat[0].double() + stat[1].double(), mean) < tol, prefix
        assert _rel(stat[2], ginv) < tol and _rel(stat[3], sd64[prefix + ".bias"]) < 1e-6, prefix

    leaky = orc.leaky_relu
    # init MLP
    a0 = leaky(orc.linear(xc, sd64, "init_node_feature_trans.mlp.0.linear"))
    a1i = leaky(orc.linear(orc.batch_norm_train(a0, sd64, "init_node_feature_trans.mlp.0.batch_norm"), sd64,
                           "init_node_feature_trans.mlp.1.linear"))
    assert _rel(sv.init_a[0], a0) < tol and _rel(sv.init_a[1], a1i) < tol
    stat_ok(sv.init_stat[0], a0, "init_node_feature_trans.mlp.0.batch_norm")
    stat_ok(sv.init_stat[1], a1i, "init_node_feature_trans.mlp.1.batch_norm")
    # message-passing layers
    T = sv.tg.g.n_types
    for i in range(3):
        p1, p2 = f"brch_1_graph_conv_layers.{i}", f"brch_2_coll_conv_layers.{i}"
        assert _rel(sv.a1[i], leaky(cap[f"nnconv.{i}"])) < tol, i
        assert _rel(sv.a2[i], leaky(cap[f"gin.{i}"])) < tol, i
        stat_ok(sv.stat1[i], leaky(cap[f"nnconv.{i}"]), p1 + ".batch_norm")
        stat_ok(sv.stat2[i], leaky(cap[f"gin.{i}"]), p2 + ".batch_norm")
        h2 = cap[f"h2_in.{i}"]
        keep = colc[0] != colc[1]
        u_ref = (1.0 + sd64[p2 + ".ginConv.eps"]) * h2 + torch.zeros_like(h2).index_add_(0, colc[1][keep], h2[colc[0][keep]])
        assert _rel(sv.u[i], u_ref) < tol, i
        # teacher forced on the kept input: u is the aggregate of BN(a2_{i-1}) (the init output at layer 0)
        h2_in, h2_stat = (sv.skip[0], None) if i == 0 else (sv.a2[i - 1], sv.stat2[i - 1])
        u_kept = train.gin_aggregate(h2_in, sv.tg.g.col_rowptr, sv.tg.g.col_src, net.brch_2_coll_conv_layers[i].ginConv.eps, n,
                                     in_stat=h2_stat)
        assert _rel(sv.u[i], u_kept) < 1e-6, i
        rep = sv.tg.g.type_rep_edge[:T].long().cpu()
        wt_ref = orc.edge_weight_matrices(attrc[rep], sd64, p1 + ".mlp", W, W)
        assert _rel(sv.wtab[i], wt_ref) < 1e-5, i
    for k in range(4):
        assert _rel(sv.skip[k], cap["init"] if k == 0 else cap[f"mid.{k}"]) < tol, k
    # final MLP
    v = cap["cat"]
    for l in range(4):
        pre = f"final_mlp.0.mlp.{l}"
        a = leaky(orc.linear(v, sd64, pre + ".linear"))
        assert _rel(sv.fin_a[l], a) < tol, l
        stat_ok(sv.fin_stat[l], a, pre + ".batch_norm")
        v = orc.batch_norm_train(a, sd64, pre + ".batch_norm")
    assert _rel(probs, want_p) < tol


# ---------------------------------------------------------------------------------------------- the whole step
# The gate of tests/test_training_hip.py::test_training_step_with_many_edge_types, whose comment above GRAD_SEEDS gives the
# reasoning: which parameters a float32 run of this ill-conditioned step gets wrong is a lottery of the rounding realisation
# (a seed draws a bad one with probability ~0.3), so over NINE seeds at least THREE must have their worst parameter within
# 4 x of the float32 oracle's own error, and none may be off by more than the float32 oracle itself can be.  A wrong adjoint
# is off on every seed and fails both.
# The float32 oracle's own error is itself ONE draw of that lottery.  On the labyrinth layout at depth 3 (width 64) relabelling
# the nodes -- the same arithmetic summed in another order -- moves the float32 oracle's worst parameter from 7.9e-2 to 2.1e-1
# (seed 2) and its error on the init layer's bias (a sum that nearly cancels) from 2.1e-2 to 5.8e-2 (seed 5).  So the yardstick
# here is the float32 oracle's error over TWO realisations, the graph as given and with its nodes relabelled, per parameter the
# larger: the same rule, with the float32 oracle's own error measured rather than sampled once.
GRAD_SEEDS = (1, 2, 3, 4, 5, 6, 7, 8, 9)


def _f32_oracle_err(sd, x, adj, attr, col, ref_grads):
    """{parameter: the float32 oracle's relative error against the fp64 gradients}, the larger of two rounding realisations."""
    n = int(x.shape[0])
    p = torch.randperm(n, generator=torch.Generator().manual_seed(0))
    inv = torch.empty_like(p)
    inv[p] = torch.arange(n)
    sd32 = orc.cast_sd(sd, torch.float32)
    _, _, _, g_a = orc.training_step_grads(sd32, x, adj, attr, col)
    _, _, _, g_b = orc.training_step_grads(sd32, x[p], inv[adj], attr, inv[col])
    return {k: max(_rel(g_a[k], ref_grads[k]), _rel(g_b[k], ref_grads[k])) for k in ref_grads}


def _synth():
    from tilingnn_amd.synth import make_super_graph
    sg = make_super_graph(600, 6000, 7500, tile_count=2, n_edge_types=25, seed=9)
    return sg.to_torch(DEV)[:4], 2 + 25, 2


def _laby():
    return graph_tensors(load_labyrinth_graph(), torch.float32, DEV)[:4], 15, 3


@pytest.mark.parametrize("case", ["synthetic", "labyrinth"])
def test_training_step_width64_against_the_oracle(case):
    """Every parameter gradient of one width-64 step against the fp64 oracle (autograd over the restatement), with the
    float32 oracle's own error as the yardstick.  The oracle materialises [Ea, 4096] per layer at this width: depth <= 3."""
    from tilingnn_amd.graph_networks.networks.TilinGNN import TilinGNN
    from tilingnn_amd.solver.ml_solver.losses import Losses
    from tilingnn_amd.weights import make_state_dict
    (x, adj, attr, col), fe, depth = _synth() if case == "synthetic" else _laby()
    torch.set_num_threads(8)
    worst = []
    for seed in GRAD_SEEDS:
        net = TilinGNN(adj_edge_features_dim=fe, network_depth=depth, network_width=W, node_features_dim=3)
        sd = make_state_dict(fe, depth, W, 1, 3, seed=seed)
        net.load_state_dict(sd)
        net = net.to(DEV).train()
        net.autograd = True
        probs, _ = net(x, adj, attr, col)
        loss, _, _ = Losses.calculate_unsupervised_loss(probs, x, col, adj, attr)
        loss.backward()
        _, ref_loss, _, ref_grads = orc.training_step_grads(orc.cast_sd(sd, torch.float64), x.double().cpu(), adj.cpu(),
                                                            attr.double().cpu(), col.cpu())
        assert abs(float(loss.detach()) - float(ref_loss)) < 1e-4 * float(ref_loss)
        err32 = _f32_oracle_err(sd, x.cpu(), adj.cpu(), attr.cpu(), col.cpu(), ref_grads)
        floor = float(np.median(list(err32.values())))
        errs = {k: _rel(p.grad, ref_grads[k]) for k, p in net.named_parameters()}
        assert set(errs) == set(err32)
        print(f"{case} seed {seed}: worst parameter ours {max(errs.values()):.2e}, float32 oracle's worst "
              f"{max(err32.values()):.2e}, float32 oracle's median {floor:.2e}")
        assert max(errs.values()) < max(0.06, 2.0 * max(err32.values())), max(errs.items(), key=lambda kv: kv[1])
        worst.append(max(e / (max(err32[k], floor) + 2.5e-6) for k, e in errs.items()))
    print("worst parameter, ours / float32 oracle, per seed:", [f"{w:.1f}" for w in worst])
    assert sorted(worst)[2] <= 4.0, worst


@pytest.mark.parametrize("depth", [3, 20])
def test_library_backward_equals_the_spelled_out_schedule_width64(depth):
    """tgnn_backward and train.backward_train enqueue the same kernels in the same order at width 64: the same bits."""
    from tilingnn_amd import train
    net, _ = _net(15, depth, 0)
    x, adj, attr, col, _ = graph_tensors(load_labyrinth_graph(), torch.float32, DEV)
    probs, sv = train.forward_train(net, x, adj, attr, col)
    dprobs = _rng(1)(int(x.shape[0]), 1).to(DEV) * 1e-2
    a = train.backward_library(net, sv, dprobs)
    b = train.backward_train(net, sv, dprobs)
    assert sorted(a) == sorted(b) == sorted(k for k, _ in net.named_parameters())
    for k in a:
        assert torch.isfinite(a[k]).all(), k
        assert torch.equal(a[k].reshape(-1), b[k].reshape(-1)), k


# ---------------------------------------------------------------------------------------------- end to end
def test_trainer_loop_width64_checkpoint_scores_in_bf16(tmp_path):
    """Trainer.train on a width-64 network over layout files: the loss falls over 4 epochs and checkpoints are written; the
    checkpoint loads through ML_Solver.load_saved_network into a fresh width-64 TilinGNN, which scores the labyrinth layout
    with bf16 activation storage (config 3) next to the fp64 oracle on the same weights."""
    import os
    from tests.golden_util import GOLDEN
    from tilingnn_amd.graph_networks.networks.TilinGNN import TilinGNN
    from tilingnn_amd.solver.ml_solver.ml_solver import ML_Solver
    from tilingnn_amd.solver.ml_solver.trainer import Trainer
    from tilingnn_amd.tiling.tile_graph import TileGraph
    from tilingnn_amd.util import data_util as du
    graph = TileGraph(2)
    graph.load_graph_state(os.path.join(GOLDEN, "complete_graph_small.pkl"), sidecar=False)
    rng = np.random.default_rng(0)
    for split, count in (("train", 4), ("test", 2)):
        os.makedirs(tmp_path / split, exist_ok=True)
        for i in range(count):
            tiles = sorted(int(v) for v in rng.choice(150, size=int(rng.integers(60, 140)), replace=False))
            x, ci, cf, ai, af, re_index = du.create_brick_layout_from_super_set(graph, tiles)
            du.write_brick_layout_data(f"layout_{i}.pkl", re_index, node_features=x, collide_edge_index=ci,
                                       collide_edge_features=cf, align_edge_index=ai, align_edge_features=af,
                                       prefix=str(tmp_path / split / "raw"))
    net, _ = _net(15, 3, 5)
    solver = ML_Solver(None, DEV, graph, net, num_prob_maps=1)
    opt = torch.optim.Adam(net.parameters(), lr=2e-3)
    trainer = Trainer(None, None, DEV, net, str(tmp_path))
    history = trainer.train(solver, opt, batch_size=1, training_epoch=4, save_model_per_epoch=2, shuffle_seed=1,
                            log=lambda *_: None)
    assert len(history) == 4 and history[-1][0] < history[0][0] and all(np.isfinite(h).all() for h in history)
    saved = sorted(os.listdir(tmp_path / "model"))
    models = [f for f in saved if f.startswith("model_")]
    assert any(f.startswith("model_0_") for f in saved) and any(f.startswith("optimizer_0_") for f in saved)
    assert not net.autograd

    fresh = TilinGNN(adj_edge_features_dim=15, network_depth=3, network_width=W, node_features_dim=3).to(DEV)
    loader = ML_Solver(None, DEV, graph, fresh, num_prob_maps=1)
    ckpt = str(tmp_path / "model" / models[-1])
    loader.load_saved_network(ckpt)
    sd = torch.load(ckpt, map_location="cpu")
    for k, v in fresh.state_dict().items():
        assert torch.equal(v.cpu(), sd[k]), k
    fresh.activation_dtype = torch.bfloat16
    x, adj, attr, col, _ = graph_tensors(load_labyrinth_graph(), torch.float32, DEV)
    with torch.no_grad():
        probs, _ = fresh(x=x, adj_e_index=adj, adj_e_features=attr, col_e_idx=col)
        want, _ = orc.tilingnn_forward(orc.cast_sd(sd, torch.float64), x.double().cpu(), adj.cpu(), attr.double().cpu(), col.cpu())
    p = probs.float().cpu().numpy()
    assert probs.shape == (1254, 1) and np.isfinite(p).all() and (p > 0).all() and (p < 1).all()
    print(f"trained width-64 checkpoint, bf16 storage: mean probability {p.mean():.4f} vs fp64 {want.numpy().mean():.4f}")
    assert abs(p.mean() - want.numpy().mean()) < 5e-2


# ---------------------------------------------------------------------------------------------- boundaries
def test_other_widths_and_too_many_edge_types_still_raise():
    from tilingnn_amd.solver.ml_solver.losses import Losses
    from tilingnn_amd.synth import make_super_graph
    x, adj, attr, col, _ = graph_tensors(load_labyrinth_graph(), torch.float32, DEV)
    net, _ = _net(15, 2, 1, width=96)
    net.autograd = True
    with pytest.raises(NotImplementedError, match="32 or 64"):
        probs, _ = net(x, adj, attr, col)
        Losses.calculate_unsupervised_loss(probs, x, col, adj, attr)[0].backward()
    sg = make_super_graph(400, 4000, 5000, tile_count=2, n_edge_types=64, seed=3)
    x, adj, attr, col, _ = sg.to_torch(DEV)
    assert torch.unique(attr, dim=0).shape[0] == 64
    net, _ = _net(2 + 64, 2, 1)
    net.autograd = True
    with pytest.raises(NotImplementedError, match="at most 63"):
        net(x, adj, attr, col)
