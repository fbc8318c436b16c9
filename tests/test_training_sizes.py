"""The adjoint kernels of the training step at the sizes they run at and on graphs whose transpose is another graph.

tests/test_training_hip.py and tests/test_training_width64.py stop at 5 000 rows, and every larger graph they use stores both
directions of every pair.  Here: N_BIG = 66 003 rows (past every block / partial-row cap of csrc/backward.hip: the 8192 x 8 and
16384 x 4 rows of the type sums, the 512 partial rows of the column sums, the 512 row ranges of the weight gradient, the
2048 x 256 edges of the loss backward), N_MID = 4 099 at width 32 where only width 64 had kernel tests, and the directed graphs
of tests/train_graphs.py (one direction per pair, hubs whose in- and out-degree differ by hundreds).  Every check is teacher
forced -- same kept inputs, same upstream gradient, one layer in fp64 -- so BatchNorm amplification does not enter and the gates
are the kernel tests' own: 1e-6 .. 1e-5."""
import functools
from types import SimpleNamespace

import pytest
import torch

from oracle import tilingnn_oracle as orc
from tests import train_graphs as tgr
from tests.golden_util import graph_tensors, load_labyrinth_graph
from tests.train_graphs import N_BIG, N_MID

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
FE = 15                                    # edge-attribute columns (the labyrinth layout's)
WIDTHS = [32, 64]


def _rel(got, want):
    got = got.detach().double()
    want = want.detach().double().to(got.device)
    return float((got - want).abs().max() / want.abs().max().clamp(min=1e-30))


def _gate(what, got, want, bound):
    err = _rel(got, want)
    print(f"{what}: {err:.2e} (gate {bound:.0e})")
    assert err < bound, (what, err)


def _rng(seed):
    g = torch.Generator().manual_seed(seed)
    return lambda *shape: torch.randn(*shape, generator=g)


def _net(fe, depth, seed, width):
    from tilingnn_amd.graph_networks.networks.TilinGNN import TilinGNN
    from tilingnn_amd.weights import make_state_dict
    net = TilinGNN(adj_edge_features_dim=fe, network_depth=depth, network_width=width, node_features_dim=3)
    sd = make_state_dict(fe, depth, width, 1, 3, seed=seed)
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


@functools.lru_cache(maxsize=None)
def _prepared(n, T):
    """The directed graph of (n, T) on the device, prepared both ways; built once and read only."""
    from tilingnn_amd import ops, train
    ea, ec = (tgr.EA_BIG, tgr.EC_BIG) if n == N_BIG else (30000, 25000)
    cpu = tgr.directed_graph(n, ea, ec, T, FE, seed=1000 + T)
    x, adj, attr, col = (t.to(DEV) for t in cpu)
    graph = ops.prepare_graph(n, adj, attr, col)
    assert graph.n_types == T and graph.n_adj_edges == ea
    return SimpleNamespace(n=n, ea=ea, ec=ec, cpu=cpu, x=x, adj=adj, attr=attr, col=col, graph=graph,
                           tg=train.TrainGraph(graph, adj, col))


# ---------------------------------------------------------------------------------------------- 1. type sums
@pytest.mark.parametrize("width", WIDTHS)
@pytest.mark.parametrize("n,T", [(N_MID, 0), (N_MID, 1), (N_MID, 13), (N_MID, 63), (N_BIG, 2)])
def test_type_sums_on_the_directed_graph(n, T, width):
    """tgnn_nnconv_type_sum over the forward CSR and over the transposed CSR TrainGraph builds: rows without in-edges, a hub row
    of 700 edges (of one type on the forward CSR), a row stride wider than the width, a root scale; width 32 at T = 63 asks for
    exactly 64 KiB of dynamic LDS; at N_BIG every block takes a second trip of the grid-stride loop.  T = 0: the arrays of the
    one-type graph with no type slot (the kernel must leave nothing of the edges behind)."""
    from tilingnn_amd import train
    p = _prepared(n, max(T, 1))
    g, tg, adj = p.graph, p.tg, p.adj
    et = g.edge_type[:p.ea].long()
    r = _rng(n + 7 * T + width)
    wide = r(n, width + 16).to(DEV)
    rows = wide[:, :width]                                   # ld_rows = width + 16
    own = r(n, width).to(DEV)
    scale = (r(n).abs() + 0.5).to(DEV)
    no_in_edges = {"forward": slice(n - tgr.NO_IN_TAIL, n), "transposed": slice(*tgr.NO_OUT)}
    for name, rowptr, src, typ, gather_from, scatter_to in (
            ("forward", g.adj_rowptr, g.adj_src, g.adj_type, adj[0], adj[1]),
            ("transposed", tg.adjT_rowptr, tg.adjT_src, tg.adjT_type, adj[1], adj[0])):
        got = train.type_sum(rows, own, scale, rowptr, src, typ, n, T).view(n, T + 1, width)
        want = torch.zeros(n, T + 1, width, dtype=torch.float64, device=DEV)
        if T:
            want.view(n * (T + 1), width).index_add_(0, scatter_to * (T + 1) + et, rows.double()[gather_from])
        want[:, T] = own.double() * scale.double()[:, None]
        _gate(f"type sums, {name} CSR", got, want, 1e-6)
        if T:
            assert float(got[no_in_edges[name], :T].abs().max()) == 0.0     # rows without in-edges: zero type slots
            hub = tgr.ADJ_SINK if name == "forward" else tgr.ADJ_SOURCE
            assert float(want[hub, :T].abs().max()) > 0.0
    # the mean divides by the IN-degree
    deg = torch.bincount(adj[1], minlength=n).clamp(min=1).float()
    assert torch.equal(tg.deg, deg) and _rel(tg.inv_deg, 1.0 / deg.double()) < 1e-7
    assert float(deg[tgr.ADJ_SINK]) >= 700 and float(deg[tgr.ADJ_SOURCE]) < 100


# ---------------------------------------------------------------------------------------------- 2. GIN aggregation
@pytest.mark.parametrize("with_stat", [False, True])
@pytest.mark.parametrize("n,width", [(N_MID, 32), (N_BIG, 32), (N_BIG, 64)])
def test_gin_aggregate_on_the_directed_graph(n, width, with_stat):
    """tgnn_gin_aggregate over the collision CSR (the forward's use) and over its transpose (the adjoint's): self loops dropped,
    hubs of 400 edges on either side, with and without the BatchNorm record folded into the gather."""
    from tilingnn_amd import train
    p = _prepared(n, 13)
    g, tg, col = p.graph, p.tg, p.col
    a = (_rng(9 + width)(n, width) + 0.3).to(DEV)
    eps = torch.tensor([0.25], device=DEV)
    bn = _bn(width, 4)
    stat = _bn_stat(a, bn) if with_stat else None
    x = _bn_ref(a.double(), bn, False) if with_stat else a.double()
    for name, rowptr, src, s, d in (("collision CSR", g.col_rowptr, g.col_src, col[0], col[1]),
                                    ("transposed", tg.colT_rowptr, tg.colT_src, col[1], col[0])):
        got = train.gin_aggregate(a, rowptr, src, eps, n, in_stat=stat)
        keep = s != d
        want = 1.25 * x + torch.zeros_like(x).index_add_(0, d[keep], x[s[keep]])
        _gate(f"GIN aggregate, {name}", got, want, 1e-5)


# ---------------------------------------------------------------------------------------------- 3. capped reductions
@pytest.mark.parametrize("c", [32, 256])
def test_colsum_past_the_partial_cap(c):
    """66 003 rows: 512 partial rows of 129 rows each (the last one short)."""
    from tilingnn_amd import train
    x = _rng(c)(N_BIG, c).to(DEV)
    _gate("colsum", train.colsum(x), x.double().sum(0), 1e-6)
    wide = _rng(c + 1)(N_BIG, c + 8).to(DEV)
    _gate("colsum, row stride > width", train.colsum(wide[:, :c]), wide[:, :c].double().sum(0), 1e-6)


@pytest.mark.parametrize("leaky", [True, False])
@pytest.mark.parametrize("f", [32, 256])
def test_batchnorm_backward_past_the_partial_cap(f, leaky):
    from tilingnn_amd import ops, train
    n = N_BIG
    r = _rng(n + f)
    z = (r(n, f) + 0.3).to(DEV)
    a = torch.where(z > 0, z, 0.01 * z) if leaky else z
    dy, scale = r(n, f).to(DEV), (r(n).abs() + 0.5).to(DEV)
    bn = _bn(f, 7)
    zz = z.double().requires_grad_(True)
    gam, bet = bn.weight.detach().double().requires_grad_(True), bn.bias.detach().double().requires_grad_(True)
    aa = torch.where(zz > 0, zz, 0.01 * zz) if leaky else zz
    y = (aa - aa.mean(0)) / torch.sqrt(aa.var(0, unbiased=False) + bn.eps) * gam + bet
    (y * dy.double()).sum().backward()
    dz, scaled, dgamma, dbeta = train.bn_bwd(dy, a, _bn_stat(a, bn), bn.eps, ops.ACT_LEAKY_RELU if leaky else ops.ACT_NONE,
                                             row_scale=scale)
    _gate("dz", dz, zz.grad, 1e-5)
    _gate("d gamma", dgamma, gam.grad, 1e-5)
    _gate("d beta", dbeta, bet.grad, 1e-5)
    _gate("dz * row scale", scaled, zz.grad * scale.double()[:, None], 1e-5)


@pytest.mark.parametrize("width", WIDTHS)
def test_merge_backward_past_the_partial_cap(width):
    """tgnn_merge_bwd_reduce with residual and carry at 66 003 rows: 129 rows per partial row round up to 160, so 413 of the
    512 partial rows are used and the last block is short."""
    from tilingnn_amd import ops, train
    from tilingnn_amd._lib import check, lib, ptr
    n, W = N_BIG, width
    r = _rng(n + W)
    z1, z2 = (r(n, W) + 0.2).to(DEV), (r(n, W) + 0.2).to(DEV)
    a1, a2 = torch.where(z1 > 0, z1, 0.01 * z1), torch.where(z2 > 0, z2, 0.01 * z2)
    bn1, bn2 = _bn(W, 1), _bn(W, 2)
    st1, st2 = _bn_stat(a1, bn1), _bn_stat(a2, bn2)
    dcat = r(n, 3 * W).to(DEV)                                           # dh lives in slot 2, the residual in slot 0
    before = dcat.clone()
    carry = r(n, W).to(DEV)
    q1, q2 = z1.double().requires_grad_(True), z2.double().requires_grad_(True)
    y1, y2 = _bn_ref(q1, bn1, True), _bn_ref(q2, bn2, True)
    ((y1 * y2 * before[:, 2 * W:].double()).sum() + (y2 * carry.double()).sum()).backward()
    dy1, dy2 = torch.empty(n, W, device=DEV), torch.empty(n, W, device=DEV)
    coef, dgb = torch.empty(2, 2, W, device=DEV), torch.empty(4, W, device=DEV)
    nb = lib.tgnn_reduce_workspace_bytes(W)
    ws = torch.empty(nb, dtype=torch.uint8, device=DEV)
    check(lib.tgnn_merge_bwd_reduce(ptr(dcat[:, 2 * W:]), 3 * W, ptr(a1), ptr(st1), ptr(a2), ptr(st2), ptr(carry), n, W,
                                    bn1.eps, bn2.eps, ptr(dy1), ptr(dy2), ptr(dcat), 3 * W, ptr(coef[0]), ptr(dgb[0]),
                                    ptr(dgb[1]), ptr(coef[1]), ptr(dgb[2]), ptr(dgb[3]), ptr(ws), nb, train._s(dy1)))
    dz1, _ = train.bn_bwd_apply(dy1, a1, st1, coef[0], ops.ACT_LEAKY_RELU)
    dz2, _ = train.bn_bwd_apply(dy2, a2, st2, coef[1], ops.ACT_LEAKY_RELU)
    _gate("dz1", dz1, q1.grad, 1e-5)
    _gate("dz2", dz2, q2.grad, 1e-5)
    with torch.no_grad():
        dy1_ref = before[:, 2 * W:].double() * y2
        dy2_ref = before[:, 2 * W:].double() * y1 + carry.double()
        for dy_ref, y, bn, k in ((dy1_ref, y1, bn1, 0), (dy2_ref, y2, bn2, 2)):
            xhat = (y - bn.bias.detach().double()) / bn.weight.detach().double()
            _gate(f"d gamma {k // 2 + 1}", dgb[k], (dy_ref * xhat).sum(0), 1e-5)
            _gate(f"d beta {k // 2 + 1}", dgb[k + 1], dy_ref.sum(0), 1e-5)
    assert torch.equal(dcat[:, :W], before[:, :W] + before[:, 2 * W:])   # the residual slot: one fp32 addition per element
    assert torch.equal(dcat[:, W:], before[:, W:])                       # the other slots: untouched


@pytest.mark.parametrize("cout,cin", [(32, 32), (32, 448), (256, 128)])
def test_wgrad_past_the_row_range_cap(cout, cin):
    """66 003 rows: at (32, 32) the plan stops at its 512 row ranges (of 144 rows: 459 are used); the wider shapes split the
    rows into 276 and 243 ranges."""
    from tilingnn_amd import train
    r = _rng(cout + cin)
    dz, x = r(N_BIG, cout).to(DEV), r(N_BIG, cin).to(DEV)
    w, b = train.wgrad(dz, x, with_bias=True)
    _gate("dW", w, dz.double().t() @ x.double(), 2e-6)
    _gate("d bias", b, dz.double().sum(0), 2e-6)


@pytest.mark.parametrize("width", WIDTHS)
def test_wgrad_slot_major_past_the_row_range_cap(width):
    from tilingnn_amd import train
    r = _rng(3 + width)
    skip, dz = r(3, N_BIG, width).to(DEV), r(N_BIG, 256).to(DEV)
    cat = torch.cat(list(skip), dim=1)                                   # TilinGNN.py:74
    got, gb = train.wgrad(dz, skip, slot_major=True, with_bias=True)
    _gate("dW over slots", got, dz.double().t() @ cat.double(), 2e-6)
    _gate("d bias", gb, dz.double().sum(0), 2e-6)
    want, wb = train.wgrad(dz, cat, with_bias=True)
    assert torch.equal(got, want) and torch.equal(gb, wb)               # the same kernel, the same sums: the same bits


# ---------------------------------------------------------------------------------------------- 4. composed adjoints
@pytest.mark.parametrize("width", WIDTHS)
@pytest.mark.parametrize("n,T", [(N_MID, 13), (N_MID, 63), (N_BIG, 13)])
def test_nnconv_and_gin_adjoints_teacher_forced_on_the_directed_graph(n, T, width):
    """train.nnconv_backward and train.gin_backward against fp64 autograd over the oracle's ops (the chunked NNConv:
    tests/test_training_sizes_host.py pins its gradients to the reference's op sequence), same inputs and same upstream
    gradient.  On this graph the transposed CSR is not the forward CSR and in-degree is not out-degree; at T = 63 the
    input-gradient product is a dense_act with K = 64 width."""
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

    # ---- NNConv
    wtab = ops.edge_weight_table(attr, tg.g, *l1.nnConv._edge_mlp_params(), width).contiguous()
    grads = {}
    dh = train.nnconv_backward(l1.nnConv, p1, tg, wtab, h, dz, dz * tg.inv_deg[:, None], attr, grads)
    leaf = {k: (v.clone().requires_grad_(True) if k.startswith(p1) and v.is_floating_point() else v) for k, v in sd64.items()}
    hh = h.double().cpu().requires_grad_(True)
    out = orc.nnconv_mean_dedup(hh, adj_c, attr_c.double(), leaf, p1)
    (out * dz.double().cpu()).sum().backward()
    _gate("NNConv dh", dh, hh.grad, 1e-5)
    for k, v in grads.items():
        _gate(k, v.reshape(leaf[k].shape), leaf[k].grad, 1e-5)
    assert set(grads) == {p1 + ".nnConv.root", p1 + ".nnConv.bias"} | {f"{p1}.mlp.mlp.{k}.linear.{w}" for k in range(3)
                                                                       for w in ("weight", "bias")}

    # ---- GIN
    leaf = {k: (v.clone().requires_grad_(True) if k.startswith(p2) and v.is_floating_point() and not k.endswith(".eps")
                else v) for k, v in sd64.items()}
    out = orc.gin_conv(hh := h.double().cpu().requires_grad_(True), col_c, leaf, p2)
    (out * dz.double().cpu()).sum().backward()
    u = train.gin_aggregate(h, tg.g.col_rowptr, tg.g.col_src, l2.ginConv.eps, n)
    gw = l2.ginConv._mlp_params()
    t1 = ops.dense_act(u, gw[0], gw[1], ops.ACT_SIGMOID)[0]
    t3 = ops.dense_act(ops.dense_act(t1, gw[2], gw[3], ops.ACT_SIGMOID)[0], gw[4], gw[5], ops.ACT_SIGMOID)[0]
    grads = {}
    dh2 = train.gin_backward(l2.ginConv, p2, tg, u, t3, dz, grads)
    _gate("GIN dh", dh2, hh.grad, 1e-5)
    for k, v in grads.items():
        _gate(k, v.reshape(leaf[k].shape), leaf[k].grad, 1e-5)
    assert set(grads) == {f"{p2}.ginConv.nn.mlp.{k}.linear.{w}" for k in range(3) for w in ("weight", "bias")}


# ---------------------------------------------------------------------------------------------- 5. what the forward keeps
def test_forward_train_keeps_what_the_backward_reads_width32():
    """tests/test_training_width64.py::test_forward_train_keeps_what_the_backward_reads at width 32, the reference's own
    network_width: depth 3, the labyrinth layout, every buffer tgnn_forward_train keeps against the fp64 oracle's
    intermediates; u must be the GIN aggregate its MLP read.  Same tolerances."""
    from tilingnn_amd import train
    W = 32
    g = load_labyrinth_graph()
    net, sd = _net(15, 3, 4, W)
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


BIG_DEPTH = 2


@functools.lru_cache(maxsize=None)
def _big_forward(width):
    """One training forward at N_BIG (the general launch schedule), kept for the tests below; read only."""
    from tilingnn_amd import train
    p = _prepared(N_BIG, 13)
    net, sd = _net(FE, BIG_DEPTH, 3, width)
    probs, sv = train.forward_train(net, p.x, p.adj, p.attr, p.col)
    return net, sd, probs, sv


@pytest.mark.parametrize("width", WIDTHS)
def test_forward_train_keeps_what_the_backward_reads_at_size(width):
    """66 003 nodes, depth 2, teacher forced only (no oracle forward): every kept buffer against fp64 of the kept buffers it was
    made from.  u: the GIN aggregate of the kept input under its kept record (1e-6); wtab: the oracle's edge MLP on the
    representative rows (1e-5); every BatchNorm record: the fp64 mean and gamma / sqrt(var + eps) of the kept activation itself
    (1e-6: the kernel sums in fp64 and rounds once); skip[k + 1] = BN1(a1_k) BN2(a2_k) (+ skip[k - 2] from k = 2 on,
    TilinGNN.py:67-69) from the kept activations in fp64 (1e-5)."""
    from tilingnn_amd import train
    net, sd, probs, sv = _big_forward(width)
    p = _prepared(N_BIG, 13)
    n, T = N_BIG, 13
    sd64 = orc.cast_sd(sd, torch.float64)
    assert sv.tg.g.n_types == T and torch.isfinite(probs).all()

    def bn64(stat, a, bn, what):
        """checks the record, returns BatchNorm(a) in fp64 from a's own statistics"""
        a64 = a.double()
        mean = a64.mean(0)
        invstd = 1.0 / torch.sqrt(((a64 - mean) ** 2).mean(0) + bn.eps)
        gamma, beta = bn.weight.detach().double(), bn.bias.detach().double()
        _gate(what + " mean", stat[0].double() + stat[1].double(), mean, 1e-6)
        _gate(what + " gamma invstd", stat[2], gamma * invstd, 1e-6)
        _gate(what + " beta", stat[3], beta, 1e-6)
        return (a64 - mean) * invstd * gamma + beta

    init = net.init_node_feature_trans.mlp
    bn64(sv.init_stat[0], sv.init_a[0], init[0].batch_norm, "init 0")
    h0 = bn64(sv.init_stat[1], sv.init_a[1], init[1].batch_norm, "init 1")
    _gate("skip[0]", sv.skip[0], h0, 1e-5)
    rep = sv.tg.g.type_rep_edge[:T].long().cpu()
    for i in range(BIG_DEPTH):
        l1, l2 = net.brch_1_graph_conv_layers[i], net.brch_2_coll_conv_layers[i]
        y1 = bn64(sv.stat1[i], sv.a1[i], l1.batch_norm, f"layer {i} branch 1")
        y2 = bn64(sv.stat2[i], sv.a2[i], l2.batch_norm, f"layer {i} branch 2")
        want = y1 * y2 + (sv.skip[i - 2].double() if i >= 2 else 0.0)
        _gate(f"skip[{i + 1}]", sv.skip[i + 1], want, 1e-5)
        h2_in, h2_stat = (sv.skip[0], None) if i == 0 else (sv.a2[i - 1], sv.stat2[i - 1])
        u_kept = train.gin_aggregate(h2_in, sv.tg.g.col_rowptr, sv.tg.g.col_src, l2.ginConv.eps, n, in_stat=h2_stat)
        _gate(f"u[{i}]", sv.u[i], u_kept, 1e-6)
        wt_ref = orc.edge_weight_matrices(p.cpu[2].double()[rep], sd64, f"brch_1_graph_conv_layers.{i}.mlp", width, width)
        _gate(f"wtab[{i}]", sv.wtab[i], wt_ref, 1e-5)
    for l, layer in enumerate(net.final_mlp[0].mlp):
        bn64(sv.fin_stat[l], sv.fin_a[l], layer.batch_norm, f"final {l}")


# ---------------------------------------------------------------------------------------------- 6. the library backward
@pytest.mark.parametrize("width", WIDTHS)
def test_library_backward_equals_the_spelled_out_schedule_at_size(width):
    """tgnn_backward and train.backward_train at 66 003 nodes -- where tgnn_backward's workspace carving and every capped kernel
    matter: the same kernels in the same order, the same bits in every gradient; all finite."""
    from tilingnn_amd import train
    net, _, probs, sv = _big_forward(width)
    dprobs = _rng(1)(N_BIG, 1).to(DEV) * 1e-2
    a = train.backward_library(net, sv, dprobs)
    b = train.backward_train(net, sv, dprobs)
    assert sorted(a) == sorted(b) == sorted(k for k, _ in net.named_parameters())
    for k in a:
        assert torch.isfinite(a[k]).all() and torch.isfinite(b[k]).all(), k
        assert torch.equal(a[k].reshape(-1), b[k].reshape(-1)), k
        assert float(a[k].abs().max()) > 0.0, k


# ---------------------------------------------------------------------------------------------- 7. the loss backward
def test_loss_backward_past_its_grid_cap():
    """600 002 collision edges: more than the 2048 x 256 of one sweep of tgnn_unsupervised_loss_bwd's edge kernel."""
    from tilingnn_amd.solver.ml_solver.losses import Losses
    torch.set_num_threads(8)
    p = _prepared(N_BIG, 13)
    x_c, adj_c, attr_c, col_c = p.cpu
    q0 = 0.02 + 0.96 * torch.rand(N_BIG, 1, generator=torch.Generator().manual_seed(1))
    pr = q0.to(DEV).requires_grad_(True)
    loss, min_index, _ = Losses.calculate_unsupervised_loss(pr, p.x, p.col, p.adj, p.attr)
    (3.0 * loss).backward()
    q = q0.double().requires_grad_(True)
    ref = orc.unsupervised_losses(q, x_c.double(), col_c, adj_c, attr_c.double())
    (3.0 * ref.min()).backward()
    want_loss = float(ref.detach().min())
    gap = abs(float(loss.detach()) - want_loss) / want_loss
    print(f"loss: {gap:.2e} (gate 1e-05)")
    assert int(min_index) == 0 and gap < 1e-5
    _gate("d loss / d probs", pr.grad, q.grad, 1e-5)
