"""BASELINE config 3 on the GPU: network_width 64 with bf16 storage of the activations between kernels (csrc/bf16_path.hip).

Protocol: per op, TEACHER FORCED on bf16-rounded inputs, against the fp64 oracle evaluated on those same inputs.
Stated tolerance: 2^-7 = 7.8e-3 of the output's max-norm -- one bf16 rounding of the weights (the NNConv type matrices,
the GIN MLP, the first final Linear) plus one of the stored output, each 2^-9 relative per element; everything in between
(products, sums, BatchNorm statistics) is exact-product / fp32-sum / fp64-statistics arithmetic.  Measured values are
printed.  The BatchNorm partial sums must be the sums of the STORED (rounded) values to fp64 accuracy."""
import numpy as np
import pytest
import torch

from oracle import tilingnn_oracle as orc
from tests.golden_util import graph_tensors, load_labyrinth_graph
from tilingnn_amd.weights import make_state_dict

pytestmark = pytest.mark.gpu
TOL_BF16 = 2.0 ** -7
W = 64


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available()
    return torch.device("cuda:0")


def make_net(dev, fe=15, depth=20, fx=5, seed=0):
    from tilingnn_amd import TilinGNN
    net = TilinGNN(adj_edge_features_dim=fe, network_depth=depth, network_width=W, node_features_dim=fx)
    sd = make_state_dict(fe, depth, W, 1, fx, seed=seed)
    net.load_state_dict(sd, strict=True)
    return net.to(dev).train(), sd


def bf(t):
    """fp32/fp64 CPU tensor -> the bf16-rounded values, as float32."""
    return t.float().to(torch.bfloat16).float()


def sums_from(parts, n_parts, f=W):
    p = parts[: n_parts * 2 * f].view(n_parts, 2, f).sum(0).cpu()
    return p[0], p[1]


def layer_case(dev, g, n, depth, i, seed):
    from tilingnn_amd import ops
    net, sd = make_net(dev, depth=depth)
    sd64 = orc.cast_sd(sd, torch.float64)
    x, adj, attr, col, _ = g
    gen = torch.Generator().manual_seed(seed)
    h = bf(torch.randn(n, W, generator=gen))
    graph = ops.prepare_graph(n, adj, attr, col)
    return net, sd64, h, graph


def check_nnconv_and_gin(dev, g, n, i=1, chunked=False):
    from tilingnn_amd import ops, ops_bf16
    x, adj, attr, col, _ = g
    net, sd64, h, graph = layer_case(dev, g, n, 3, i, 7)
    adjc, attrc, colc = adj.cpu(), attr.cpu().double(), col.cpu()
    p1, p2 = f"brch_1_graph_conv_layers.{i}", f"brch_2_coll_conv_layers.{i}"
    leaky = torch.nn.functional.leaky_relu
    with torch.no_grad():
        nn_fn = orc.nnconv_mean_dedup if chunked else orc.nnconv_mean
        want_nn = leaky(nn_fn(h.double(), adjc, attrc, sd64, p1))
        want_gin = leaky(orc.gin_conv(h.double(), colc, sd64, p2))
    l1, l2 = net.brch_1_graph_conv_layers[i], net.brch_2_coll_conv_layers[i]
    wtab = ops.edge_weight_table(attr, graph, *l1.nnConv._edge_mlp_params(), W)
    parts = ops.new_partials(W, dev)
    hb = h.to(dev).to(torch.bfloat16)
    got, npart = ops_bf16.nnconv64(hb, graph, wtab, l1.nnConv.root, l1.nnConv.bias, ops.ACT_LEAKY_RELU, parts)
    e_nn = orc.rel_max_err(got.float().cpu(), want_nn)
    s, q = sums_from(parts, npart)
    gd = got.double().cpu()
    assert float((s - gd.sum(0)).abs().max()) < 1e-9 * float(gd.abs().sum(0).max())
    assert float((q - (gd * gd).sum(0)).abs().max()) < 1e-9 * float((gd * gd).sum(0).max())
    parts2 = ops.new_partials(W, dev)
    got_g, np2 = ops_bf16.gin64(hb, graph, l2.ginConv.eps, *l2.ginConv._mlp_params(), act=ops.ACT_LEAKY_RELU, partials=parts2)
    e_gin = orc.rel_max_err(got_g.float().cpu(), want_gin)
    s2, q2 = sums_from(parts2, np2)
    gd2 = got_g.double().cpu()
    assert float((s2 - gd2.sum(0)).abs().max()) < 1e-9 * float(gd2.abs().sum(0).max())
    assert float((q2 - (gd2 * gd2).sum(0)).abs().max()) < 1e-9 * float((gd2 * gd2).sum(0).max())
    # the two layer seams WITH their BatchNorm (GraphConv: statistics of the stored bf16 values; CollConv: the normalised
    # output is what is stored)
    with torch.no_grad():
        want_gc = orc.batch_norm_train(want_nn, sd64, p1 + ".batch_norm")
        want_cc = orc.batch_norm_train(want_gin, sd64, p2 + ".batch_norm")
    st1 = ops.bn_finalize(parts, npart, n, l1.batch_norm, update_running=False)
    e_gc = orc.rel_max_err(ops.bn_apply(got.float(), st1).cpu(), want_gc)
    cc = ops_bf16.collconv64(hb, graph, l2.ginConv.eps, *l2.ginConv._mlp_params(), l2.batch_norm, update_running=False)
    e_cc = orc.rel_max_err(cc.float().cpu(), want_cc)
    return e_nn, e_gin, e_gc, e_cc


def test_nnconv_and_gin_on_the_real_graph(dev):
    g = graph_tensors(load_labyrinth_graph(), torch.float32, dev)
    e_nn, e_gin, e_gc, e_cc = check_nnconv_and_gin(dev, g, 1254)
    print(f"bf16 path, labyrinth: NNConv {e_nn:.2e}, GIN {e_gin:.2e}, GraphConv incl. BN {e_gc:.2e}, CollConv incl. BN {e_cc:.2e} "
          "(max-norm relative vs fp64 on the same bf16 inputs)")
    assert max(e_nn, e_gin, e_gc, e_cc) < TOL_BF16


def test_gin_folds_the_previous_batchnorm(dev):
    """in_stat: GIN_{i+1} reads the pre-BatchNorm bf16 activations of layer i and applies BN_i inside its sum."""
    from tilingnn_amd import ops, ops_bf16
    g = graph_tensors(load_labyrinth_graph(), torch.float32, dev)
    x, adj, attr, col, _ = g
    net, sd64, a, graph = layer_case(dev, g, 1254, 3, 1, 11)
    l2 = net.brch_2_coll_conv_layers[1]
    gen = torch.Generator().manual_seed(3)
    gamma, beta = torch.rand(W, generator=gen) + 0.5, torch.randn(W, generator=gen)
    mean, var = a.double().mean(0), a.double().var(0, unbiased=False)
    mh = mean.float()
    stat = torch.stack([mh, (mean - mh.double()).float(), (gamma.double() / torch.sqrt(var + 1e-5)).float(), beta])
    xin = ((a.double() - mean) / torch.sqrt(var + 1e-5)) * gamma.double() + beta.double()
    with torch.no_grad():
        want = orc.gin_conv(xin, col.cpu(), sd64, "brch_2_coll_conv_layers.1")
    got, _ = ops_bf16.gin64(a.to(dev).to(torch.bfloat16), graph, l2.ginConv.eps, *l2.ginConv._mlp_params(), in_stat=stat.to(dev))
    err = orc.rel_max_err(got.float().cpu(), want)
    print(f"bf16 GIN with folded BatchNorm: {err:.2e}")
    assert err < TOL_BF16


def test_merge_and_final_linear(dev):
    from tilingnn_amd import ops, ops_bf16
    n, s = 5000, 21
    gen = torch.Generator().manual_seed(5)
    a1, a2, r = (bf(torch.randn(n, W, generator=gen)) for _ in range(3))
    def record(v):
        mean, var = v.double().mean(0), v.double().var(0, unbiased=False)
        mh = mean.float()
        return torch.stack([mh, (mean - mh.double()).float(), (1.0 / torch.sqrt(var + 1e-5)).float(), torch.zeros(W)])
    st1, st2 = record(a1), record(a2)
    bn = lambda v, st: ((v.double() - st[0].double()) - st[1].double()) * st[2].double() + st[3].double()
    for resid in (None, r):
        want = bn(a1, st1) * bn(a2, st2) + (resid.double() if resid is not None else 0.0)
        got = ops_bf16.merge(a1.to(dev).bfloat16(), st1.to(dev), a2.to(dev).bfloat16(), st2.to(dev),
                             resid.to(dev).bfloat16() if resid is not None else None)
        err = orc.rel_max_err(got.float().cpu(), want)
        assert err < 2.0 ** -8, err                            # one rounding of the result
    mid = bf(torch.randn(s, n, W, generator=gen))
    w = torch.randn(256, s * W, generator=gen) / (s * W) ** 0.5
    b = torch.randn(256, generator=gen)
    cat = torch.cat(list(mid), dim=1).double()
    want = torch.nn.functional.leaky_relu(cat @ w.double().t() + b.double())
    parts = ops.new_partials(256, dev)
    got, npart = ops_bf16.dense_slots(mid.to(dev).bfloat16().contiguous(), w.to(dev), b.to(dev), ops.ACT_LEAKY_RELU, parts)
    err = orc.rel_max_err(got.cpu(), want)
    print(f"bf16 first final Linear (1344 -> 256): {err:.2e}")
    assert err < TOL_BF16
    sm, sq = sums_from(parts, npart, 256)
    gd = got.double().cpu()
    assert float((sm - gd.sum(0)).abs().max()) < 1e-9 * float(gd.abs().sum(0).max())
    assert float((sq - (gd * gd).sum(0)).abs().max()) < 1e-9 * float((gd * gd).sum(0).max())


def test_whole_forward_against_the_oracle_per_layer(dev):
    """The bf16 forward on the real graph: probabilities against the fp64 oracle (the network is chaotic end to end, the
    reference's own fp32 run is 1e-1 off; reported), shapes / range / reproducibility, running statistics updated once."""
    g = graph_tensors(load_labyrinth_graph(), torch.float32, dev)
    x3, adj, attr, col, _ = g
    x = torch.cat([x3, torch.zeros(x3.shape[0], 2, device=dev)], dim=1)[:, [0, 1, 3, 4, 2]].contiguous()   # tile_count 4: Fx = 5
    net, sd = make_net(dev, depth=20)
    net.activation_dtype = torch.bfloat16
    probs, passthrough = net(x=x, adj_e_index=adj, adj_e_features=attr, col_e_idx=col)
    assert probs.shape == (1254, 1) and probs.dtype == torch.float32 and passthrough is attr
    p = probs.cpu().numpy()
    assert np.isfinite(p).all() and (p > 0).all() and (p < 1).all()
    net2, _ = make_net(dev, depth=20)
    net2.activation_dtype = torch.bfloat16
    assert torch.equal(net2(x=x, adj_e_index=adj, adj_e_features=attr, col_e_idx=col)[0], probs)
    assert int(net.brch_1_graph_conv_layers[3].batch_norm.num_batches_tracked) == 1
    sd64 = orc.cast_sd(sd, torch.float64)
    with torch.no_grad():
        want, _ = orc.tilingnn_forward(sd64, x.cpu().double(), adj.cpu(), attr.cpu().double(), col.cpu())
    net32, _ = make_net(dev, depth=20)
    p32 = net32(x=x, adj_e_index=adj, adj_e_features=attr, col_e_idx=col)[0].cpu().numpy()
    gap16, gap32 = np.abs(p - want.numpy()).max(), np.abs(p32 - want.numpy()).max()
    # (reported, not gated: twenty train-mode BatchNorms amplify the 2^-9 storage rounding of every layer to O(1) in single
    #  probabilities -- the reference's own fp32 run is 1e-1 off its fp64 run at width 32 -- the distribution is what survives)
    print(f"end to end, width 64, depth 20: max|p - p_fp64| bf16 storage {gap16:.3e}; fp32 general kernels {gap32:.3e}; "
          f"mean probability bf16 {p.mean():.4f} vs fp64 {want.numpy().mean():.4f}")
    assert abs(p.mean() - want.numpy().mean()) < 5e-2
    # shallow network: out of the chaotic regime
    net3, sd3 = make_net(dev, depth=2)
    net3.activation_dtype = torch.bfloat16
    p3 = net3(x=x, adj_e_index=adj, adj_e_features=attr, col_e_idx=col)[0].cpu()
    with torch.no_grad():
        want3, _ = orc.tilingnn_forward(orc.cast_sd(sd3, torch.float64), x.cpu().double(), adj.cpu(), attr.cpu().double(), col.cpu())
    gap3 = float((p3.double() - want3).abs().max())
    print(f"end to end, depth 2: {gap3:.3e}")
    assert gap3 < 1.5e-1          # measured 4.4e-2: per-op 4e-3 through six more train-mode BatchNorms


@pytest.fixture(scope="module")
def big(dev):
    from tilingnn_amd.synth import make_super_graph
    sg = make_super_graph(100_000, 1_000_000, 1_250_000, tile_count=4, n_edge_types=13, seed=2)
    return sg.to_torch(dev)


def test_config3_size_layers_against_the_oracle(dev, big):
    """BASELINE config 3: 100 000 nodes / 1 000 000 + 1 250 000 edges, tile_count 4, width 64 -- NNConv and GIN teacher
    forced against the fp64 oracle (type-deduplicated NNConv, pinned to the port on the labyrinth graph)."""
    e_nn, e_gin, e_gc, e_cc = check_nnconv_and_gin(dev, big, 100_000, i=2, chunked=True)
    print(f"config 3 (100k / 1M / width 64, bf16 storage): NNConv {e_nn:.2e}, GIN {e_gin:.2e}, GraphConv incl. BN {e_gc:.2e}, "
          f"CollConv incl. BN {e_cc:.2e}")
    assert max(e_nn, e_gin, e_gc, e_cc) < TOL_BF16


def test_config3_forward_runs_and_is_reproducible(dev, big):
    x, adj, attr, col, _ = big
    net, _ = make_net(dev)
    net.activation_dtype = torch.bfloat16
    p1 = net(x=x, adj_e_index=adj, adj_e_features=attr, col_e_idx=col)[0].clone()
    net2, _ = make_net(dev)
    net2.activation_dtype = torch.bfloat16
    p2 = net2(x=x, adj_e_index=adj, adj_e_features=attr, col_e_idx=col)[0]
    assert p1.shape == (100_000, 1) and bool(torch.isfinite(p1).all()) and torch.equal(p1, p2)


def test_config3_new_layout_takes_the_early_init_mlp(dev, big):
    """[r6] A new layout (cache off): the init MLP is queued on the side stream in front of the preparation
    (tgnn_forward_bf16_begin) -- the same bits as the cached layout's forward, and ONE running-statistics update."""
    x, adj, attr, col, _ = big
    ref, _ = make_net(dev)
    ref.activation_dtype = torch.bfloat16
    ref(x=x, adj_e_index=adj, adj_e_features=attr, col_e_idx=col)                       # (fills the layout cache: no begin)
    ref2, _ = make_net(dev)
    ref2.activation_dtype = torch.bfloat16
    want = ref2(x=x, adj_e_index=adj, adj_e_features=attr, col_e_idx=col)[0].clone()    # cached layout: the plain forward
    net, _ = make_net(dev)
    net.activation_dtype = torch.bfloat16
    net.cache_graph = False
    got = net(x=x, adj_e_index=adj, adj_e_features=attr, col_e_idx=col)[0]
    torch.cuda.synchronize()
    assert torch.equal(got, want)
    for k, v in ref2.state_dict().items():
        if k.endswith("num_batches_tracked"):
            assert int(net.state_dict()[k]) == 1 == int(v), k
        elif k.endswith(("running_mean", "running_var")):
            assert torch.equal(net.state_dict()[k], v), k


def compose_forward(net, x, adj, attr, col, graph=None, kernel=None):
    """TilinGNN.forward (TilinGNN.py:51-78) spelled out op by op with the per-op entry points validated above -- the checker
    of the fused library call `tgnn_forward_bf16` (same kernels, same order: bit-identical probabilities).
    graph: the prepared layout (default: prepared here); kernel: the NNConv structure (`ops_bf16.nnconv64`).
    -> (probs, intermediates, the deep copy of `net` whose running statistics this run has updated); intermediates: "mid" the
    bf16 skip buffer [D + 1] x [N, 64], "h2" the collision branch's outputs, "a1" the pre-BatchNorm NNConv outputs, "f1" the
    first final Linear's output (fp32 [N, 256], pre-BatchNorm) and "f1_stat" its BatchNorm record."""
    from tilingnn_amd import ops, ops_bf16
    import copy
    net = copy.deepcopy(net)                                   # running statistics are updated by both runs
    dev, n, D = x.device, int(x.shape[0]), net.network_depth
    if graph is None:
        graph = ops.prepare_graph(n, adj, attr, col)
    P = lambda c: ops.new_partials(c, dev)
    inter = {"h2": [], "a1": []}

    def lin_bn(layer, a, in_stat):
        parts = P(layer.linear.out_features)
        out, npart = ops.dense_act(a, layer.linear.weight, layer.linear.bias, ops.ACT_LEAKY_RELU, in_stat=in_stat, partials=parts)
        return out, ops.bn_finalize(parts, npart, n, layer.batch_norm, update_running=True)
    l0, l1 = net.init_node_feature_trans.mlp
    t0, s0 = lin_bn(l0, x, None)
    a, s1 = lin_bn(l1, t0, s0)
    mid = [ops_bf16.to_bf16(ops.bn_apply(a, s1))]
    h2 = mid[0]
    for i in range(D):
        g1, g2 = net.brch_1_graph_conv_layers[i], net.brch_2_coll_conv_layers[i]
        h2 = ops_bf16.collconv64(h2, graph, g2.ginConv.eps, *g2.ginConv._mlp_params(), g2.batch_norm)
        wtab = ops.edge_weight_table(attr, graph, *g1.nnConv._edge_mlp_params(), W)
        p1 = P(W)
        a1, np1 = ops_bf16.nnconv64(mid[i], graph, wtab, g1.nnConv.root, g1.nnConv.bias, ops.ACT_LEAKY_RELU, p1, kernel=kernel)
        st1 = ops.bn_finalize(p1, np1, n, g1.batch_norm, update_running=True)
        mid.append(ops_bf16.merge(a1, st1, h2, None, mid[i - 2] if i >= 2 else None))
        inter["h2"].append(h2)
        inter["a1"].append(a1)
    f = net.final_mlp[0].mlp
    pf = P(256)
    h, npf = ops_bf16.dense_slots(torch.stack(mid).contiguous(), f[0].linear.weight, f[0].linear.bias, ops.ACT_LEAKY_RELU, pf)
    st = ops.bn_finalize(pf, npf, n, f[0].batch_norm, update_running=True)
    inter.update(mid=mid, f1=h, f1_stat=st)
    for layer in f[1:]:
        h, st = lin_bn(layer, h, st)
    last = net.final_mlp[1].linear
    probs, _ = ops.dense_act(h, last.weight, last.bias, ops.ACT_SIGMOID, in_stat=st)
    return probs, inter, net


@pytest.mark.parametrize("depth", [1, 3])
def test_library_forward_is_the_composition_of_its_ops(dev, depth):
    g = graph_tensors(load_labyrinth_graph(), torch.float32, dev)
    x3, adj, attr, col, _ = g
    x = torch.cat([x3, torch.zeros(x3.shape[0], 2, device=dev)], dim=1)[:, [0, 1, 3, 4, 2]].contiguous()
    net, _ = make_net(dev, depth=depth)
    want, inter, _ = compose_forward(net, x, adj, attr, col)
    assert len(inter["mid"]) == depth + 1 and inter["f1"].shape == (1254, 256)
    net.activation_dtype = torch.bfloat16
    got = net(x=x, adj_e_index=adj, adj_e_features=attr, col_e_idx=col)[0]
    d = float((got - want).abs().max())
    print(f"depth {depth}: max |library - composition| = {d:.3e}")
    assert torch.equal(got, want)

@pytest.mark.gpu
def test_final_linear_rows_kernel(dev):
    """[r4] From 49 152 rows on the first final Linear runs on the rows-per-wave kernel (W as a bf16 operand image, every wave 32 rows x
    all 256 columns): fp64 gate, BatchNorm sums of what was stored, and the same bits as the block-tile kernel row by row (the same
    rows through a call below the threshold)."""
    from tilingnn_amd import ops, ops_bf16
    n, s = 60001, 21
    gen = torch.Generator().manual_seed(6)
    mid = bf(torch.randn(s, n, W, generator=gen)).to(dev).bfloat16().contiguous()
    w = (torch.randn(256, s * W, generator=gen) / (s * W) ** 0.5).to(dev)
    b = torch.randn(256, generator=gen).to(dev)
    parts = ops.new_partials(256, dev)
    got, npart = ops_bf16.dense_slots(mid, w, b, ops.ACT_LEAKY_RELU, parts)
    cat = torch.cat(list(mid.float()), dim=1).double()
    want = torch.nn.functional.leaky_relu(cat @ w.double().t() + b.double())
    assert orc.rel_max_err(got.cpu(), want.cpu()) < TOL_BF16
    sm, sq = sums_from(parts, npart, 256)
    gd = got.double().cpu()
    assert float((sm - gd.sum(0)).abs().max()) < 1e-9 * float(gd.abs().sum(0).max())
    assert float((sq - (gd * gd).sum(0)).abs().max()) < 1e-9 * float((gd * gd).sum(0).max())
    m = 40000
    ref, _ = ops_bf16.dense_slots(mid[:, :m].contiguous(), w, b, ops.ACT_LEAKY_RELU, ops.new_partials(256, dev))
    assert torch.equal(got[:m], ref)

