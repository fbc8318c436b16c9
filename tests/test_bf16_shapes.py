"""The bf16-storage path (BASELINE config 3, csrc/bf16_path.hip) at the shapes its other tests do not reach: the case table of
tests/bf16_cases.py (rows below the 8-way split, ragged tiles, rows without in-edges, every remainder of the gather loop, hubs
with hundreds of in-edges, no collision edges at all, the block cap), bare graphs, both NNConv structures, the switches at
49 152 rows, and forwards that are refused.

Gates: TOL_BF16 = 2^-7 of the output's max-norm against fp64 on the same bf16-rounded inputs (tests/test_bf16_path.py states
it; tests/test_bf16_cases_host.py shows that the reference's own storage roundings use at most 0.6 of it on these inputs),
the existing 1e-9 gate of the BatchNorm partial sums, 2^-8 for the merge, bit-equality between the library's forward and the
composition of its ops, and bounds computed at run time from a reference (fp32 torch against fp64; the composition against
fp64).  Every measured value is printed."""
import copy

import pytest
import torch

from oracle import tilingnn_oracle as orc
from tests import bf16_cases as bc
from tests.test_bf16_path import TOL_BF16, W, bf, compose_forward, make_net, sums_from

pytestmark = pytest.mark.gpu
P2 = "brch_2_coll_conv_layers.1"
leaky = torch.nn.functional.leaky_relu


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available()
    return torch.device("cuda:0")


@pytest.fixture(scope="module")
def net3(dev):
    """make_state_dict(15, 3, 64, 1, 5, seed=0): the weights of the host model."""
    net, sd = make_net(dev, depth=3)
    return net, orc.cast_sd(sd, torch.float64), orc.cast_sd(sd, torch.float32)


def on(dev, *ts):
    return tuple(t.to(dev) for t in ts)


def check_sums(parts, npart, got, f=W):
    """The partial rows are [npart][2 f]: sums and sums of squares of the STORED values, to fp64 accuracy."""
    s, q = sums_from(parts, npart, f)
    gd = got.double().cpu()
    assert float((s - gd.sum(0)).abs().max()) <= 1e-9 * float(gd.abs().sum(0).max())
    assert float((q - (gd * gd).sum(0)).abs().max()) <= 1e-9 * float((gd * gd).sum(0).max())


def gin_blocks(n, dev):
    """gin64_mlp_blocks (csrc/bf16_path.hip): 128 rows per block, all CUs but 32 (never fewer than a quarter), whole eights."""
    from tilingnn_amd import ops
    cus = torch.cuda.get_device_properties(dev).multi_processor_count
    cap = cus - 32 if cus - 32 > cus // 4 else max(cus // 4, 1)
    nb = min(max((n + 127) // 128, 1), ops.BN_MAX_PARTIALS, cap)
    return nb & ~7 if nb >= 8 else nb


_seam_cache = {}


def seam_case(dev, case):
    """One layout of the table, its prepared graph and the teacher-forced bf16 input (the host model's)."""
    from tilingnn_amd import ops
    if case not in _seam_cache:
        n = case[0]
        x, adj, attr, col = bc.case_graph(case)
        h = bf(torch.randn(n, W, generator=torch.Generator().manual_seed(7)))
        graph = ops.prepare_graph(n, *on(dev, adj, attr, col))
        _seam_cache[case] = (n, col, h, graph)
    return _seam_cache[case]


# ------------------------------------------------------------------------------------------------ 1. GIN / CollConv seams
@pytest.mark.parametrize("case", bc.CASES, ids=bc.case_id)
def test_gin_seam_over_the_case_table(dev, net3, case):
    from tilingnn_amd import ops, ops_bf16
    net, sd64, _ = net3
    n, col, h, graph = seam_case(dev, case)
    l2 = net.brch_2_coll_conv_layers[1]
    hb = h.to(dev).to(torch.bfloat16)
    with torch.no_grad():
        want = orc.gin_conv(h.double(), col, sd64, P2)
    for act, ref in ((ops.ACT_NONE, want), (ops.ACT_LEAKY_RELU, leaky(want))):
        parts = ops.new_partials(W, dev)
        got, npart = ops_bf16.gin64(hb, graph, l2.ginConv.eps, *l2.ginConv._mlp_params(), act=act, partials=parts)
        err = orc.rel_max_err(got.float().cpu(), ref)
        print(f"{bc.case_id(case)} gin64 act {act}: {err:.2e}, {npart} partial rows")
        assert got.shape == (n, W) and err < TOL_BF16
        assert npart == gin_blocks(n, dev)
        check_sums(parts, npart, got)
        if n > bc.ISOLATED_ROW + 1:
            # a row without in-edges, closed form: the MLP of (1 + eps) h[5]
            r = bc.ISOLATED_ROW
            assert int(bc.col_in_degree(n, col)[r]) == 0
            with torch.no_grad():
                row = orc.mlp((1.0 + sd64[P2 + ".ginConv.eps"]) * h.double()[r:r + 1], sd64, P2 + ".ginConv.nn", 3, orc.sigmoid, bn=False)
            row = leaky(row) if act == ops.ACT_LEAKY_RELU else row
            e_row = orc.rel_max_err(got[r:r + 1].float().cpu(), row)
            print(f"{bc.case_id(case)} gin64 act {act}: isolated row {e_row:.2e} of its own max")
            assert e_row < TOL_BF16


@pytest.mark.parametrize("case", [c for c in bc.CASES if c[0] in (17, 130, 1030)], ids=bc.case_id)
def test_gin_folds_the_previous_batchnorm_with_an_activation(dev, net3, case):
    """in_stat AND LeakyReLU in one call (the record built as test_bf16_path.test_gin_folds_the_previous_batchnorm builds it)."""
    from tilingnn_amd import ops, ops_bf16
    net, sd64, _ = net3
    n, col, a, graph = seam_case(dev, case)
    l2 = net.brch_2_coll_conv_layers[1]
    gen = torch.Generator().manual_seed(3)
    gamma, beta = torch.rand(W, generator=gen) + 0.5, torch.randn(W, generator=gen)
    mean, var = a.double().mean(0), a.double().var(0, unbiased=False)
    mh = mean.float()
    stat = torch.stack([mh, (mean - mh.double()).float(), (gamma.double() / torch.sqrt(var + 1e-5)).float(), beta])
    xin = ((a.double() - mean) / torch.sqrt(var + 1e-5)) * gamma.double() + beta.double()
    with torch.no_grad():
        want = leaky(orc.gin_conv(xin, col, sd64, P2))
    parts = ops.new_partials(W, dev)
    got, npart = ops_bf16.gin64(a.to(dev).to(torch.bfloat16), graph, l2.ginConv.eps, *l2.ginConv._mlp_params(),
                                act=ops.ACT_LEAKY_RELU, in_stat=stat.to(dev), partials=parts)
    err = orc.rel_max_err(got.float().cpu(), want)
    print(f"{bc.case_id(case)} gin64 with folded BatchNorm and LeakyReLU: {err:.2e}")
    assert err < TOL_BF16
    check_sums(parts, npart, got)


@pytest.mark.parametrize("case", bc.CASES, ids=bc.case_id)
def test_collconv_seam_over_the_case_table(dev, net3, case):
    """CollConv incl. its train-mode BatchNorm (n = 2 included: two rows are a batch), and its running-statistics update."""
    from tilingnn_amd import ops_bf16
    net, sd64, sd32 = net3
    n, col, h, graph = seam_case(dev, case)
    l2 = net.brch_2_coll_conv_layers[1]
    hb = h.to(dev).to(torch.bfloat16)
    up64, up32 = copy.deepcopy(sd64), copy.deepcopy(sd32)
    with torch.no_grad():
        want = orc.batch_norm_train(leaky(orc.gin_conv(h.double(), col, up64, P2)), up64, P2 + ".batch_norm", update_running=True)
        orc.batch_norm_train(leaky(orc.gin_conv(h.float(), col, up32, P2)), up32, P2 + ".batch_norm", update_running=True)
    bn = copy.deepcopy(l2.batch_norm)
    got = ops_bf16.collconv64(hb, graph, l2.ginConv.eps, *l2.ginConv._mlp_params(), bn, update_running=False)
    err = orc.rel_max_err(got.float().cpu(), want)
    assert int(bn.num_batches_tracked) == 0 and torch.equal(bn.running_mean, l2.batch_norm.running_mean)
    got2 = ops_bf16.collconv64(hb, graph, l2.ginConv.eps, *l2.ginConv._mlp_params(), bn, update_running=True)
    assert torch.equal(got, got2)
    rm64, rv64 = up64[P2 + ".batch_norm.running_mean"], up64[P2 + ".batch_norm.running_var"]
    e_rm = orc.rel_max_err(bn.running_mean.cpu(), rm64)
    e_rv = orc.rel_max_err(bn.running_var.cpu(), rv64)
    e32 = orc.rel_max_err(up32[P2 + ".batch_norm.running_var"], rv64)
    print(f"{bc.case_id(case)} collconv64: {err:.2e}; running_mean {e_rm:.2e}; running_var {e_rv:.2e} against fp32 torch's {e32:.2e}")
    assert err < TOL_BF16
    assert int(bn.num_batches_tracked) == 1
    assert e_rm < TOL_BF16
    assert e_rv <= max(8 * e32, 1e-6)


# ------------------------------------------------------------------------------------------------ 2. NNConv, both kernels
def nnconv_inputs(dev, n, n_types, seed=2):
    gen = torch.Generator().manual_seed(seed)
    h = torch.randn(n, W, generator=gen).to(dev).to(torch.bfloat16)
    wtab = torch.rand(max(n_types, 1), W, W, generator=gen).to(dev)[:n_types]
    root = (torch.randn(W, W, generator=gen) * 0.3).to(dev)
    bias = torch.randn(W, generator=gen).to(dev)
    return h, wtab, root, bias


def fp64_nnconv64(h, adj, edge_type, wtab, root, bias, n, act_leaky):
    """oracle/tilingnn_oracle.py: nnconv_mean in fp64 on the device, on the weights as the path rounds them (once, to bf16)."""
    wb, rb = wtab.to(torch.bfloat16).double(), root.to(torch.bfloat16).double()
    src, dst = adj[0], adj[1]
    agg = torch.zeros(n, W, dtype=torch.float64, device=h.device)
    if src.numel():
        agg.index_add_(0, dst, torch.einsum("ek,eko->eo", h.double()[src], wb[edge_type]))
    deg = torch.zeros(n, dtype=torch.float64, device=h.device).index_add_(0, dst, torch.ones_like(dst, dtype=torch.float64))
    out = agg / deg.clamp(min=1).unsqueeze(1) + h.double() @ rb + bias.double()
    return torch.where(out >= 0, out, out * 0.01) if act_leaky else out


# (case of the table, edge types; 0 = no adjacency edge at all: the root term plus the bias)
NN_CASES = [((2, 1, 0), 13), ((9, 2, 0), 13), ((17, 3, 0), 16), ((17, 3, 0), 0), ((130, 8, 0), 16), ((1030, 8, 300), 13),
            ((29_000, 7, 1500), 16), ((29_000, 7, 1500), 0)]


@pytest.mark.parametrize("case,n_types", NN_CASES, ids=[f"{bc.case_id(c)}-T{t}" for c, t in NN_CASES])
@pytest.mark.parametrize("kernel", ["eg", "cols"])
def test_nnconv64_on_both_structures(dev, case, n_types, kernel):
    from tilingnn_amd import ops, ops_bf16
    n = case[0]
    _, adj, attr, _ = bc.case_graph(case, n_types=max(n_types, 1))
    if n_types == 0:
        adj, attr = adj[:, :0], attr[:0]
    adj, attr = on(dev, adj, attr)
    ea = int(adj.shape[1])
    g = ops.prepare_graph(n, adj, attr, torch.zeros(2, 0, dtype=torch.int64, device=dev), groups=(kernel == "eg"))
    assert g.n_types == (int(torch.unique(attr, dim=0).shape[0]) if ea else 0) == min(n_types, ea)
    h, wtab, root, bias = nnconv_inputs(dev, n, g.n_types)
    # the reference's edge types come from the attribute rows themselves (torch.unique), not from the preparation under test:
    # the library's type t is matched to its class by ONE edge that carries it (type_rep_edge), every other edge is independent
    edge_type = torch.zeros(0, dtype=torch.int64, device=dev)
    if ea:
        _, inv = torch.unique(attr, dim=0, return_inverse=True)
        cls_of_type = inv[g.type_rep_edge[:g.n_types].long()]
        assert sorted(cls_of_type.tolist()) == list(range(g.n_types))
        edge_type = torch.empty_like(cls_of_type).scatter_(0, cls_of_type, torch.arange(g.n_types, device=dev))[inv]
    for act in (ops.ACT_NONE, ops.ACT_LEAKY_RELU):
        want = fp64_nnconv64(h, adj, edge_type, wtab, root, bias, n, act == ops.ACT_LEAKY_RELU)
        parts = ops.new_partials(W, dev)
        out, npart = ops_bf16.nnconv64(h, g, wtab, root, bias, act, parts, kernel=kernel)
        err = orc.rel_max_err(out.float().cpu(), want.cpu())
        print(f"{bc.case_id(case)} T {g.n_types} nnconv64 {kernel} act {act}: {err:.2e}")
        assert out.shape == (n, W) and bool(torch.isfinite(out.float()).all()) and err < TOL_BF16
        check_sums(parts, npart, out)
        if n_types == 0:
            bare = h.double() @ root.to(torch.bfloat16).double() + bias.double()
            assert orc.rel_max_err(want.cpu(), (torch.where(bare >= 0, bare, bare * 0.01) if act == ops.ACT_LEAKY_RELU else bare).cpu()) < 1e-12
        if case[2] and n_types:
            r = bc.HUB_ROW                                    # hundreds of in-edges in ONE row, against the row's own max
            e_hub = orc.rel_max_err(out[r:r + 1].float().cpu(), want[r:r + 1].cpu())
            print(f"{bc.case_id(case)} T {g.n_types} nnconv64 {kernel} act {act}: hub row {e_hub:.2e} of its own max")
            assert int((adj[1] == r).sum()) >= case[2] and e_hub < TOL_BF16


@pytest.mark.parametrize("kernel", ["eg", "cols"])
def test_nnconv64_refuses_seventeen_types(dev, kernel):
    """17 edge types: both structures are BUILT (the width-32 kernels take up to tgnn_nnconv_cols_max_types() = 22 types), and
    both width-64 entry points refuse them before their first launch -- 18 weight images of 8 KB and the waves' staging do not
    fit 160 KB of LDS (tgnn_nnconv64_bf16_fwd / _eg_fwd: TGNN_ERR_UNSUPPORTED) -- which `check` turns into a Python exception."""
    from tilingnn_amd import _lib, ops, ops_bf16
    n = 130
    _, adj, attr, _ = bc.case_graph((n, 8, 0), n_types=17)
    adj, attr = on(dev, adj, attr)
    g = ops.prepare_graph(n, adj, attr, torch.zeros(2, 0, dtype=torch.int64, device=dev), groups=(kernel == "eg"))
    assert g.n_types == 17 == ops_bf16.max_types() + 1
    assert (ops.graph_groups(g) if kernel == "eg" else ops.graph_columns(g)) is not None
    h, wtab, root, bias = nnconv_inputs(dev, n, 17)
    with pytest.raises(_lib.TgnnError, match="17 edge types"):
        ops_bf16.nnconv64(h, g, wtab, root, bias, ops.ACT_NONE, ops.new_partials(W, dev), kernel=kernel)


# ------------------------------------------------------------------------------------------------ 3. element-wise, first final Linear
@pytest.mark.parametrize("count", [1, 255, 257, 64 * 4099])
def test_to_bf16_is_round_to_nearest_even(dev, count):
    from tilingnn_amd import ops_bf16
    gen = torch.Generator().manual_seed(count)
    v = torch.randn(count, generator=gen) * torch.exp(4 * torch.randn(count, generator=gen))
    ties = v[::7].to(torch.bfloat16).float().view(torch.int32) | 0x8000   # exactly half way between two bf16 neighbours
    v[::7] = ties.view(torch.float32)
    v = v.to(dev)
    assert torch.equal(ops_bf16.to_bf16(v), v.to(torch.bfloat16))


@pytest.mark.parametrize("n", [2, 37, 4099])
@pytest.mark.parametrize("with_resid", [False, True])
def test_merge_as_the_forward_calls_it(dev, n, with_resid):
    """stat2 = None: a2 is the collision branch's BatchNorm OUTPUT.  One rounding of the result: 2^-8."""
    from tilingnn_amd import ops_bf16
    gen = torch.Generator().manual_seed(5 + n)
    a1, a2, r = (bf(torch.randn(n, W, generator=gen)) for _ in range(3))
    mean, var = a1.double().mean(0), a1.double().var(0, unbiased=False)
    mh = mean.float()
    st1 = torch.stack([mh, (mean - mh.double()).float(), (1.0 / torch.sqrt(var + 1e-5)).float(), torch.randn(W, generator=gen)])
    want = (((a1.double() - st1[0].double()) - st1[1].double()) * st1[2].double() + st1[3].double()) * a2.double()
    if with_resid:
        want = want + r.double()
    got = ops_bf16.merge(a1.to(dev).bfloat16(), st1.to(dev), a2.to(dev).bfloat16(), None, r.to(dev).bfloat16() if with_resid else None)
    err = orc.rel_max_err(got.float().cpu(), want)
    print(f"merge n {n} resid {with_resid}: {err:.2e}")
    assert got.shape == (n, W) and err < 2.0 ** -8


def dense_case(dev, n, s, m, seed):
    from tilingnn_amd import ops, ops_bf16
    gen = torch.Generator().manual_seed(seed)
    mid = bf(torch.randn(s, n, W, generator=gen)).to(dev).bfloat16().contiguous()
    w = (torch.randn(m, s * W, generator=gen) / (s * W) ** 0.5).to(dev)
    b = torch.randn(m, generator=gen).to(dev)
    parts = ops.new_partials(m, dev)
    got, npart = ops_bf16.dense_slots(mid, w, b, ops.ACT_LEAKY_RELU, parts)
    cat = torch.cat(list(mid.float()), dim=1).double()
    want = leaky(cat @ w.double().t() + b.double())
    err = orc.rel_max_err(got.cpu(), want.cpu())
    print(f"dense_slots n {n} slots {s} out {m}: {err:.2e}, {npart} partial rows")
    assert got.shape == (n, m) and npart == (n + 127) // 128 and err < TOL_BF16
    check_sums(parts, npart, got, m)                                       # (rows of [2 out_dim])


@pytest.mark.parametrize("s", [2, 4, 21])
@pytest.mark.parametrize("n", [2, 127, 128, 129, 300])
def test_first_final_linear_at_ragged_row_counts(dev, n, s):
    dense_case(dev, n, s, 256, 100 * s + n)


@pytest.mark.parametrize("m", [1, 100, 255])
def test_first_final_linear_at_other_widths(dev, m):
    """tgnn_dense_bf16_slots_fwd takes out_dim 1 .. 256: the block-tile kernel clamps the weight rows it stages and masks the
    columns it stores (dense_bf16_slots_kernel); the partial rows are [2 out_dim] wide."""
    dense_case(dev, 300, 4, m, 7 + m)


# ------------------------------------------------------------------------------------------------ 4. forward == composition
def bf16_net(dev, depth, cache):
    net, sd = make_net(dev, depth=depth)
    net.activation_dtype = torch.bfloat16
    net.cache_graph = cache
    return net, sd


def assert_same_forward(got, want, net_lib, net_comp, what):
    d = float((got - want).abs().max())
    print(f"{what}: max |library - composition| = {d:.3e}")
    assert torch.equal(got, want), what
    assert bool(torch.isfinite(got).all()) and float(got.min()) > 0.0 and float(got.max()) < 1.0, what
    a, b = net_lib.state_dict(), net_comp.state_dict()
    assert a.keys() == b.keys()
    for k, v in a.items():
        if k.endswith("num_batches_tracked"):
            assert int(v) == 1 == int(b[k]), (what, k)
        else:
            assert torch.equal(v, b[k]), (what, k)


FWD_CASES = [((2, 1, 0), ""), ((17, 3, 0), ""), ((130, 8, 0), ""), ((3000, 1, 0), ""),
             ((130, 8, 0), "no_adj"), ((130, 8, 0), "no_col"), ((130, 8, 0), "neither")]


def fwd_layout(dev, case, empty):
    x, adj, attr, col = bc.case_graph(case)
    if empty in ("no_adj", "neither"):
        adj, attr = adj[:, :0], attr[:0]
    if empty in ("no_col", "neither"):
        col = col[:, :0]
    return on(dev, x, adj.contiguous(), attr.contiguous(), col.contiguous())


@pytest.mark.parametrize("case,empty", FWD_CASES, ids=[bc.case_id(c) + (("-" + e) if e else "") for c, e in FWD_CASES])
@pytest.mark.parametrize("structure", ["groups", "columns"])
def test_forward_is_its_composition_over_the_case_table(dev, request, case, empty, structure):
    """tgnn_forward_bf16 at depth 3 against the op-by-op composition (sections 1 - 3 tie every op to the oracle), bit for bit,
    running statistics included -- as a NEW layout (the init MLP queued in front of the preparation) and as a cached one, over
    edge groups and over type columns.  A new layout's structure is the preparation's choice: edge groups for layouts of the
    general schedule (the `general_schedule` fixture puts every size there), type columns with ops.GROUPS off -- asserted."""
    from tilingnn_amd import ops
    from tilingnn_amd._lib import lib
    from tilingnn_amd.graph_networks import _graph_cache
    n = case[0]
    cid = bc.case_id(case) + (("-" + empty) if empty else "")
    if structure == "groups":
        request.getfixturevalue("general_schedule")
    x, adj, attr, col = fwd_layout(dev, case, empty)
    args = dict(x=x, adj_e_index=adj, adj_e_features=attr, col_e_idx=col)
    prev_eg = lib.tgnn_set_nnconv_eg(0) if structure == "columns" else lib.tgnn_set_nnconv_eg(-1)
    keep_groups = ops.GROUPS
    try:
        if structure == "columns":
            ops.GROUPS = False
            graph = ops.prepare_graph(n, adj, attr, col)
            assert graph.cols is not None and graph.groups is None
            kernel = "cols"
        else:
            graph = ops.prepare_graph(n, adj, attr, col, groups=True)
            assert graph.groups is not None
            kernel = "eg"
        ref, _ = bf16_net(dev, 3, False)
        want, inter, net_comp = compose_forward(ref, x, adj, attr, col, graph=graph, kernel=kernel)
        assert len(inter["mid"]) == 4 and all(m.shape == (n, W) for m in inter["mid"])
        # a cached layout: the plain forward on the structure under test
        _graph_cache.clear()
        _graph_cache.put_full(n, adj, attr, col, graph)
        net, _ = bf16_net(dev, 3, True)
        assert_same_forward(net(**args)[0], want, net, net_comp, f"{cid} over {structure}, cached layout")
        _graph_cache.clear()
        # a new layout: the init MLP runs beside the preparation, which chooses the structure (the one under test: asserted)
        default = ops.prepare_graph(n, adj, attr, col)
        assert (default.groups is not None) == (structure == "groups") and (default.cols is not None) == (structure == "columns")
        net, _ = bf16_net(dev, 3, False)
        assert_same_forward(net(**args)[0], want, net, net_comp, f"{cid} over {structure}, new layout")
    finally:
        ops.GROUPS = keep_groups
        lib.tgnn_set_nnconv_eg(prev_eg)
        _graph_cache.clear()


def test_forward_is_its_composition_without_the_early_init_mlp(dev, monkeypatch):
    """TGNN_BF16_BEGIN=0: a new layout's forward queues its init MLP itself."""
    monkeypatch.setenv("TGNN_BF16_BEGIN", "0")
    x, adj, attr, col = fwd_layout(dev, (130, 8, 0), "")
    ref, _ = bf16_net(dev, 3, False)
    want, _, net_comp = compose_forward(ref, x, adj, attr, col)
    net, _ = bf16_net(dev, 3, False)
    got = net(x=x, adj_e_index=adj, adj_e_features=attr, col_e_idx=col)[0]
    assert_same_forward(got, want, net, net_comp, "TGNN_BF16_BEGIN=0")


# ------------------------------------------------------------------------------------------------ 5. past 49 152 rows
def big_layout(dev, n):
    return on(dev, *bc.random_graph(n, 4, 4, 13, seed=49, hub=0))


def test_forward_below_the_row_switches_is_its_composition(dev):
    """49 151 rows: the block-tile kernels run in the library's forward and in the composition."""
    x, adj, attr, col = big_layout(dev, 49_151)
    ref, _ = bf16_net(dev, 1, False)
    want, _, net_comp = compose_forward(ref, x, adj, attr, col)
    net, _ = bf16_net(dev, 1, False)
    got = net(x=x, adj_e_index=adj, adj_e_features=attr, col_e_idx=col)[0]
    assert_same_forward(got, want, net, net_comp, "49 151 rows")


def test_forward_past_the_row_switches_against_fp64(dev):
    """49 153 rows, depth 1: from 49 152 rows on the first final Linear runs on the rows-per-wave kernel (in the library and in
    the composition: the same kernel on the same bits) and the LIBRARY alone puts the final MLP's Linears 1 .. 3 on the fp16-pair
    kernels with bounds built from BatchNorm parameters (tail_f16).  Reference: the rest of the network in fp64 from the
    composition's f1 (three Linear + LeakyReLU + train-mode BatchNorm layers and the sigmoid head).  g_comp = max|p_composition -
    p_ref|, g_lib = max|p_library - p_ref|: both sides are fp32-accurate kernels of the same layers, so g_lib <= max(4 g_comp,
    1e-5 = the project's per-op TOL), and g_comp < 2e-4 = TOL_ILL of BatchNorm-amplified seams.  That the library did take the
    fp16-pair tail shows in its bits: they differ from the composition's.
    Measured on an MI355X: g_comp = 6.864e-07, g_lib = 5.256e-07 (profiles/bf16_shapes_errors.txt)."""
    n = 49_153
    x, adj, attr, col = big_layout(dev, n)
    ref, sd = bf16_net(dev, 1, False)
    p_comp, inter, _ = compose_forward(ref, x, adj, attr, col)
    net, _ = bf16_net(dev, 1, False)
    p_lib = net(x=x, adj_e_index=adj, adj_e_features=attr, col_e_idx=col)[0]
    sd64 = {k: v.to(dev) for k, v in orc.cast_sd(sd, torch.float64).items()}
    with torch.no_grad():
        v = orc.batch_norm_train(inter["f1"].double(), sd64, "final_mlp.0.mlp.0.batch_norm")
        for i in (1, 2, 3):
            v = orc.linear_trans(v, sd64, f"final_mlp.0.mlp.{i}", orc.leaky_relu, bn=True)
        p_ref = orc.linear_trans(v, sd64, "final_mlp.1", orc.sigmoid, bn=False)
    g_comp = float((p_comp.double() - p_ref).abs().max())
    g_lib = float((p_lib.double() - p_ref).abs().max())
    print(f"49 153 rows, final MLP behind f1 against fp64: composition {g_comp:.3e}, library (fp16-pair tail) {g_lib:.3e}")
    assert p_lib.shape == (n, 1) and bool(torch.isfinite(p_lib).all())
    assert not torch.equal(p_lib, p_comp), "the library's forward did not take the fp16-pair tail (tail_f16)"
    assert g_comp < 2e-4
    assert g_lib <= max(4 * g_comp, 1e-5)


# ------------------------------------------------------------------------------------------------ 6. refused forwards
N_REFUSED = 300


def refused(fn, exc):
    """True if fn() raises exc.  The exception -- and with its traceback the refused call's frame and the workspace tensor in it --
    is gone when this returns, as after an `except` clause in a caller's loop: the allocator hands the workspace's address out again."""
    try:
        fn()
    except exc:
        return True
    return False


def layout_a(dev):
    return on(dev, *bc.random_graph(N_REFUSED, 4, 4, 13, seed=61))


def refused_layout(dev, how):
    """("types17": 17 edge types -- the check behind the preparation; "col_index": a collision index out of range -- the
    preparation itself raises) -> (layout, the exception)."""
    if how == "types17":
        return on(dev, *bc.random_graph(N_REFUSED, 4, 4, 17, seed=62)), ValueError
    x, adj, attr, col = bc.random_graph(N_REFUSED, 4, 4, 13, seed=63)
    col[0, 11] = N_REFUSED + 5
    return on(dev, x, adj, attr, col), IndexError


def sd_clone(net):
    return {k: v.clone() for k, v in net.state_dict().items()}


REFUSALS = [("types17", True), ("col_index", True), ("types17", False), ("col_index", False)]
REFUSAL_IDS = [f"{h}-{'cached' if c else 'uncached'}" for h, c in REFUSALS]


class LibSpy:
    """ops_bf16's library handle with the workspace addresses of tgnn_forward_bf16_begin / tgnn_forward_bf16 written down."""

    def __init__(self, lib):
        self._lib, self.begin_ws, self.forward_ws = lib, [], []

    def __getattr__(self, name):
        fn = getattr(self._lib, name)
        at = {"tgnn_forward_bf16_begin": (5, self.begin_ws), "tgnn_forward_bf16": (7, self.forward_ws)}.get(name)
        if at is None:
            return fn

        def call(*args):
            at[1].append(args[at[0]].value)
            return fn(*args)
        return call


def need(cond, what):
    """A precondition of the refusal tests -- not an AssertionError: the strict xfail of gate (b) must not be met by it."""
    if not cond:
        raise RuntimeError(what)


def run_refusal(dev, how, cache_on_refusal, monkeypatch):
    """1. forward A with x0 (fills the layout cache); 2. forward B, refused (cache_on_refusal = False: as a network with
    cache_graph off meets it -- the init MLP and its running-statistics update are queued BEFORE the preparation that
    refuses); 3. forward A with x1.  -> (step 3's probabilities, state dict before / after step 2, a fresh network's step 3).
    The stale record can only be met when step 3's workspace lies where the refused call's lay: asserted, so that gate (a)
    cannot pass for want of the coincidence.  With the cache on, the preparation comes first and `begin` is never queued:
    those variants pin that (and are otherwise plain)."""
    from tilingnn_amd import ops_bf16
    spy = LibSpy(ops_bf16.lib)
    monkeypatch.setattr(ops_bf16, "lib", spy)
    xa, adj, attr, col = layout_a(dev)
    x1 = torch.randn(N_REFUSED, bc.FX, generator=torch.Generator().manual_seed(64)).to(dev)
    (xb, adjb, attrb, colb), exc = refused_layout(dev, how)
    a0 = dict(x=xa, adj_e_index=adj, adj_e_features=attr, col_e_idx=col)
    a1 = dict(a0, x=x1)
    net, _ = bf16_net(dev, 3, True)
    net(**a0)
    before, after = sd_clone(net), sd_clone(net)
    net.cache_graph = cache_on_refusal
    need(refused(lambda: net(x=xb, adj_e_index=adjb, adj_e_features=attrb, col_e_idx=colb), exc), "step 2 was not refused")
    net.cache_graph = True
    need(len(spy.forward_ws) == 1 and len(spy.begin_ws) == (0 if cache_on_refusal else 1), "begin / forward calls of steps 1 and 2")
    for k, v in net.state_dict().items():
        after[k].copy_(v)              # (into tensors that exist: nothing is allocated between the refusal and step 3's workspace)
    p3 = net(**a1)[0].clone()
    need(len(spy.forward_ws) == 2 and len(spy.begin_ws) == (0 if cache_on_refusal else 1), "begin / forward calls of step 3")
    if not cache_on_refusal:
        need(spy.forward_ws[1] == spy.begin_ws[0], "step 3's workspace does not lie at the refused call's address")
    fresh, _ = bf16_net(dev, 3, True)
    fresh(**a0)
    want = fresh(**a1)[0].clone()
    return p3, before, after, want


@pytest.mark.parametrize("how,cache_on_refusal", REFUSALS, ids=REFUSAL_IDS)
def test_refused_forward_leaves_no_pending_init_mlp(dev, monkeypatch, how, cache_on_refusal):
    """(a) The forward after a refused one scores ITS x.  A refused new layout had its init MLP queued already
    (tgnn_forward_bf16_begin): the library remembers (workspace, node count), Python frees the workspace, the next cached layout
    of the same node count gets the same address from the allocator -- without tgnn_forward_bf16_drop on the error paths of
    ops_bf16.forward it would skip its own init MLP and score what the refused call left there.  Observed on an MI355X with
    the drop taken out (the parent commit's behaviour): both uncached variants fail, step 3 returns other probabilities."""
    p3, _, _, want = run_refusal(dev, how, cache_on_refusal, monkeypatch)
    assert torch.equal(p3, want)


XFAIL_B = pytest.mark.xfail(strict=True, raises=AssertionError, reason="a refused NEW layout (cache_graph off) has queued its init MLP, with the running-"
                            "statistics update of the two init BatchNorms, in front of the preparation that refuses it: the update "
                            "stays (DESIGN.md, config 3: known limits).  Undoing it costs the successful path a copy or a launch.")


@pytest.mark.parametrize("how,cache_on_refusal", [pytest.param(h, c, marks=() if c else XFAIL_B) for h, c in REFUSALS], ids=REFUSAL_IDS)
def test_refused_forward_leaves_the_running_statistics(dev, monkeypatch, how, cache_on_refusal):
    """(b) all-or-nothing: the state dict behind a refused forward is the state dict in front of it."""
    _, before, after, _ = run_refusal(dev, how, cache_on_refusal, monkeypatch)
    assert before.keys() == after.keys()
    for k, v in before.items():
        assert torch.equal(v, after[k]), k


def test_refusals_in_front_of_the_first_launch(dev):
    """Width 32 and eval mode are refused by ops_bf16.forward's first lines (ValueError); the next ordinary forward returns the
    bits of a fresh network."""
    from tilingnn_amd import TilinGNN
    from tilingnn_amd.weights import make_state_dict
    xa, adj, attr, col = layout_a(dev)
    a0 = dict(x=xa, adj_e_index=adj, adj_e_features=attr, col_e_idx=col)
    fresh, _ = bf16_net(dev, 3, True)
    want = fresh(**a0)[0].clone()
    narrow = TilinGNN(adj_edge_features_dim=bc.FE, network_depth=3, network_width=32, node_features_dim=bc.FX)
    narrow.load_state_dict(make_state_dict(bc.FE, 3, 32, 1, bc.FX, seed=0), strict=True)
    narrow = narrow.to(dev).train()
    narrow.activation_dtype = torch.bfloat16
    assert refused(lambda: narrow(**a0), ValueError)
    net, _ = bf16_net(dev, 3, True)
    before = sd_clone(net)
    net.eval()
    assert refused(lambda: net(**a0), ValueError)
    net.train()
    after = sd_clone(net)
    assert all(torch.equal(v, after[k]) for k, v in before.items())
    assert torch.equal(net(**a0)[0], want)
    for cache in (True, False):
        other, _ = bf16_net(dev, 3, cache)
        assert torch.equal(other(**a0)[0], want)
