"""K small layouts' graphs from ONE library call (csrc/graph_prep.hip: graph_prep_small_union_kernel behind
tgnn_graph_prep_small_many; ops.prepare_graphs_small, TilinGNN.forward_many(union=True, union_prep=True), ML_Solver.union_prep).
Every layout's team of blocks runs the solo kernel's body with the solo launch's block count, so every comparison here is
torch.equal / == -- nothing is floating-point arithmetic, there is no tolerance.  The expectation is never the code under test:
it is ops.prepare_graph with ops.SMALL_PREP = False (the separate library calls), computed once per layout."""
import numpy as np
import pytest
import torch

from tests.test_forward_union import _layout, _solver, bunny_crops, net  # noqa: F401  (module-scoped fixtures of the crop tests)
from tests.test_union_area_gpu import ring9  # noqa: F401

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "GPU tests need a GPU"
    return torch.device("cuda:0")


def _same(ref, got):
    assert (got.n_nodes, got.n_adj_edges, got.n_col_edges, got.n_types, got.max_in_degree) == \
        (ref.n_nodes, ref.n_adj_edges, ref.n_col_edges, ref.n_types, ref.max_in_degree)
    n, t = ref.n_nodes, ref.n_types
    na, nc = int(ref.adj_rowptr[n]), int(ref.col_rowptr[n])
    for name, cut in (("adj_rowptr", n + 1), ("adj_src", na), ("adj_eid", na), ("adj_type", na), ("edge_type", ref.n_adj_edges),
                      ("type_rep_edge", t), ("col_rowptr", n + 1), ("col_src", nc), ("col_eid", nc)):
        a, b = getattr(ref, name)[:cut].cpu(), getattr(got, name)[:cut].cpu()
        assert torch.equal(a, b), name
    assert (ref.cols is None) == (got.cols is None)
    if ref.cols is not None:
        ntiles = (n + 15) // 16
        assert torch.equal(ref.cols.tile_col_ptr[:ntiles + 1].cpu(), got.cols.tile_col_ptr[:ntiles + 1].cpu())
        ncol = int(ref.cols.tile_col_ptr[ntiles])
        assert torch.equal(ref.cols.col_meta[:ncol].cpu(), got.cols.col_meta[:ncol].cpu())
        assert torch.equal(ref.cols.col_src[:ncol * 16].cpu(), got.cols.col_src[:ncol * 16].cpu())


def _reference(item):
    """The separate library calls (SMALL_PREP off), whatever the test does afterwards."""
    from tilingnn_amd import ops
    before = ops.SMALL_PREP
    ops.SMALL_PREP = False
    try:
        return ops.prepare_graph(*item)
    finally:
        ops.SMALL_PREP = before


def _synthetic(n, ea, ec, types, seed, dev):
    """(n, adj, attr, col) of the synthetic-layout helper; an odd edge count drops the last edge of the next even one."""
    from tilingnn_amd.synth import make_super_graph
    sg = make_super_graph(n, ea + (ea & 1), ec + (ec & 1), tile_count=2, n_edge_types=types, seed=seed)
    _, adj, attr, col, _ = sg.to_torch(dev)
    return (n, adj[:, :ea].contiguous(), attr[:ea].contiguous(), col[:, :ec].contiguous())


def _teams(items):
    from tilingnn_amd import _lib
    return _lib.graph_prep_small_many_plan([int(i[1].shape[1]) for i in items], [int(i[3].shape[1]) for i in items],
                                           [i[0] for i in items], 240)[0]


@pytest.fixture(scope="module")
def shapes(dev):
    """The smallest layout that reaches every path of the kernel, with its reference.  -> (names, items, refs)"""
    rng = np.random.default_rng(0)
    named = {}
    named["n2"] = (2, torch.tensor([[0], [1]], device=dev), torch.ones(1, 4, device=dev), torch.tensor([[1], [0]], device=dev))
    named["n16"] = _synthetic(16, 64, 48, 13, 1, dev)                       # one 16-row tile
    named["n17"] = _synthetic(17, 68, 50, 13, 2, dev)                       # two tiles, the second of one row
    named["team2"] = _synthetic(300, 2049, 1500, 13, 3, dev)
    named["team5"] = _synthetic(1000, 8193, 6000, 13, 4, dev)               # more than one LDS de-dup share
    named["team16"] = _synthetic(4096, 30000, 32000, 13, 5, dev)
    named["types3"] = _synthetic(170, 1360, 1700, 3, 6, dev)
    # collision self loops (dropped), rows without in-edges, signed zeros in the attribute rows
    n = 40
    adj = torch.tensor(rng.integers(0, 20, size=(2, 150)), device=dev)
    col = torch.tensor(rng.integers(0, n, size=(2, 200)), device=dev)
    col[1, :30] = col[0, :30]
    attr = torch.tensor(rng.integers(0, 3, size=(150, 4)).astype(np.float32), device=dev)
    attr[::7, 0] = -0.0
    named["loops"] = (n, adj, attr, col)
    s = _synthetic(64, 256, 192, 13, 7, dev)
    named["ec0"] = (s[0], s[1], s[2], torch.empty(2, 0, dtype=torch.int64, device=dev))
    named["ea0"] = (s[0], torch.empty(2, 0, dtype=torch.int64, device=dev), torch.empty(0, s[2].shape[1], device=dev), s[3])
    # 4 000 distinct attribute rows: more than the column structure -- and the one-launch numbering -- takes: the fall-back word
    e = 4000
    named["fallback"] = (500, torch.tensor(rng.integers(0, 500, size=(2, e)), device=dev),
                         torch.tensor(rng.normal(size=(e, 3)).astype(np.float32), device=dev),
                         torch.tensor(rng.integers(0, 500, size=(2, 100)), device=dev))
    names, items = list(named), list(named.values())
    teams = dict(zip(names, _teams(items)))
    assert (teams["n2"], teams["team2"], teams["team5"], teams["team16"]) == (1, 2, 5, 16), teams
    refs = [_reference(i) for i in items]
    torch.cuda.synchronize()
    assert refs[names.index("types3")].n_types == 3 and refs[names.index("team5")].n_types == 13
    assert refs[names.index("fallback")].cols is None and refs[names.index("fallback")].n_types == e
    return names, items, refs


def _counts():
    from tilingnn_amd import _lib
    return _lib.graph_prep_small_many_counts()


def _assert_call_equals(shapes, order):
    from tilingnn_amd import ops
    names, items, refs = shapes
    before = _counts()
    got = ops.prepare_graphs_small([items[i] for i in order])
    after = _counts()
    assert len(got) == len(order)
    assert after[1] - before[1] == len(order)                   # (all of them are eligible by size: all ride in the launches)
    for i, g in zip(order, got):
        if names[i] == "fallback":
            assert g is None                                    # (the caller prepares it with ops.prepare_graph)
            continue
        assert g is not None, names[i]
        _same(refs[i], g)
    return after[0] - before[0]


# ------------------------------------------------------------------------------------------------ 1. the preparation alone
def test_every_shape_in_one_call(shapes):
    assert _assert_call_equals(shapes, list(range(len(shapes[0])))) == 1


def test_the_same_list_reversed(shapes):
    assert _assert_call_equals(shapes, list(range(len(shapes[0])))[::-1]) == 1


def test_one_layout_given_twice(shapes):
    names = shapes[0]
    k = names.index("team5")
    assert _assert_call_equals(shapes, [k, names.index("n17"), k]) == 1


def test_calls_in_a_row_and_on_a_second_stream(dev, shapes):
    """Counters are re-armed and the library's buffer sets go round (a ring of four): three calls on one stream, then one on a
    second stream right behind one on the first."""
    names = shapes[0]
    order = [names.index(s) for s in ("team2", "n2", "team16", "loops", "n16")]
    for _ in range(3):
        _assert_call_equals(shapes, order)
    side = torch.cuda.Stream(dev)
    side.wait_stream(torch.cuda.current_stream(dev))
    _assert_call_equals(shapes, order)
    with torch.cuda.stream(side):
        _assert_call_equals(shapes, order[::-1])
    torch.cuda.current_stream(dev).wait_stream(side)
    _assert_call_equals(shapes, order)


def test_twenty_teams_of_sixteen_blocks_take_two_launches(dev):
    """16 blocks each: 15 fit one launch of (256 - 16) blocks, the other 5 ride in the second."""
    from tilingnn_amd import _lib, ops
    distinct = [_synthetic(700, 30722, 2000, 13, 20 + s, dev) for s in range(3)]
    refs = [_reference(i) for i in distinct]
    items = [distinct[j % 3] for j in range(20)]
    assert _teams(items) == [16] * 20
    capacity = torch.cuda.get_device_properties(dev).multi_processor_count - 16
    planned = _lib.graph_prep_small_many_plan([30722] * 20, [2000] * 20, [700] * 20, capacity)[2]
    before = _counts()
    got = ops.prepare_graphs_small(items)
    after = _counts()
    assert (after[0] - before[0], after[1] - before[1]) == (planned, 20)
    assert planned == 2, capacity
    for j, g in enumerate(got):
        _same(refs[j % 3], g)


def test_a_call_of_one_layout_equals_the_solo_call(shapes):
    from tilingnn_amd import ops
    names, items, refs = shapes
    for name in ("n17", "team5"):
        i = names.index(name)
        assert ops.SMALL_PREP
        solo = ops.prepare_graph(*items[i])                     # (tgnn_graph_prep_small)
        got = ops.prepare_graphs_small([items[i]])[0]
        _same(solo, got)
        _same(refs[i], got)


def test_layouts_out_of_the_size_range_are_left_to_the_caller(dev, shapes):
    from tilingnn_amd import ops
    names, items, refs = shapes
    big = _synthetic(4097, 8000, 8000, 13, 9, dev)
    i = names.index("n16")
    before = _counts()
    got = ops.prepare_graphs_small([items[i], big, items[i]])
    after = _counts()
    assert got[1] is None and (after[0] - before[0], after[1] - before[1]) == (1, 2)
    _same(refs[i], got[0])
    _same(refs[i], got[2])
    assert ops.prepare_graphs_small([]) == [] and ops.prepare_graphs_small([big]) == [None]


# ------------------------------------------------------------------------------------------------ 2. index errors
@pytest.mark.parametrize("which", ["adj_e_index", "col_e_idx"])
def test_an_edge_end_out_of_range_names_its_layout_and_leaves_the_others_alone(shapes, which):
    from tilingnn_amd import ops
    names, items, refs = shapes
    a, b = names.index("team2"), names.index("n17")
    n, adj, attr, col = items[names.index("types3")]
    bad_adj, bad_col = adj.clone(), col.clone()
    (bad_adj if which == "adj_e_index" else bad_col)[1, 5] = n   # an edge end equal to n
    call = [items[a], (n, bad_adj, attr, bad_col), items[b]]
    with pytest.raises(IndexError) as exc:
        ops.prepare_graphs_small(call)
    assert "layout 1" in str(exc.value) and which in str(exc.value)
    # the binding below: the word of the middle layout alone is set, its neighbours' outputs are the reference's
    checked = [(i[0], i[1], ops._f32c(i[2], "adj_e_features"), i[3]) for i in call]
    words, pieces = ops._prepare_graphs_small_queue(checked)
    assert [(w[1], w[2]) for w in words] == [(0, 0), (1, 0) if which == "adj_e_index" else (0, 1), (0, 0)]
    for j, i in ((0, a), (2, b)):
        _same(refs[i], ops._small_graph_from_words(checked[j], words[j], pieces[j]))


# ------------------------------------------------------------------------------------------------ 3. forward_many, solve_many
def _forward_pair(net, args):
    """(forward_many(union=True), forward_many(union=True, union_prep=True), preparation launches / layouts of the second)"""
    from tilingnn_amd.graph_networks import _graph_cache
    _graph_cache.clear()
    want = net.forward_many(args, union=True)
    torch.cuda.synchronize()
    _graph_cache.clear()
    before = _counts()
    got = net.forward_many(args, union=True, union_prep=True)
    torch.cuda.synchronize()
    after = _counts()
    assert len(got) == len(want) == len(args)
    for a, b in zip(got, want):
        assert a.shape == b.shape and torch.equal(a, b)
    return after[0] - before[0], after[1] - before[1]


def _crop_args(dev, crops):
    from tilingnn_amd.util.algorithms import PackedLayouts
    pk = PackedLayouts(crops, dev)
    views = [pk.layout(k) for k in range(pk.k)]
    return [(v.node_feature, v.align_edge_index, v.align_edge_features, v.collide_edge_index) for v in views]


def test_the_bunny_crops_are_prepared_by_one_launch_and_cached(dev, net, bunny_crops, monkeypatch):  # noqa: F811
    from tilingnn_amd.graph_networks import _graph_cache
    monkeypatch.setattr(_graph_cache, "_MAX", 64)
    args = _crop_args(dev, bunny_crops[1])
    assert net.cache_graph
    assert _forward_pair(net, args) == (1, len(args))
    before = _counts()
    again = net.forward_many(args, union=True, union_prep=True)   # every graph is in the cache: nothing is prepared
    torch.cuda.synchronize()
    assert _counts() == before
    for a, b in zip(again, net.forward_many(args, union=True)):
        assert torch.equal(a, b)
    # union_prep without union: today's call
    plain = net.forward_many(args, union_prep=True)
    torch.cuda.synchronize()
    assert _counts() == before
    for a, b in zip(plain, again):
        assert torch.equal(a, b)


def test_a_large_layout_between_small_ones(dev, net, monkeypatch):  # noqa: F811
    layouts = [_layout(300, dev, 41), _layout(5000, dev, 42), _layout(520, dev, 43), _layout(33, dev, 44)]
    assert _forward_pair(net, layouts) == (1, 3)
    monkeypatch.setattr(net, "cache_graph", False)
    assert _forward_pair(net, layouts) == (1, 3)


def _assert_same_solves(ms, layouts, seed):
    from tilingnn_amd.util import algorithms as alg
    ms.union_forward = True
    try:
        want = alg.solve_many_by_device_greedy(ms, layouts, seed=seed)
        want_rounds = list(alg.solve_many_by_device_greedy.last_rounds)
        before = _counts()
        ms.union_prep = True
        got = alg.solve_many_by_device_greedy(ms, layouts, seed=seed)
        rounds = list(alg.solve_many_by_device_greedy.last_rounds)
    finally:
        ms.union_forward = ms.union_prep = False
    after = _counts()
    assert after[1] > before[1] and after[0] - before[0] <= max(rounds)       # (one launch per scored round here)
    assert rounds == want_rounds and len(got) == len(want) == len(layouts)
    for k, (g, w) in enumerate(zip(got, want)):
        assert np.array_equal(g[0], w[0]), k                    # selection
        assert g[2] == w[2], k                                  # order
        assert g[1] == w[1], k                                  # score


def test_solve_many_on_the_bunny_crops(net, bunny_crops):  # noqa: F811
    graph, crops = bunny_crops
    _assert_same_solves(_solver(net, graph), crops, 5)


def test_solve_many_on_eight_synthetic_layouts(dev, net):  # noqa: F811
    from tilingnn_amd.util.algorithms import DeviceLayout
    layouts = [DeviceLayout(*_layout(n, dev, 80 + i)) for i, n in enumerate((300, 400, 500, 600, 700, 800, 900, 1000))]
    _assert_same_solves(_solver(net), layouts, 0)
