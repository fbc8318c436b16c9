"""K small layouts inside ONE persistent kernel launch (csrc/forward_small.hip: forward_layers_small_union_kernel behind
tgnn_forward_union; TilinGNN.forward_many(union=True), ML_Solver.union_forward = True for solve_many).  Every layout's team of blocks
performs the arithmetic of the solo kernel -- the same block count, sum orders and formulas -- so every comparison here is
torch.equal / == against the layout's solo forward, computed first, never a tolerance."""
import os

import numpy as np
import pytest
import torch

from tests.golden_util import graph_tensors, load_labyrinth_graph
from tests.test_hip_parity import make_net
from tests.test_small_layout import small_limit
from tests.test_union_area_gpu import CROP_KW, SIL, ring9  # noqa: F401  (ring9: the module-scoped fixture of the crop tests)

pytestmark = pytest.mark.gpu
FE = 15


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "GPU tests need a GPU"
    return torch.device("cuda:0")


@pytest.fixture(scope="module")
def net(dev):
    return make_net(dev, depth=20)[0]


def _layout(n, dev, seed, types=13, adj=None, col=None):
    """A synthetic layout of `types` edge types whose attribute rows are padded to the network's 15 columns."""
    from tilingnn_amd.synth import make_super_graph
    if adj is None:
        adj, col = (8 * n, 10 * n) if n >= 100 else (4 * n, 3 * n)
    sg = make_super_graph(n, adj, col, tile_count=2, n_edge_types=types, seed=seed)
    x, a, attr, c, _ = sg.to_torch(dev)
    if attr.shape[1] < FE:
        attr = torch.cat([attr, torch.zeros(attr.shape[0], FE - attr.shape[1], device=dev)], 1).contiguous()
    return (x, a, attr, c)


def _solo(net, layouts):
    out = [net(x=l[0], adj_e_index=l[1], adj_e_features=l[2], col_e_idx=l[3])[0].clone() for l in layouts]
    torch.cuda.synchronize()
    return out


def _counts():
    from tilingnn_amd import _lib
    return _lib.forward_union_counts()


def _assert_union_equals(net, layouts, solo, order, in_union=None):
    """forward_many(union=True) over layouts[order] against the solo outputs; `in_union`: how many of them the union must score."""
    before = _counts()
    outs = net.forward_many([layouts[i] for i in order], union=True)
    torch.cuda.synchronize()
    after = _counts()
    assert len(outs) == len(order)
    for i, o in zip(order, outs):
        assert o.shape == solo[i].shape and torch.equal(o, solo[i]), (order, i)
    if in_union is not None:
        assert after[1] - before[1] == in_union, (before, after)
    return after[0] - before[0]


# ------------------------------------------------------------------------------------------------ 1. the smallest teams
@pytest.fixture(scope="module")
def tiny(dev, net):
    """2 nodes (BatchNorm's minimum: one adjacency pair, no collision edge), 16 (exactly one tile), 17 (a one-row second tile), 33."""
    layouts = [_layout(2, dev, 1, adj=2, col=0), _layout(16, dev, 2), _layout(17, dev, 3), _layout(33, dev, 4)]
    return layouts, _solo(net, layouts)


@pytest.mark.parametrize("which", [0, 1, 2, 3])
def test_one_tiny_layout_per_call(net, tiny, which):
    layouts, solo = tiny
    assert int(layouts[which][0].shape[0]) == (2, 16, 17, 33)[which]
    launches = _assert_union_equals(net, layouts, solo, [which], in_union=1)
    assert launches == 1


def test_the_four_tiny_layouts_in_one_launch(net, tiny):
    layouts, solo = tiny
    assert _assert_union_equals(net, layouts, solo, [0, 1, 2, 3], in_union=4) == 1


# ------------------------------------------------------------------------------------------------ 2. unequal teams in one launch
@pytest.fixture(scope="module")
def mixed(dev, net):
    """17, 170, 640, the labyrinth's 1 254 and 48 nodes; 3 and 13 edge types mixed, so that the launch's dynamic LDS (the largest
    type count's) exceeds what the 3-type teams use themselves."""
    g = load_labyrinth_graph()
    layouts = [_layout(17, dev, 11, types=3), _layout(170, dev, 12, types=13), _layout(640, dev, 13, types=3),
               tuple(graph_tensors(g, torch.float32, dev)[:4]), _layout(48, dev, 14, types=13)]
    from tilingnn_amd import ops
    types = [ops.prepare_graph(int(l[0].shape[0]), l[1], l[2], l[3]).n_types for l in layouts]
    assert types[0] == 3 and types[2] == 3 and types[1] == 13 and types[4] >= 10, types
    return layouts, _solo(net, layouts)


@pytest.mark.parametrize("order", [[0, 1, 2, 3, 4], [4, 3, 2, 1, 0], [4, 3, 2, 1, 0, 0]])
def test_teams_of_different_size_and_type_count(net, mixed, order):
    layouts, solo = mixed
    for _ in range(3):                                          # (counters and partial rows are re-armed by every call)
        assert _assert_union_equals(net, layouts, solo, order, in_union=len(order)) == 1


# ------------------------------------------------------------------------------------------------ 3. more blocks than fit
def test_more_blocks_than_one_launch_may_carry(dev, net):
    capacity = torch.cuda.get_device_properties(dev).multi_processor_count - 16
    if capacity >= 320:
        pytest.skip(f"{capacity} blocks fit one launch on this device: eight layouts of 40 blocks do not overflow it")
    layouts = [_layout(640, dev, 30 + k) for k in range(8)]
    solo = _solo(net, layouts)
    launches = _assert_union_equals(net, layouts, solo, list(range(8)), in_union=8)
    assert launches >= 2


# ------------------------------------------------------------------------------------------------ 4. mixed eligibility
def test_a_large_layout_between_small_ones_and_the_limit_switched_off(dev, net):
    from tilingnn_amd import _lib
    layouts = [_layout(300, dev, 41), _layout(5000, dev, 42), _layout(520, dev, 43), _layout(33, dev, 44)]
    solo = _solo(net, layouts)
    paths = _lib.forward_path_counts()
    _assert_union_equals(net, layouts, solo, [0, 1, 2, 3], in_union=3)
    after = _lib.forward_path_counts()
    assert after[1] - paths[1] == 3 and sum(after) - sum(paths) == 4       # (a union layout counts as a small-path forward)
    with small_limit(0):
        general = _solo(net, layouts)
        assert _assert_union_equals(net, layouts, general, [0, 1, 2, 3], in_union=0) == 0
    _assert_union_equals(net, layouts, solo, [3, 2, 0], in_union=3)


# ------------------------------------------------------------------------------------------------ 5. BatchNorm buffers, eval mode
def test_running_statistics_stay_untouched_and_eval_mode_takes_the_lanes(dev, mixed):
    layouts, _ = mixed
    net = make_net(dev, depth=20)[0]
    solo = _solo(net, layouts)                                  # (train mode: this updates the running statistics, like any forward)
    buffers = {k: v.clone() for k, v in net.state_dict().items() if "running_" in k or "num_batches_tracked" in k}
    assert len(buffers) >= 3 * (2 * 20 + 6)
    _assert_union_equals(net, layouts, solo, [0, 1, 2, 3, 4], in_union=5)
    for k, v in net.state_dict().items():
        if k in buffers:
            assert torch.equal(v, buffers[k]), k
    net.eval()
    try:
        want = net.forward_many(layouts)
        torch.cuda.synchronize()
        before = _counts()
        got = net.forward_many(layouts, union=True)
        torch.cuda.synchronize()
        assert _counts() == before                              # (running statistics: nothing enters the union)
        for a, b in zip(got, want):
            assert torch.equal(a, b)
    finally:
        net.train()


# ------------------------------------------------------------------------------------------------ 6. / 7. the crops, the solves
@pytest.fixture(scope="module")
def bunny_crops(ring9):  # noqa: F811
    from tilingnn_amd.tiling import tile_factory as tf
    from tilingnn_amd.util.shape_processor import load_polygons
    ext, holes = load_polygons(os.path.join(SIL, "bunny.txt"))
    crops = tf.crop_multiple_layouts_from_contour(ext, holes, ring9.graph, device="cuda:0", coverage=True, **CROP_KW)
    assert 12 <= len(crops) < 24
    return ring9.graph, [c[0] for c in crops]


def test_the_bunny_crops_side_by_side_and_in_one_launch(dev, net, bunny_crops):
    from tilingnn_amd.util.algorithms import PackedLayouts
    _, crops = bunny_crops
    pk = PackedLayouts(crops, dev)
    views = [pk.layout(k) for k in range(pk.k)]
    args = [(v.node_feature, v.align_edge_index, v.align_edge_features, v.collide_edge_index) for v in views]
    want = net.forward_many(args)
    torch.cuda.synchronize()
    before = _counts()
    got = net.forward_many(args, union=True)
    torch.cuda.synchronize()
    after = _counts()
    assert after[1] - before[1] == len(args) and after[0] - before[0] == 1
    for a, b in zip(got, want):
        assert torch.equal(a, b)


def _solver(net, graph=None):
    from tilingnn_amd.solver.ml_solver.ml_solver import ML_Solver
    return ML_Solver(None, torch.device("cuda:0"), graph, net, num_prob_maps=1)


def _assert_same_solves(ms, layouts, seed):
    from tilingnn_amd.util import algorithms as alg
    want = alg.solve_many_by_device_greedy(ms, layouts, seed=seed)
    want_rounds = list(alg.solve_many_by_device_greedy.last_rounds)
    before = _counts()
    ms.union_forward = True
    try:
        got = alg.solve_many_by_device_greedy(ms, layouts, seed=seed)
    finally:
        ms.union_forward = False
    rounds = list(alg.solve_many_by_device_greedy.last_rounds)
    assert _counts()[1] > before[1]
    assert rounds == want_rounds and len(got) == len(want) == len(layouts)
    for k, (g, w) in enumerate(zip(got, want)):
        assert np.array_equal(g[0], w[0]), k
        assert g[2] == w[2], k
        assert g[1] == w[1], k
    return rounds


def test_solve_many_with_the_union_forward_on_the_bunny_crops(net, bunny_crops):
    graph, crops = bunny_crops
    ms = _solver(net, graph)
    _assert_same_solves(ms, crops, 5)
    ms.union_forward = True
    outs = ms.solve_many(crops[:4], seed=3)
    ms.union_forward = False
    for (a, sa), (b, sb) in zip(outs, ms.solve_many(crops[:4], seed=3)):
        assert np.array_equal(a.predict, b.predict) and sa == sb and a.predict_order == b.predict_order
        assert np.array_equal(a.predict_probs.view(np.int32), b.predict_probs.view(np.int32))


@pytest.mark.parametrize("sizes", [(300, 520, 900, 1300, 1700, 2100, 2600, 3000), (400, 6000, 900)])
def test_solve_many_with_the_union_forward_on_synthetic_layouts(dev, net, sizes):
    """Eight layouts of 300 ... 3 000 nodes; and a set with a 6 000-node layout, so that the mid-size path joins the loop."""
    from tilingnn_amd.util.algorithms import DeviceLayout
    layouts = [DeviceLayout(*_layout(n, dev, 60 + i)) for i, n in enumerate(sizes)]
    rounds = _assert_same_solves(_solver(net), layouts, 0)
    assert len(set(rounds)) > 1
