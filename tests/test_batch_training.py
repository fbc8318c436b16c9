"""Mini-batch training on the GPU: `ops.batch_union` (csrc/batch_union.hip) bit for bit against the numpy oracle of the disjoint
union (tests/batch_oracle.py), one `Trainer.train_batch_step` against the fp64 oracle's step on the oracle-built union and against
the existing `train_step` on the same union, and `Trainer.train_batches` end to end over layout files.

Layouts are cut from tests/golden/complete_graph_small.pkl as tests/test_training_hip.py::test_trainer_loop_on_layout_files cuts
them: 60-140 of its 150 tiles, 3 node features -- 12-byte rows, so the members of a union start unaligned."""
import os

import numpy as np
import pytest
import torch

from oracle import tilingnn_oracle as orc
from tests import batch_oracle
from tests.golden_util import GOLDEN

pytestmark = pytest.mark.gpu
DEV = "cuda:0"


def _small_graph():
    from tilingnn_amd.tiling.tile_graph import TileGraph
    graph = TileGraph(2)
    graph.load_graph_state(os.path.join(GOLDEN, "complete_graph_small.pkl"), sidecar=False)
    return graph


def _cut(graph, rng):
    """(x, adj, attr, col) numpy + the raw tuple of create_brick_layout_from_super_set for one random crop."""
    from tilingnn_amd.util import data_util as du
    tiles = sorted(int(v) for v in rng.choice(150, size=int(rng.integers(60, 140)), replace=False))
    x, ci, cf, ai, af, re_index = du.create_brick_layout_from_super_set(graph, tiles)
    arrays = (np.asarray(x, np.float32), np.asarray(ai, np.int64).reshape(2, -1),
              np.asarray(af, np.float32).reshape(np.asarray(ai).reshape(2, -1).shape[1], -1), np.asarray(ci, np.int64).reshape(2, -1))
    return arrays, (x, ci, cf, ai, af, re_index)


@pytest.fixture(scope="module")
def crops():
    """Four crops as numpy arrays (never modified) and packed on the device."""
    from tilingnn_amd.util.algorithms import DeviceLayout, PackedLayouts
    graph, rng = _small_graph(), np.random.default_rng(0)
    arrays = [_cut(graph, rng)[0] for _ in range(4)]
    assert all(a[0].shape[1] == 3 and a[1].shape[1] and a[3].shape[1] for a in arrays)
    assert any(a[0].shape[0] % 4 for a in arrays[:-1])              # 12-byte rows: some member starts off a 16-byte boundary
    layouts = [DeviceLayout(*(torch.from_numpy(v).to(DEV) for v in a)) for a in arrays]
    return arrays, PackedLayouts(layouts, DEV)


def _equal_to_oracle(got, arrays, ids):
    x, adj, attr, col = batch_oracle.union(arrays, ids)
    for name, g, w in (("x", got.node_feature, x), ("adj", got.align_edge_index, adj), ("attr", got.align_edge_features, attr),
                       ("col", got.collide_edge_index, col)):
        want = torch.from_numpy(w)
        assert g.dtype == want.dtype and tuple(g.shape) == tuple(want.shape), (name, ids, g.shape, want.shape)
        assert torch.equal(g.cpu(), want), (name, ids)


def _upload(arrays, ids):
    from tilingnn_amd.util.algorithms import DeviceLayout
    return DeviceLayout(*(torch.from_numpy(v).to(DEV) for v in batch_oracle.union(arrays, ids)))


def _net(depth, seed, width=32):
    from tilingnn_amd.graph_networks.networks.TilinGNN import TilinGNN
    from tilingnn_amd.weights import make_state_dict
    net = TilinGNN(adj_edge_features_dim=15, network_depth=depth, network_width=width, node_features_dim=3)
    sd = make_state_dict(15, depth, width, 1, 3, seed=seed)
    net.load_state_dict(sd)
    return net.to(DEV).train(), sd


def _trainer(net, tmp_path):
    from tilingnn_amd.solver.ml_solver.trainer import Trainer
    return Trainer(None, None, DEV, net, str(tmp_path))


# ---------------------------------------------------------------------------------------------- 1. the union's bits
def test_union_bits(crops):
    from tilingnn_amd import _lib, ops
    from tilingnn_amd.util.algorithms import DeviceLayout, PackedLayouts
    arrays, packed = crops
    for ids in ([0], [2, 0, 1], [1, 1]):
        first = ops.batch_union(packed, ids)
        _equal_to_oracle(first, arrays, ids)
        again = ops.batch_union(packed, ids)                        # the same bits on every call, in new tensors
        assert again.node_feature.data_ptr() != first.node_feature.data_ptr()
        _equal_to_oracle(again, arrays, ids)

    # five members: one without adjacency edges, one without collision edges, one without nodes
    fe = arrays[0][2].shape[1]
    no_adj = (arrays[2][0], np.zeros((2, 0), np.int64), np.zeros((0, fe), np.float32), arrays[2][3])
    no_col = (arrays[3][0], arrays[3][1], arrays[3][2], np.zeros((2, 0), np.int64))
    nothing = (np.zeros((0, 3), np.float32), np.zeros((2, 0), np.int64), np.zeros((0, fe), np.float32), np.zeros((2, 0), np.int64))
    five = [arrays[0], no_adj, nothing, no_col, arrays[1]]
    pk5 = PackedLayouts([DeviceLayout(*(torch.from_numpy(v).to(DEV) for v in a)) for a in five], DEV)
    for ids in ([0, 1, 2, 3, 4], [2, 4, 1, 3, 0], [3, 2, 2, 1], [2], [1, 3]):
        _equal_to_oracle(ops.batch_union(pk5, ids), five, ids)

    # arguments: checked on the host, before the launch
    with pytest.raises(_lib.TgnnError, match="ids"):
        ops.batch_union(packed, [0, 4])
    with pytest.raises(_lib.TgnnError, match="ids"):
        ops.batch_union(packed, [-1])
    n = [a[0].shape[0] for a in arrays]
    ea = [a[1].shape[1] for a in arrays]
    ec = [a[3].shape[1] for a in arrays]
    good = ([0, n[0], n[0] + n[1]], [0, ea[0], ea[0] + ea[1]], [0, ec[0], ec[0] + ec[1]])
    _equal_to_oracle(ops.batch_union(packed, [0, 1], _offsets=good), arrays, [0, 1])
    for t in range(3):
        bad = [list(o) for o in good]
        bad[t][1], bad[t][2] = bad[t][2], bad[t][1]                 # not monotonic
        with pytest.raises(_lib.TgnnError, match="offset table"):
            ops.batch_union(packed, [0, 1], _offsets=bad)
    with pytest.raises(_lib.TgnnError):
        ops.batch_union(packed, [0, 1], _offsets=([1, n[0] + 1, n[0] + n[1] + 1], good[1], good[2]))     # does not start at 0
    torch.cuda.synchronize()


# ---------------------------------------------------------------------------------------------- 2. semantics of a step
def test_one_step_is_one_batch(crops, tmp_path):
    """A batch of 3 at depth 3: ONE BatchNorm update (statistics over all rows of the union), ONE loss -- the fp64 oracle's
    loss on the oracle-built union, within the gate tests/test_training_width64.py holds a step's loss to."""
    arrays, packed = crops
    ids = [2, 0, 3]
    net, sd = _net(3, 5)
    opt = torch.optim.Adam(net.parameters(), lr=2e-3)
    trainer = _trainer(net, tmp_path)
    bn = net.brch_1_graph_conv_layers[1].batch_norm
    before = int(bn.num_batches_tracked)
    net.autograd = True
    try:
        loss = trainer.train_batch_step(packed, ids, opt)
    finally:
        net.autograd = False
    assert int(bn.num_batches_tracked) == before + 1
    x, adj, attr, col = (torch.from_numpy(v) for v in batch_oracle.union(arrays, ids))
    _, ref_loss, _, _ = orc.training_step_grads(orc.cast_sd(sd, torch.float64), x.double(), adj, attr.double(), col)
    print(f"batch of 3: loss {float(loss):.8f}, fp64 oracle {float(ref_loss):.8f}")
    assert abs(float(loss) - float(ref_loss)) < 1e-4 * float(ref_loss)
    assert net.cache_graph                                          # the bypass of the graph cache ends with the step


# ---------------------------------------------------------------------------------------------- 3. the same step as before
def _rel_gap(a, b):
    a, b = a.double(), b.double()
    return float((a - b).abs().max() / b.abs().max().clamp(min=1e-30))


def test_same_step_as_train_step_on_the_uploaded_union(crops, tmp_path):
    """The same weights, the same batch: gradients after a step through `batch_union` against gradients after the existing
    `train_step` on a DeviceLayout uploaded from the oracle-built union.  The two feed identical arrays to identical kernels, so
    only a run-to-run difference of the existing path itself may show: that is measured first (two runs, each on a freshly
    uploaded union, so that each prepares its graph anew as the union path does).  Zero -> bit equality is required; else each
    parameter's gap may be at most 4 x its measured run-to-run gap.  SGD with lr = 0 keeps the weights where they are."""
    arrays, packed = crops
    ids = [1, 3, 0]
    net, _ = _net(3, 7)
    opt = torch.optim.SGD(net.parameters(), lr=0.0)
    trainer = _trainer(net, tmp_path)
    runs = []
    net.autograd = True
    try:
        for _ in range(2):
            loss = trainer.train_step(_upload(arrays, ids), opt)
            runs.append((loss.clone(), {k: p.grad.clone() for k, p in net.named_parameters()}))
        loss = trainer.train_batch_step(packed, ids, opt)
        got = (loss.clone(), {k: p.grad.clone() for k, p in net.named_parameters()})
    finally:
        net.autograd = False
    own = {k: _rel_gap(runs[0][1][k], runs[1][1][k]) for k in runs[0][1]}
    ours = {k: _rel_gap(got[1][k], runs[1][1][k]) for k in own}
    print(f"run-to-run gap of train_step: loss {abs(float(runs[0][0]) - float(runs[1][0])):.3e}, worst parameter "
          f"{max(own.values()):.3e}; batch_union path against it: loss {abs(float(got[0]) - float(runs[1][0])):.3e}, worst "
          f"parameter {max(ours.values()):.3e}")
    assert all(torch.isfinite(g).all() for g in got[1].values())
    if max(own.values()) == 0.0 and torch.equal(runs[0][0], runs[1][0]):
        assert torch.equal(got[0], runs[1][0])
        for k in own:
            assert torch.equal(got[1][k], runs[1][1][k]), k
    else:
        for k in own:
            assert ours[k] <= 4.0 * own[k], (k, ours[k], own[k])


# ---------------------------------------------------------------------------------------------- 4. the loop
def test_train_batches_on_layout_files(tmp_path):
    from tilingnn_amd.graph_networks import _graph_cache
    from tilingnn_amd.solver.ml_solver.ml_solver import ML_Solver
    from tilingnn_amd.util import data_util as du
    graph, rng = _small_graph(), np.random.default_rng(0)
    for split, count in (("train", 5), ("test", 2)):
        os.makedirs(tmp_path / split, exist_ok=True)
        for i in range(count):
            _, (x, ci, cf, ai, af, re_index) = _cut(graph, rng)
            du.write_brick_layout_data(f"layout_{i}.pkl", re_index, node_features=x, collide_edge_index=ci,
                                       collide_edge_features=cf, align_edge_index=ai, align_edge_features=af,
                                       prefix=str(tmp_path / split / "raw"))
    net, _ = _net(3, 5)
    solver = ML_Solver(None, DEV, graph, net, num_prob_maps=1)
    opt = torch.optim.Adam(net.parameters(), lr=2e-3)
    trainer = _trainer(net, tmp_path)
    cached = len(_graph_cache._entries)
    history = trainer.train_batches(solver, opt, batch_size=2, training_epoch=4, save_model_per_epoch=2, shuffle_seed=1,
                                    log=lambda *_: None)
    print("history:", history)
    assert len(history) == 4 and all(np.isfinite(h).all() for h in history)
    assert history[-1][0] < history[0][0]
    assert len(_graph_cache._entries) <= cached + 5 + 2             # no union graph stays behind: at most the data set's own
    saved = sorted(os.listdir(tmp_path / "model"))
    models = [f for f in saved if f.startswith("model_0_")]
    optims = [f for f in saved if f.startswith("optimizer_0_")]
    assert models and optims
    assert not net.autograd and net.cache_graph
    sd = torch.load(str(tmp_path / "model" / models[0]), map_location="cpu")
    fresh, _ = _net(3, 6)
    ML_Solver(None, DEV, graph, fresh, num_prob_maps=1).load_saved_network(str(tmp_path / "model" / models[0]))
    for k, v in fresh.state_dict().items():
        assert torch.equal(v.cpu(), sd[k]), k
    torch.optim.Adam(fresh.parameters(), lr=2e-3).load_state_dict(torch.load(str(tmp_path / "model" / optims[0]), map_location="cpu"))
    with pytest.raises(NotImplementedError):
        trainer.train(solver, opt, batch_size=4)


# ---------------------------------------------------------------------------------------------- 5. width 64
def test_one_step_width64(crops, tmp_path):
    _, packed = crops
    net, _ = _net(3, 4, width=64)
    opt = torch.optim.Adam(net.parameters(), lr=2e-3)
    trainer = _trainer(net, tmp_path)
    net.autograd = True
    try:
        loss = trainer.train_batch_step(packed, [3, 1], opt)
    finally:
        net.autograd = False
    assert np.isfinite(float(loss))
    for k, p in net.named_parameters():
        assert p.grad is not None and torch.isfinite(p.grad).all(), k
