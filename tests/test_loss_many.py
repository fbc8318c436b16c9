"""The unsupervised loss of K layouts in one call (`tgnn_unsupervised_loss_many`, csrc/greedy_many.hip) and what is built on it:
`Losses.unsupervised_losses_many`, `cal_avg_loss_many`, `Trainer.train(_batches)(eval_group=)`, the best-map pick of
`solve_many_by_device_greedy`.  The batched call is THE SAME COMPUTATION per layout as `Losses.unsupervised_losses`, so it is
held to equality (torch.equal) against that call, and -- like that call in tests/test_hip_parity.py -- to 1e-6 (max-norm
relative) against fp64, here the numpy restatement of tests/loss_many_oracle.py.

Layouts are cut from tests/golden/complete_graph_small.pkl as tests/test_batch_training.py cuts them, or synthetic: random edge
ends in [0, n), adjacency lengths and areas in (0, 1], probabilities in (0.01, 0.99) -- the reference's sign asserts hold."""
import copy
import os

import numpy as np
import pytest
import torch

from tests import loss_many_oracle as lmo
from tests.test_batch_training import _cut, _net, _small_graph

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
GATE = 1e-6                                                         # tests/test_hip_parity.py: the loss against the fp64 oracle


def _dev(arrays):
    from tilingnn_amd.util.algorithms import DeviceLayout
    return DeviceLayout(*(torch.from_numpy(np.ascontiguousarray(v)).to(DEV) for v in arrays))


def _probs(rng, n, m):
    return rng.uniform(0.01, 0.99, size=(n, m)).astype(np.float32)


def _synthetic(rng, n, ea, ec, fe=2):
    x = rng.uniform(0.0, 1.0, size=(n, 3)).astype(np.float32)
    x[:, -1] = 1.0 - x[:, -1]                                       # (0, 1]
    attr = (1.0 - rng.uniform(0.0, 1.0, size=(ea, fe))).astype(np.float32)
    return (x, rng.integers(0, max(n, 1), size=(2, ea), dtype=np.int64), attr, rng.integers(0, max(n, 1), size=(2, ec), dtype=np.int64))


def _solo(layout, probs):
    from tilingnn_amd.solver.ml_solver.losses import Losses
    return Losses.unsupervised_losses(probs, layout.node_feature, layout.collide_edge_index, layout.align_edge_index,
                                      layout.align_edge_features)


def _rel(got, want):
    got, want = np.asarray(got, np.float64), np.asarray(want, np.float64)
    return float(np.abs(got - want).max() / max(np.abs(want).max(), 1e-30))


def _check_members(losses, terms, err, layouts, probs, arrays=None, probs_h=None, skip=(), label=""):
    """Rows of every member equal the solo call's; with numpy inputs given, within GATE of the fp64 restatement."""
    assert not err.cpu().numpy().any(), (label, err.cpu().tolist())
    worst = 0.0
    for k, (lay, p) in enumerate(zip(layouts, probs)):
        if k in skip:
            assert torch.isnan(losses[k]).all() and torch.isnan(terms[k]).all(), (label, k)
            continue
        want_l, want_t = _solo(lay, p)
        assert torch.equal(losses[k], want_l), (label, k, losses[k].tolist(), want_l.tolist())
        assert torch.equal(terms[k], want_t), (label, k)
        if arrays is not None:
            worst = max(worst, _rel(losses[k].cpu().numpy(), lmo.loss_terms(arrays[k], probs_h[k])[0]))
    if arrays is not None:
        print(f"{label}: worst max-norm relative error against fp64 {worst:.2e}")
        assert worst < GATE, (label, worst)


@pytest.fixture(scope="module")
def crops():
    """Four crops (numpy, never modified) of 60-140 tiles."""
    graph, rng = _small_graph(), np.random.default_rng(0)
    return [_cut(graph, rng)[0] for _ in range(4)]


def _five(crops):
    """K = 5: ordinary, no adjacency edges, no nodes, no collision edges, ordinary."""
    fe = crops[0][2].shape[1]
    no_adj = (crops[2][0], np.zeros((2, 0), np.int64), np.zeros((0, fe), np.float32), crops[2][3])
    no_col = (crops[3][0], crops[3][1], crops[3][2], np.zeros((2, 0), np.int64))
    nothing = (np.zeros((0, 3), np.float32), np.zeros((2, 0), np.int64), np.zeros((0, fe), np.float32), np.zeros((2, 0), np.int64))
    return [crops[0], no_adj, nothing, no_col, crops[1]]


# ---------------------------------------------------------------------------------------------- 1. equality with the solo call
def test_five_members_equal_their_solo_calls(crops):
    from tilingnn_amd.solver.ml_solver.losses import Losses
    from tilingnn_amd.util.algorithms import PackedLayouts
    arrays = _five(crops)
    layouts = [_dev(a) for a in arrays]
    pk = PackedLayouts(layouts, DEV)
    rng = np.random.default_rng(1)
    # M = 3, rows of 3 floats
    probs_h = [_probs(rng, a[0].shape[0], 3) for a in arrays]
    probs = [torch.from_numpy(p).to(DEV) for p in probs_h]
    losses, terms, err = Losses.unsupervised_losses_many(probs, pk)
    assert losses.shape == (5, 3) and terms.shape == (5, 3, 3) and err.shape == (5,)
    assert losses.dtype == terms.dtype == torch.float64 and err.dtype == torch.int32 and losses.is_cuda
    _check_members(losses, terms, err, layouts, probs, arrays, probs_h, skip={2}, label="M = 3")
    # M = 1: column 2 of [n, 4] tensors, rows of 4 floats
    wide_h = [_probs(rng, a[0].shape[0], 4) for a in arrays]
    wide = [torch.from_numpy(p).to(DEV) for p in wide_h]
    cols = [w[:, 2:3] for w in wide]
    assert cols[0].stride() == (4, 1)
    losses, terms, err = Losses.unsupervised_losses_many(cols, pk)
    assert losses.shape == (5, 1)
    _check_members(losses, terms, err, layouts, [c.contiguous() for c in cols], arrays, [w[:, 2:3] for w in wide_h], skip={2},
                   label="M = 1 of 4")
    # a contiguous group of a larger packed set, into rows of the caller's buffer
    buf, l_all, t_all, e_all = Losses.many_outputs(5, 3, DEV)
    got = Losses.unsupervised_losses_many(probs[3:], pk, first=3, count=2, out=(l_all[3:], t_all[3:], e_all[3:]))
    assert got[0].data_ptr() == l_all[3:].data_ptr()
    assert torch.isnan(l_all[:3]).all() and torch.isnan(t_all[:3]).all()
    for k in (3, 4):
        want_l, want_t = _solo(layouts[k], probs[k])
        assert torch.equal(l_all[k], want_l) and torch.equal(t_all[k], want_t)
    l_h, t_h, e_h = Losses.read_back_many(buf, 5, 3)
    assert np.array_equal(l_h[3:], l_all[3:].cpu().numpy()) and np.array_equal(t_h[3:], t_all[3:].cpu().numpy()) and not e_h.any()
    res = Losses.results_many(l_h, t_h, e_h, present=[False, False, False, True, True])
    assert res[:3] == [None] * 3 and float(res[4][0]) == float(l_all[4].min().to(torch.float32))


# ---------------------------------------------------------------------------------------------- 2. block-count boundaries
def test_block_count_boundaries_in_one_call():
    from tilingnn_amd.solver.ml_solver.losses import Losses
    from tilingnn_amd.util.algorithms import PackedLayouts
    rng = np.random.default_rng(2)
    # (n, ea, ec): the largest set the collision / adjacency / node / collision set; 1, 2, 3 and (clamped) 512 blocks
    shapes = [(300, 500, 1024), (300, 1025, 200), (2049, 50, 40), (300, 1000, 524289)]
    assert [lmo.loss_blocks(n, ec, ea) for n, ea, ec in shapes] == [1, 2, 3, 512]
    arrays = [_synthetic(rng, *s) for s in shapes]
    layouts = [_dev(a) for a in arrays]
    pk = PackedLayouts(layouts, DEV)
    probs_h = [_probs(rng, a[0].shape[0], 2) for a in arrays]
    probs = [torch.from_numpy(p).to(DEV) for p in probs_h]
    losses, terms, err = Losses.unsupervised_losses_many(probs, pk)
    _check_members(losses, terms, err, layouts, probs, arrays, probs_h, label="block boundaries")


# ---------------------------------------------------------------------------------------------- 3. many small layouts
def test_three_hundred_layouts_with_an_active_mask():
    from tilingnn_amd.solver.ml_solver.losses import Losses
    from tilingnn_amd.util.algorithms import PackedLayouts
    rng = np.random.default_rng(3)
    K = 300                                                         # past one 256-wide pass of the plan's scan
    arrays = [_synthetic(rng, int(rng.integers(2, 41)), int(rng.integers(0, 61)), int(rng.integers(0, 61))) for _ in range(K)]
    layouts = [_dev(a) for a in arrays]
    pk = PackedLayouts(layouts, DEV)
    probs = [torch.from_numpy(_probs(rng, a[0].shape[0], 2)).to(DEV) for a in arrays]
    active = rng.uniform(size=K) < 0.6
    assert active[:256].any() and active[256:].any() and not active.all()
    losses = torch.full((K, 2), 7.0, dtype=torch.float64, device=DEV)
    terms = torch.full((K, 2, 3), 7.0, dtype=torch.float64, device=DEV)
    err = torch.full((K,), 5, dtype=torch.int32, device=DEV)
    Losses.unsupervised_losses_many(probs, pk, active=active.tolist(), out=(losses, terms, err))
    assert not err.cpu().numpy().any()                              # cleared by the call
    on = torch.from_numpy(np.flatnonzero(active)).to(DEV)
    off = torch.from_numpy(np.flatnonzero(~active)).to(DEV)
    assert (losses[off] == 7.0).all() and (terms[off] == 7.0).all()          # inactive rows: untouched
    want = [_solo(layouts[k], probs[k]) for k in np.flatnonzero(active)]
    same_l = (losses[on] == torch.stack([w[0] for w in want])).all(dim=1)
    same_t = (terms[on] == torch.stack([w[1] for w in want])).all(dim=2).all(dim=1)
    assert same_l.all() and same_t.all(), np.flatnonzero(active)[~(same_l & same_t).cpu().numpy()].tolist()


# ---------------------------------------------------------------------------------------------- 4. compacted sub-layouts
def test_counts_select_the_compacted_sub_layouts(crops):
    from tests.test_solve_many import Packed
    from tilingnn_amd.solver.ml_solver.losses import Losses
    arrays = [crops[0], crops[1], crops[2], crops[3], _five(crops)[3]]
    layouts = [_dev(a) for a in arrays]
    st = Packed(layouts)
    pk = st.pk
    rng = np.random.default_rng(4)
    masks = [(rng.uniform(size=a[0].shape[0]) < 0.6).astype(np.int32) for a in arrays]
    masks[2][:] = 0                                                 # every node dead: a sub-layout without nodes
    alive = torch.from_numpy(np.concatenate(masks)).to(DEV)
    assert st.compact(alive) == 0
    counts_h = st.counts.cpu().numpy()
    assert not st.err.cpu().numpy().any() and counts_h[2].tolist() == [0, 0, 0]
    assert all(0 < counts_h[k, 0] < arrays[k][0].shape[0] for k in (0, 1, 3, 4))
    probs_h = [_probs(rng, int(counts_h[k, 0]), 3) for k in range(5)]
    probs = [torch.from_numpy(p).to(DEV) for p in probs_h]
    losses, terms, err = Losses.unsupervised_losses_many(probs, pk, buffers=(st.x_out, st.adj_out, st.attr_out, st.col_out),
                                                         counts=st.counts)
    subs = [st.sub(k) for k in range(5)]
    subs_h = [lmo.sub_layout(a, m) for a, m in zip(arrays, masks)]
    for k in (0, 1, 3, 4):                                          # the views are what the oracle's sub-layout says
        assert np.array_equal(subs[k].align_edge_index.cpu().numpy(), subs_h[k][1])
        assert np.array_equal(subs[k].collide_edge_index.cpu().numpy(), subs_h[k][3])
    _check_members(losses, terms, err, subs, probs, subs_h, probs_h, skip={2}, label="counts")


# ---------------------------------------------------------------------------------------------- 5. faults stay local
def test_a_fault_stays_with_its_layout(crops):
    from tilingnn_amd.solver.ml_solver.losses import Losses
    from tilingnn_amd.util.algorithms import PackedLayouts
    rng = np.random.default_rng(5)
    arrays = [tuple(np.array(v) for v in a) for a in crops]
    n1 = arrays[1][0].shape[0]
    arrays[1][1][1, 7] = n1                                         # an adjacency end one past the layout: node 0 of the next one
    layouts = [_dev(a) for a in arrays]
    pk = PackedLayouts(layouts, DEV)
    # the probabilities are views of one pool, so that even a wrong row count would stay inside an allocation
    pool = torch.from_numpy(_probs(rng, pk.n + 64, 2)).to(DEV)
    probs = [pool[pk.node_ptr_h[k]:pk.node_ptr_h[k + 1]] for k in range(4)]

    def check(got, bad, untouched_by_the_fault, label):
        losses, terms, err = got
        torch.cuda.synchronize()
        err_h = err.cpu().numpy()
        for k in bad:
            assert err_h[k] == 1 and torch.isnan(losses[k]).all(), (label, k)
        for k in untouched_by_the_fault:
            want_l, want_t = _solo(layouts[k], probs[k].contiguous())
            assert err_h[k] == 0 and torch.equal(losses[k], want_l) and torch.equal(terms[k], want_t), (label, k)
        return losses.cpu().numpy(), terms.cpu().numpy(), err_h

    host = check(Losses.unsupervised_losses_many(probs, pk), [1], [0, 2, 3], "edge end")
    with pytest.raises(IndexError, match="layout 1"):
        Losses.results_many(*host)
    assert Losses.results_many(*host, present=[True, False, True, True])[1] is None
    # offset tables that are not monotonic: the layouts whose range is broken get NaN and their error word, nothing faults
    good = PackedLayouts([_dev(a) for a in crops], DEV)
    probs_ok = probs
    layouts = [good.layout(k) for k in range(4)]
    swapped = copy.copy(good)
    table = list(good.adj_ptr_h)
    table[1], table[2] = table[2], table[1]                         # layout 1: adj_ptr[1] > adj_ptr[2]; 0 and 2 read a neighbour's edges
    swapped.adj_ptr = torch.tensor(table, dtype=torch.int64, device=DEV)
    losses, _, err_h = check(Losses.unsupervised_losses_many(probs_ok, swapped), [1], [3], "adjacency table")
    for k in (0, 2):                                                # a wrong but in-range table: a number, or NaN with the error word
        assert np.isnan(losses[k]).all() == bool(err_h[k]), k
    beyond = copy.copy(good)
    table = list(good.node_ptr_h)
    table[2] = good.n + 7                                           # past the packed nodes: breaks layouts 1 and 2
    beyond.node_ptr = torch.tensor(table, dtype=torch.int64, device=DEV)
    check(Losses.unsupervised_losses_many(probs_ok, beyond), [1, 2], [0, 3], "node table")
    neg = copy.copy(good)
    table = list(good.col_ptr_h)
    table[0] = -3
    neg.col_ptr = torch.tensor(table, dtype=torch.int64, device=DEV)
    check(Losses.unsupervised_losses_many(probs_ok, neg), [0], [1, 2, 3], "collision table")


# ---------------------------------------------------------------------------------------------- 6. evaluating a split
@pytest.fixture(scope="module")
def split(tmp_path_factory):
    """Seven layout files (one without collision edges), a depth-3 network, and `cal_avg_loss` over them in train and eval mode."""
    from tilingnn_amd.solver.ml_solver.trainer import LayoutDataset, cal_avg_loss
    from tilingnn_amd.util import data_util as du
    root = tmp_path_factory.mktemp("split")
    graph, rng = _small_graph(), np.random.default_rng(6)
    os.makedirs(root / "test", exist_ok=True)
    for i in range(7):
        _, (x, ci, cf, ai, af, re_index) = _cut(graph, rng)
        if i == 4:
            ci, cf = np.zeros((2, 0), np.int64), np.zeros((0, np.asarray(cf).shape[-1]), np.float32)
        du.write_brick_layout_data(f"layout_{i}.pkl", re_index, node_features=x, collide_edge_index=ci, collide_edge_features=cf,
                                   align_edge_index=ai, align_edge_features=af, prefix=str(root / "test" / "raw"))
    data = LayoutDataset(str(root / "test"), DEV)
    assert len(data) == 7 and data[4].collide_edge_index.numel() == 0
    net, sd = _net(3, 9)
    want_train = cal_avg_loss(net, data)
    net.eval()
    want_eval = cal_avg_loss(net, data)
    net.train()
    print(f"cal_avg_loss: train mode {want_train!r}, eval mode {want_eval!r}")
    assert np.isfinite(want_train) and np.isfinite(want_eval)
    return net, data, want_train, want_eval


@pytest.mark.parametrize("union", [False, True])
@pytest.mark.parametrize("group", [1, 3, 32])
def test_split_evaluation_is_cal_avg_loss(split, monkeypatch, group, union):
    from tilingnn_amd.solver.ml_solver import trainer as tr
    from tilingnn_amd.solver.ml_solver.losses import Losses
    net, data, want_train, want_eval = split
    calls = {"many": 0, "solo": 0}
    many, solo = Losses.unsupervised_losses_many, Losses.unsupervised_losses

    def count(name, fn):
        def wrapped(*a, **kw):
            calls[name] += 1
            return fn(*a, **kw)
        return staticmethod(wrapped)
    monkeypatch.setattr(Losses, "unsupervised_losses_many", count("many", many))
    monkeypatch.setattr(Losses, "unsupervised_losses", count("solo", solo))
    bn = net.brch_1_graph_conv_layers[1].batch_norm
    tracked = int(bn.num_batches_tracked)
    got = tr.cal_avg_loss_many(net, data, group=group, union=union)
    print(f"group {group}, union {union}: {got!r} against {want_train!r}")
    assert got == want_train
    assert calls == {"many": -(-7 // group), "solo": 0}
    assert int(bn.num_batches_tracked) == tracked and net.training and not net.autograd
    if group == 3 and union:                                        # once: running statistics instead of batch statistics
        net.eval()
        try:
            assert tr.cal_avg_loss_many(net, data, group=group, union=union) == want_eval
        finally:
            net.train()
        # a PackedLayouts instead of the data set; an empty split
        assert tr.cal_avg_loss_many(net, data.packed, group=group, union=union) == want_train
        assert np.isnan(tr.cal_avg_loss_many(net, [], group=group))


# ---------------------------------------------------------------------------------------------- 7. the training loop
def test_train_batches_with_eval_group_is_the_same_training(tmp_path):
    from tilingnn_amd.solver.ml_solver.ml_solver import ML_Solver
    from tilingnn_amd.solver.ml_solver.trainer import Trainer
    from tilingnn_amd.util import data_util as du
    graph, rng = _small_graph(), np.random.default_rng(7)
    for name, count in (("train", 5), ("test", 5)):
        os.makedirs(tmp_path / "data" / name, exist_ok=True)
        for i in range(count):
            _, (x, ci, cf, ai, af, re_index) = _cut(graph, rng)
            du.write_brick_layout_data(f"layout_{i}.pkl", re_index, node_features=x, collide_edge_index=ci, collide_edge_features=cf,
                                       align_edge_index=ai, align_edge_features=af, prefix=str(tmp_path / "data" / name / "raw"))
    _, sd = _net(3, 5)
    runs = {}
    for eval_group in (None, 4):
        net, _ = _net(3, 6)
        net.load_state_dict(sd)
        opt = torch.optim.Adam(net.parameters(), lr=2e-3)
        models = tmp_path / f"model_{eval_group}"
        trainer = Trainer(None, None, DEV, net, str(tmp_path / "data"), model_save_path=str(models))
        history = trainer.train_batches(ML_Solver(None, DEV, graph, net, num_prob_maps=1), opt, batch_size=2, training_epoch=2,
                                        save_model_per_epoch=1, shuffle_seed=1, log=lambda *_: None, eval_group=eval_group)
        last = [f for f in sorted(os.listdir(models)) if f.startswith("model_1_")]
        assert len(history) == 2 and len(last) == 1
        runs[eval_group] = (history, last[0], torch.load(str(models / last[0]), map_location="cpu"))
        assert not net.autograd
    print("history:", runs[None][0], runs[4][0])
    assert runs[None][0] == runs[4][0] and runs[None][1] == runs[4][1]
    buffers = {k for k, _ in net.named_buffers()}
    for k, v in runs[None][2].items():
        if k not in buffers:
            assert torch.equal(v, runs[4][2][k]), k


def test_train_with_eval_group_is_the_same_training(tmp_path):
    from tilingnn_amd.solver.ml_solver.trainer import Trainer
    from tilingnn_amd.util import data_util as du
    graph, rng = _small_graph(), np.random.default_rng(8)
    for name, count in (("train", 3), ("test", 2)):
        os.makedirs(tmp_path / "data" / name, exist_ok=True)
        for i in range(count):
            _, (x, ci, cf, ai, af, re_index) = _cut(graph, rng)
            du.write_brick_layout_data(f"layout_{i}.pkl", re_index, node_features=x, collide_edge_index=ci, collide_edge_features=cf,
                                       align_edge_index=ai, align_edge_features=af, prefix=str(tmp_path / "data" / name / "raw"))
    _, sd = _net(3, 5)
    histories = []
    for eval_group in (None, 2):
        net, _ = _net(3, 6)
        net.load_state_dict(sd)
        trainer = Trainer(None, None, DEV, net, str(tmp_path / "data"), model_save_path=str(tmp_path / f"model_{eval_group}"))
        histories.append(trainer.train(None, torch.optim.Adam(net.parameters(), lr=2e-3), training_epoch=2, shuffle_seed=1,
                                       log=lambda *_: None, eval_group=eval_group))
    assert histories[0] == histories[1] and all(np.isfinite(h).all() for h in histories[0])


# ---------------------------------------------------------------------------------------------- 8. the best map of a round
def test_solve_many_picks_the_best_map_per_round_in_one_call(crops, monkeypatch):
    from tilingnn_amd import TilinGNN
    from tilingnn_amd.solver.ml_solver.losses import Losses
    from tilingnn_amd.solver.ml_solver.ml_solver import ML_Solver
    from tilingnn_amd.util import algorithms as alg
    from tilingnn_amd.weights import make_state_dict
    net = TilinGNN(15, 4, 32, output_dim=3, node_features_dim=3)
    net.load_state_dict(make_state_dict(15, 4, 32, 3, 3, seed=4))
    net = net.to(DEV).train()
    solver = ML_Solver(None, DEV, None, net, num_prob_maps=3)
    layouts = [_dev(a) for a in crops]
    alone = []
    for k, lay in enumerate(layouts):
        first = solver.predict_on_device(lay)
        selection, score, order = alg.solve_by_device_greedy(solver, lay, seed=11 + k)
        alone.append((selection, score, order, alg.solve_by_device_greedy.last_rounds, first))
    calls = {"many": 0, "solo": 0}
    many, solo = Losses.unsupervised_losses_many, Losses.unsupervised_losses

    def count(name, fn):
        def wrapped(*a, **kw):
            calls[name] += 1
            return fn(*a, **kw)
        return staticmethod(wrapped)
    monkeypatch.setattr(Losses, "unsupervised_losses_many", count("many", many))
    monkeypatch.setattr(Losses, "unsupervised_losses", count("solo", solo))
    for union in (False, True):
        solver.union_forward = union
        calls.update(many=0, solo=0)
        results = alg.solve_many_by_device_greedy(solver, layouts, seeds=[11 + k for k in range(4)])
        rounds, firsts = alg.solve_many_by_device_greedy.last_rounds, alg.solve_many_by_device_greedy.last_first_probs
        assert calls["solo"] == 0 and 1 <= calls["many"] <= max(rounds), (union, calls, rounds)
        for k, (selection, score, order) in enumerate(results):
            assert np.array_equal(selection, alone[k][0]) and score == alone[k][1] and order == alone[k][2], (union, k)
            assert rounds[k] == alone[k][3], (union, k, rounds[k], alone[k][3])
            assert torch.equal(firsts[k], alone[k][4]), (union, k)
