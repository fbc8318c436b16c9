"""The tree search with its branch sweeps on the device -- solve_by_treesearch, DeviceTreeSweep (tilingnn_amd/util/algorithms.py),
ML_Solver.predict_top_maps, ML_Solver.solve_tree -- against the search restated on the host with the loop-tracing oracle as the
veto (tests/tree_search_restatement.py) on the small graph: the same selections, orders, result order, scores and prediction
count, bit for bit, in the batched mode and in the reference's literal mode, with the generators where the restatement leaves them.

The network is a STUB with the recipe's maps (tree_search_restatement.recipe_maps): prediction number c of a search gives the
float32 maps `np.random.default_rng(1000 * seed + c).random((n_tiles, M))` on the tiles of the sub-layout's nodes, ranked by the
recipe's own loss; the last test runs a real three-map network.
"""
import gzip
import os
import random
import shutil

import numpy as np
import pytest
import torch

from tests import tree_search_restatement as ts
from tests.golden_util import GOLDEN
from tests.test_hole_sweep_solve import Fixture
from tests.test_tree_search_host import CONFIGS, restated

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda:0")
SCORE = lambda selection, layout: float(np.sum(selection))


@pytest.fixture(scope="module")
def small():
    from tilingnn_amd.tiling.tile_graph import TileGraph
    g = TileGraph(2)
    g.load_graph_state(os.path.join(GOLDEN, "complete_graph_small.pkl"), sidecar=False)
    return Fixture(g)


@pytest.fixture(scope="module")
def ring9(tmp_path_factory):
    from tilingnn_amd.tiling.tile_graph import TileGraph
    path = str(tmp_path_factory.mktemp("labyrinth") / "complete_graph_ring9.pkl")
    with gzip.open(os.path.join(GOLDEN, "complete_graph_ring9.pkl.gz"), "rb") as src, open(path, "wb") as dst:
        shutil.copyfileobj(src, dst)
    g = TileGraph(2)
    g.load_graph_state(path, sidecar=False)
    return Fixture(g)


class StubSolver:
    """What the search asks of a solver: .device and predict_top_maps(sub-layouts, top_k), each sub-layout naming its
    prediction by `.predict_index` and its nodes by `.inverse_index`.  One call per step."""

    def __init__(self, seed, layout, n_tiles, n_maps):
        self.device, self.seed, self.n_tiles, self.n_maps = DEV, seed, n_tiles, n_maps
        self.tiles = np.array([layout.inverse_index[i] for i in range(len(layout.node_feature))], dtype=np.int64)
        self.calls, self.asked = 0, []

    def predict_top_maps(self, subs, top_k):
        self.calls += 1
        out = []
        for sub in subs:
            self.asked.append(sub.predict_index)
            ids = sub.inverse_index.cpu().numpy()
            out.append(ts.recipe_maps(self.seed, self.n_tiles, self.n_maps, top_k)(sub.predict_index, self.tiles[ids]))
        return out


def _same_state(a, b):
    return a[0] == b[0] and np.array_equal(a[1], b[1]) and a[2:] == b[2:]


def _assert_same_results(got, want):
    assert len(got) == len(want.results)
    for (sel, score, order), (wsel, wscore, worder) in zip(got, want.results):
        assert sel.dtype == wsel.dtype and sel.tobytes() == wsel.tobytes() and order == worder and score == wscore


@pytest.mark.parametrize("config", range(3))
@pytest.mark.parametrize("seed", range(8))
def test_batched_search_is_the_restated_search(small, config, seed):
    from tilingnn_amd.util import algorithms as alg
    fx, cfg = small, dict(CONFIGS[config])
    want = restated(fx.rings, fx.col, cfg, seed)
    n_maps = cfg.pop("n_maps")
    stub = StubSolver(seed, fx.layout, fx.n, n_maps)
    np.random.seed(123)
    random.seed(123)
    before = np.random.get_state(), random.getstate()
    got, cnt = alg.solve_by_treesearch(stub, fx.layout, seed=seed, score_fn=SCORE, **cfg)
    assert _same_state(before[0], np.random.get_state()) and before[1] == random.getstate()     # neither global generator is touched
    dsw = alg.solve_by_treesearch.last_sweep
    print(f"\ntree search small config {config} seed {seed}: {cnt} predictions, {dsw.calls} sweep calls, {dsw.branches} branches, "
          f"{dsw.vetoes} vetoes, {len(got)} results, pool of {dsw.n_slots}")
    assert cnt == want.predict_cnt and stub.asked == list(range(1, cnt + 1))
    _assert_same_results(got, want)
    # one forward call and one sweep call per STEP, not per branch
    assert dsw.calls == stub.calls == alg.solve_by_treesearch.last_steps == len(want.steps)
    assert dsw.branches == sum(len(step) for step in want.steps) and (dsw.branches > dsw.calls or config == 0 and cfg["beam"] == 1)
    assert dsw.vetoes == sum(b.vetoes for step in want.steps for b in step)
    if cfg["check_holes"]:
        for sel, _, _ in got:
            assert fx.solved(fx.layout, sel).count_holes(DEV)[1] == 0


@pytest.mark.parametrize("top_k", [1, 2])
@pytest.mark.parametrize("seed", range(8))
def test_literal_search_is_the_restated_literal_search(small, top_k, seed):
    from tilingnn_amd.util import algorithms as alg
    fx = small
    kw = dict(top_k=top_k, check_holes=True, max_predictions=14, beam=1, roots=1, literal=True)
    np.random.seed(seed)
    random.seed(seed)
    want = ts.search(fx.rings, fx.col, ts.recipe_maps(seed, fx.n, top_k, top_k), score_fn=lambda sel: float(sel.sum()), **kw)
    want_state = np.random.get_state(), random.getstate()
    np.random.seed(seed)
    random.seed(seed)
    got, cnt = alg.solve_by_treesearch(StubSolver(seed, fx.layout, fx.n, top_k), fx.layout, score_fn=SCORE, **kw)
    assert _same_state(want_state[0], np.random.get_state()) and want_state[1] == random.getstate()
    assert cnt == want.predict_cnt
    _assert_same_results(got, want)
    dsw = alg.solve_by_treesearch.last_sweep
    assert dsw.calls == dsw.branches == sum(len(step) for step in want.steps)       # K = 1 per branch: the stream orders them
    assert dsw.vetoes == sum(b.vetoes for step in want.steps for b in step)


def test_the_pool_grows_without_dropping_a_state(small):
    from tilingnn_amd.util.algorithms import DeviceTreeSweep
    fx = small
    dsw = DeviceTreeSweep(fx.graph, fx.n, fx.col, np.arange(fx.n), True, DEV, slots=1)
    root = dsw.new_slot()
    rng = np.random.RandomState(1)
    order = rng.permutation(fx.n)
    (stats, acc, gone), = dsw.sweep([(root, root, order, np.full(fx.n, 0.5), rng)])
    rows = [t[root].clone() for t in (dsw.unlabelled, dsw.tile_alive, dsw.label, dsw.chi_cache)]
    slots = [dsw.new_slot() for _ in range(5)]
    assert dsw.n_slots == 8 and sorted(slots + [root]) == list(range(6))
    assert all(torch.equal(t[root], r) for t, r in zip((dsw.unlabelled, dsw.tile_alive, dsw.label, dsw.chi_cache), rows))
    assert dsw.unlabelled[slots[-1]].all().item() and not dsw.tile_alive[slots[-1]].any().item()
    assert int((rows[0] == 0).sum()) == len(acc) + len(gone) and stats[3] == len(acc) > 0
    with pytest.raises(ValueError, match="DeviceTreeSweep"):
        dsw.sweep([(root, slots[0], order, np.ones(fx.n), rng), (root, root, order, np.ones(fx.n), rng)])
    assert dsw.calls == 1


def test_ring9_one_sweep_call_per_step(ring9):
    from tilingnn_amd.util import algorithms as alg
    fx = ring9
    stub = StubSolver(0, fx.layout, fx.n, 1)
    got, cnt = alg.solve_by_treesearch(stub, fx.layout, top_k=1, check_holes=True, max_predictions=12, beam=4, roots=4, seed=0, score_fn=SCORE)
    dsw = alg.solve_by_treesearch.last_sweep
    print(f"\ntree search ring 9: {cnt} predictions, {dsw.calls} sweep calls, {dsw.branches} branches, {dsw.vetoes} vetoes, {len(got)} results")
    assert cnt == 12 and dsw.calls == stub.calls == alg.solve_by_treesearch.last_steps == 3 and dsw.branches == 12
    col = np.asarray(fx.col).reshape(2, -1)
    for sel, _, order in got:
        chosen = sel > 0
        assert not (chosen[col[0]] & chosen[col[1]]).any() and fx.solved(fx.layout, sel).count_holes(DEV)[1] == 0


def test_real_network_top_maps_and_solve_tree(small):
    """Seed-0 weights of a three-map network on a half cut of the small graph."""
    from tilingnn_amd import TilinGNN
    from tilingnn_amd.solver.ml_solver.ml_solver import ML_Solver
    from tilingnn_amd.util import algorithms as alg
    from tilingnn_amd.weights import make_state_dict
    fx = small
    layout = fx.half(5)
    fe, fxd = int(np.asarray(layout.align_edge_features).shape[1]), int(np.asarray(layout.node_feature).shape[1])
    net = TilinGNN(adj_edge_features_dim=fe, network_depth=20, network_width=32, output_dim=3, node_features_dim=fxd)
    net.load_state_dict(make_state_dict(fe, 20, 32, 3, fxd, seed=0), strict=True)
    solver = ML_Solver(None, DEV, fx.graph, net.to(DEV).train(), num_prob_maps=3, score_fn=SCORE)
    n = len(layout.node_feature)
    one = solver.predict(layout)
    x, adj, attr, col, colf = layout.get_data_as_torch_tensor(DEV)
    full = solver.network.forward_checked(x=x, adj_e_index=adj, adj_e_features=attr, col_e_idx=col, col_e_features=colf)[0].detach()
    rank = np.argsort(solver.get_unsupervised_losses_from_layout(layout, full))
    for top_k in (1, 2, 3, 5):
        top, lone = solver.predict_top_maps([alg.DeviceLayout.upload(layout, DEV), alg.DeviceLayout.upload(fx.cut([17]), DEV)], top_k)
        keep = min(top_k, 3)
        assert top.dtype == np.float32 and top.shape == (n, keep) and top[:, 0].tobytes() == one.tobytes()
        assert top.tobytes() == np.ascontiguousarray(full.cpu().numpy()[:, rank[:keep]]).tobytes()
        assert lone.shape == (1, keep) and (lone == 1.0).all() and lone.dtype == np.float32       # one node, no edge: ones
    runs = []
    for _ in range(2):
        out = solver.solve_tree(layout, top_k=2, check_holes=True, max_predictions=16, beam=4, roots=2, seed=3)
        runs.append([(o.predict.tobytes(), tuple(o.predict_order), score, o.predict_probs.tobytes()) for o, score in out])
    assert runs[0] == runs[1] and len(runs[0]) > 0 and solver.last_predict_cnt <= 16
    scores = [r[2] for r in runs[0]]
    assert scores == sorted(scores, reverse=True) and all(r[3] == one.tobytes() for r in runs[0])
    for o, score in out:
        assert score == o.predict.sum() == len(o.predict_order) and o.count_holes(DEV)[1] == 0
    print(f"\nsolve_tree with the network: {solver.last_predict_cnt} predictions, {len(out)} tilings of {scores} tiles")
