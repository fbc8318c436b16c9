"""The hole-free greedy solve -- solve_by_probablistic_greedy(check_holes=True), HostSweep.round(guard=...), HoleGuard
(tilingnn_amd/util/algorithms.py), ML_Solver.solve(check_holes=True), BrickLayout.hole_deltas -- against the guarded sweep
restated on the host with the loop-tracing oracle as the veto (tests/hole_guard_restatement.py): the same selection, order and
round count bit for bit; no hole in any prefix of the order; and nothing changed where the option is off.

The network is a STUB with the recipe's probabilities (the pattern of tests/test_greedy_solve_restated.py): the layout is the whole
complete graph (node i = tile i) and round r gives `np.random.default_rng(1000 * seed + r).random(n)[ids]`.
"""
import gzip
import os
import shutil

import numpy as np
import pytest
import torch

from tests import hole_guard_restatement as hg
from tests import topology_oracle as to
from tests.golden_util import GOLDEN

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda:0")


class Fixture:
    def __init__(self, graph):
        from tilingnn_amd.tiling.brick_layout import BrickLayout
        from tilingnn_amd.util import data_util as du
        from tilingnn_amd.util.data_util import graph_on_device
        self.graph = graph
        self.rings = [np.asarray(t.tile_poly.exterior)[:-1] for t in graph.tiles]
        self.n = len(self.rings)
        self.col = graph.arrays.colli_edges
        self.on_device = graph_on_device(graph, DEV)
        self.layout = BrickLayout(graph, *du.create_brick_layout_from_super_set(graph, list(range(self.n))))
        assert all(self.layout.inverse_index[i] == i for i in range(self.n))

    def solved(self, selection):
        import copy
        layout = copy.deepcopy(self.layout)
        layout.predict = np.asarray(selection, dtype=float)
        return layout


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
    """What solve_by_probablistic_greedy asks of a solver: .device and predict(sub-layout) -> numpy probabilities.  One predict
    call per round, so the calls are the round count."""

    def __init__(self, seed, n):
        self.device, self.seed, self.n, self.round = DEV, seed, n, 0

    def predict(self, sub):
        self.round += 1
        ids = np.arange(self.n) if sub.inverse_index is None else sub.inverse_index.cpu().numpy()
        return hg.round_probs(self.seed, self.round, self.n, ids)


def _solve(fx, seed, **kw):
    from tilingnn_amd.util import algorithms as alg
    stub = StubSolver(seed, fx.n)
    np.random.seed(seed)
    sel, score, order = alg.solve_by_probablistic_greedy(stub, fx.layout, score_fn=lambda s, l: None, **kw)
    return sel, order, stub.round


@pytest.mark.parametrize("seed", range(8))
def test_guarded_solve_is_the_restated_sweep(seed, small):
    from tilingnn_amd.util import algorithms as alg
    want = hg.solve(small.rings, small.col, seed)
    assert want.topology == (1, 0)
    sel, order, rounds = _solve(small, seed, check_holes=True)
    guard = alg.solve_by_probablistic_greedy.last_guard
    print(f"\nhole guard small seed {seed}: {int(sel.sum())} tiles, {rounds} rounds, {guard.vetoes} vetoes, {guard.launches} launches "
          f"(restated: {int(want.selection.sum())}, {want.rounds}, {want.vetoes})")
    assert np.array_equal(sel, want.selection) and sel.dtype == want.selection.dtype
    assert order == want.order and rounds == want.rounds
    assert guard.vetoes == want.vetoes and guard.launches == len(order)
    assert small.solved(sel).count_holes(DEV) == (1, 0)


def test_ring9_the_guard_avoids_the_hole_the_plain_sweep_leaves(ring9):
    """Seed 0 of the recipe on ring 9.  Measured with the restatement on the host when the guard was designed (about a minute a
    seed there, so quoted, not run): unguarded 325 tiles, 1 component, 1 hole; guarded 326 tiles, 65 rounds, 3 589 vetoes."""
    from tilingnn_amd.util import algorithms as alg
    fx = ring9
    plain, plain_order, plain_rounds = _solve(fx, 0)
    assert int(plain.sum()) == 325 and fx.solved(plain).count_holes(DEV) == (1, 1)       # else the rest shows nothing
    sel, order, rounds = _solve(fx, 0, check_holes=True)
    guard = alg.solve_by_probablistic_greedy.last_guard
    print(f"\nhole guard ring 9 seed 0: unguarded {int(plain.sum())} tiles in {plain_rounds} rounds; guarded {int(sel.sum())} tiles, "
          f"{rounds} rounds, {guard.vetoes} vetoes, {guard.launches} launches")
    assert fx.solved(sel).count_holes(DEV) == (1, 0) and int(sel.sum()) == 326
    assert (rounds, guard.vetoes) == (65, 3589)
    assert guard.launches == len(order) == 326 and sorted(order) == np.flatnonzero(sel).tolist()
    # every prefix of the order: no hole
    prefixes = np.zeros((len(order), fx.n), dtype=np.int32)
    for k, node in enumerate(order):
        prefixes[k:, node] = 1
    topo = fx.on_device.union_topology(torch.from_numpy(prefixes).to(DEV)).cpu().numpy()
    assert (topo[:, 2] == 0).all() and (topo[:, 1] == 0).all()
    # what is left out is left out for a reason: every unselected tile that collides with no selected one would open a hole
    chosen = sel == 1
    blocked = chosen.copy()
    blocked[fx.col[1][chosen[fx.col[0]]]] = True
    rest = np.flatnonzero(~blocked)
    rings = [fx.rings[i] for i in np.flatnonzero(chosen)]
    assert to.topology(rings) == (1, 0)
    for t in rest:
        assert to.topology(rings + [fx.rings[t]])[1] > 0, int(t)
    print(f"  {rest.size} tiles stay out because each would enclose a gap")


def test_check_holes_off_is_the_run_without_the_argument(small):
    runs = []
    for kw in ({}, {"check_holes": False}):
        sel, order, rounds = _solve(small, 3, **kw)
        runs.append((sel.tobytes(), tuple(order), rounds, np.random.get_state()[1].tobytes(), np.random.get_state()[2]))
    assert runs[0] == runs[1]
    from tilingnn_amd.util.algorithms import HostSweep                      # ... and the sweep itself, guard=None
    stream = []
    for kw in ({}, {"guard": None}):
        sweep = HostSweep(small.n, small.col, uniform=np.random.RandomState(5).uniform)
        killed = sweep.round(sweep.ids(), hg.round_probs(5, 1, small.n, sweep.ids()), **kw)
        stream.append((tuple(int(v) for v in killed), tuple(sweep.order), sweep.selection.tobytes()))
    assert stream[0] == stream[1] and stream[0][1]


def _cut_layout(fx, selection, seed):
    """`_solved_layout` of tests/test_union_topology_gpu.py: the selected tiles and a random half of the others."""
    from tilingnn_amd.tiling.brick_layout import BrickLayout
    from tilingnn_amd.util import data_util as du
    keep = selection | (np.random.default_rng(seed).random(fx.n) < 0.5)
    tiles = np.flatnonzero(keep)
    layout = BrickLayout(fx.graph, *du.create_brick_layout_from_super_set(fx.graph, tiles.tolist()))
    assert len(layout.node_feature) == tiles.size < fx.n
    layout.predict = np.array([1.0 if selection[layout.inverse_index[i]] else 0.0 for i in range(tiles.size)])
    return layout, tiles


def test_brick_layout_hole_deltas(ring9):
    fx = ring9
    holed = to.thinned_set(fx.n, fx.col, 7)
    layout, tiles = _cut_layout(fx, holed, 2)
    delta, state = fx.on_device.hole_deltas(torch.from_numpy(holed.astype(np.int32)).to(DEV))
    delta, state = delta.cpu().numpy()[0], state.cpu().numpy()[0]
    dc, dh, st = layout.hole_deltas(device=DEV)
    assert dc.dtype == dh.dtype == st.dtype == np.int32 and dc.shape == dh.shape == st.shape == (tiles.size,)
    assert (dc == delta[tiles, 0]).all() and (dh == delta[tiles, 1]).all() and (st == state[tiles]).all()
    assert (st == 0).any() and (dh < 0).any() and (dh > 0).any() and (st[layout.predict == 1] == 1).all()
    # another selection than `predict`
    none = layout.hole_deltas(selection=np.zeros(tiles.size))
    assert (none[0] == 1).all() and (none[1] == 0).all() and (none[2] == 0).all()
    # the two refusals
    with pytest.raises(ValueError, match="one entry per node"):
        layout.hole_deltas(selection=np.zeros(tiles.size + 1))
    i, j = fx.col[:, 0]
    clash = np.zeros(fx.n, dtype=bool)
    clash[[i, j]] = True
    with pytest.raises(ValueError, match="collide"):
        _cut_layout(fx, clash, 4)[0].hole_deltas()


def test_ml_solver_solve_passes_check_holes_on(small):
    from tilingnn_amd.solver.ml_solver.ml_solver import ML_Solver

    class Stubbed(ML_Solver):
        def __init__(self, seed, n):
            self.device, self._greedy_solver, self._score_fn = DEV, None, (lambda s, l: None)
            self.device_greedy_min_nodes, self.device_greedy_seed = 1, 0    # (the batched loop would take every layout ...)
            self.seed, self.n, self.round = seed, n, 0

        def predict(self, layout):
            inverse = getattr(layout, "inverse_index", None)
            if not torch.is_tensor(inverse):                                # the whole layout: solve()'s predict_probs
                return hg.round_probs(self.seed, 1, self.n, np.arange(self.n))
            self.round += 1
            return hg.round_probs(self.seed, self.round, self.n, inverse.cpu().numpy())

    want = hg.solve(small.rings, small.col, 2)
    solver = Stubbed(2, small.n)
    np.random.seed(2)
    out, score = solver.solve(small.layout, check_holes=True)               # (... but the guard lives in the sequential sweep)
    assert score is None and np.array_equal(out.predict, want.selection) and out.predict_order == want.order
    assert solver.round == want.rounds and out.count_holes(DEV) == (1, 0)
    solver._greedy_solver = lambda s, l: None
    with pytest.raises(ValueError, match="check_holes"):
        solver.solve(small.layout, check_holes=True)
