"""The hole-free greedy solve with the guarded sweep on the device -- solve_by_probablistic_greedy(check_holes=True,
device_sweep=True), DeviceHoleSweep, solve_many_hole_free (tilingnn_amd/util/algorithms.py), ML_Solver.solve(device_sweep=True),
ML_Solver.solve_many_hole_free (and solve_many with `check_holes_many` set), ML_Solver.predict_many -- against the guarded sweep restated on the host with the
loop-tracing oracle as the veto (tests/hole_guard_restatement.py) on the small graph, and against the host-guarded path of the
package on ring 9: the same selection, order, round count, vetoes and RNG state, bit for bit.

The network is a STUB with the recipe's probabilities (tests/test_hole_guard_solve.py): round r of a layout gives
`np.random.default_rng(1000 * seed + r).random(n_tiles)[tiles of the unlabelled nodes]`; the last test runs the real network.
"""
import gzip
import os
import shutil

import numpy as np
import pytest
import torch

from tests import hole_guard_restatement as hg
from tests.golden_util import GOLDEN

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda:0")


class Fixture:
    def __init__(self, graph):
        from tilingnn_amd.util.data_util import graph_on_device
        self.graph = graph
        self.rings = [np.asarray(t.tile_poly.exterior)[:-1] for t in graph.tiles]
        self.n = len(self.rings)
        self.col = graph.arrays.colli_edges
        self.on_device = graph_on_device(graph, DEV)
        self.layout = self.cut(np.arange(self.n))

    def cut(self, tiles):
        from tilingnn_amd.tiling.brick_layout import BrickLayout
        from tilingnn_amd.util import data_util as du
        tiles = np.asarray(tiles)
        layout = BrickLayout(self.graph, *du.create_brick_layout_from_super_set(self.graph, tiles.tolist()))
        assert len(layout.node_feature) == tiles.size and all(layout.inverse_index[i] == t for i, t in enumerate(tiles))
        return layout

    def half(self, seed):
        return self.cut(np.flatnonzero(np.random.default_rng(seed).random(self.n) < 0.5))

    def solved(self, layout, selection):
        import copy
        layout = copy.deepcopy(layout)
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


def _tiles_of(layout):
    return np.array([layout.inverse_index[i] for i in range(len(layout.node_feature))], dtype=np.int64)


class StubSolver:
    """What the loops ask of a solver: .device, predict(sub-layout) for one layout and predict_many(sub-layouts) for K, each
    sub-layout naming its layout by `.origin_index`.  The recipe's probabilities; one call per round of a layout."""

    def __init__(self, seeds, layouts, n_tiles):
        self.device, self.seeds, self.n_tiles = DEV, list(seeds), n_tiles
        self.tiles = [_tiles_of(l) for l in layouts]
        self.rounds = [0] * len(self.tiles)
        self.many_calls = 0

    def _probs(self, k, sub):
        self.rounds[k] += 1
        ids = np.arange(self.tiles[k].size) if sub.inverse_index is None else sub.inverse_index.cpu().numpy()
        return hg.round_probs(self.seeds[k], self.rounds[k], self.n_tiles, self.tiles[k][ids])

    def predict(self, sub):
        return self._probs(0, sub)

    def predict_many(self, subs):
        self.many_calls += 1
        return [self._probs(sub.origin_index, sub) for sub in subs]


def _solve(fx, layout, seed, **kw):
    """One solo solve of `layout` after np.random.seed(seed) -> (selection, order, rounds, the guard)."""
    from tilingnn_amd.util import algorithms as alg
    stub = StubSolver([seed], [layout], fx.n)
    np.random.seed(seed)
    sel, score, order = alg.solve_by_probablistic_greedy(stub, layout, score_fn=lambda s, l: None, **kw)
    return sel, order, stub.rounds[0], alg.solve_by_probablistic_greedy.last_guard


@pytest.mark.parametrize("seed", range(8))
def test_device_sweep_is_the_restated_sweep(seed, small):
    want = hg.solve(small.rings, small.col, seed)
    assert want.topology == (1, 0)
    sel, order, rounds, guard = _solve(small, small.layout, seed, check_holes=True, device_sweep=True)
    print(f"\ndevice sweep small seed {seed}: {int(sel.sum())} tiles, {rounds} rounds, {int(guard.vetoes[0])} vetoes, "
          f"{int(guard.launches[0])} launches (restated: {int(want.selection.sum())}, {want.rounds}, {want.vetoes})")
    assert np.array_equal(sel, want.selection) and sel.dtype == want.selection.dtype
    assert order == want.order and rounds == want.rounds
    assert guard.vetoes[0] == want.vetoes and guard.launches[0] == guard.calls == rounds
    assert small.solved(small.layout, sel).count_holes(DEV) == (1, 0)


def test_ring9_device_sweep_is_the_host_guarded_solve(ring9):
    fx = ring9
    host_sel, host_order, host_rounds, host_guard = _solve(fx, fx.layout, 0, check_holes=True)
    host_state = np.random.get_state()
    sel, order, rounds, guard = _solve(fx, fx.layout, 0, check_holes=True, device_sweep=True)
    state = np.random.get_state()
    print(f"\ndevice sweep ring 9 seed 0: {int(sel.sum())} tiles, {rounds} rounds, {int(guard.vetoes[0])} vetoes, {int(guard.launches[0])} "
          f"launches (host guard: {host_guard.launches} launches)")
    assert np.array_equal(sel, host_sel) and sel.dtype == host_sel.dtype and order == host_order and rounds == host_rounds
    assert (int(sel.sum()), rounds, int(guard.vetoes[0])) == (326, 65, 3589) and host_guard.vetoes == 3589
    assert guard.launches[0] == guard.calls == 65 and host_guard.launches == 326
    # the generator is where the host sweep leaves it
    assert state[0] == host_state[0] and np.array_equal(state[1], host_state[1]) and state[2:] == host_state[2:]
    # every prefix of the order: no hole, by one batched call
    prefixes = np.zeros((len(order), fx.n), dtype=np.int32)
    for k, node in enumerate(order):
        prefixes[k:, node] = 1
    topo = fx.on_device.union_topology(torch.from_numpy(prefixes).to(DEV)).cpu().numpy()
    assert (topo[:, 2] == 0).all() and (topo[:, 1] == 0).all()


def test_device_sweep_alone_raises(small):
    from tilingnn_amd.util import algorithms as alg
    with pytest.raises(ValueError, match="device_sweep"):
        alg.solve_by_probablistic_greedy(StubSolver([0], [small.layout], small.n), small.layout, device_sweep=True)


def _stubbed_solver(stub):
    from tilingnn_amd.solver.ml_solver.ml_solver import ML_Solver

    class Stubbed(ML_Solver):
        def __init__(self):
            self.device, self._greedy_solver, self._score_fn = DEV, None, (lambda s, l: None)
            self.device_greedy_min_nodes, self.device_greedy_seed = None, 0

        def predict(self, layout):
            return stub.predict(layout)

        def predict_many(self, subs):
            return stub.predict_many(subs)

    return Stubbed()


def test_solve_many_hole_free_is_k_solo_solves(ring9):
    from tilingnn_amd.tiling.brick_layout import detect_holes_many
    from tilingnn_amd.util import algorithms as alg
    fx = ring9
    layouts = [fx.layout, fx.half(1), fx.half(2), fx.half(3), fx.cut([17])]
    seeds = [4, 0, 9, 2, 6]
    want = [_solve(fx, layout, seed, check_holes=True) for layout, seed in zip(layouts, seeds)]
    np.random.seed(123)
    before = np.random.get_state()
    stub = StubSolver(seeds, layouts, fx.n)
    out = _stubbed_solver(stub).solve_many_hole_free(layouts, seed=seeds)
    after = np.random.get_state()
    assert np.array_equal(before[1], after[1]) and before[2:] == after[2:]            # the global stream is not touched
    rounds, vetoes = alg.solve_many_hole_free.last_rounds, alg.solve_many_hole_free.last_vetoes
    print(f"\nsolve_many_hole_free ring 9: tiles {[int(o.predict.sum()) for o, _ in out]}, rounds {rounds}, vetoes {vetoes}, "
          f"{alg.solve_many_hole_free.last_sweep_calls} sweep calls")
    for k, ((layout, score), (sel, order, n_rounds, guard)) in enumerate(zip(out, want)):
        assert score is None and np.array_equal(layout.predict, sel) and layout.predict.dtype == sel.dtype, k
        assert layout.predict_order == order and rounds[k] == n_rounds and vetoes[k] == guard.vetoes, k
    assert all(holes == 0 for _, holes in detect_holes_many([o for o, _ in out], DEV))
    # one sweep call and one predict_many per round of the LONGEST solve, not one per layout and round
    assert alg.solve_many_hole_free.last_sweep_calls == stub.many_calls == max(rounds) < sum(rounds)
    assert len(set(rounds)) > 1 and sum(vetoes) > 0


def test_solve_many_hole_free_refusals(small, ring9):
    from tilingnn_amd.util.algorithms import DeviceLayout
    solver = _stubbed_solver(StubSolver([0, 0], [small.layout, ring9.layout], small.n))
    with pytest.raises(ValueError, match="another complete graph"):
        solver.solve_many_hole_free([small.layout, ring9.layout])
    bare = DeviceLayout.upload(small.layout, DEV)
    with pytest.raises(ValueError, match="complete_graph"):
        solver.solve_many_hole_free([small.layout, bare])
    assert solver.solve_many_hole_free([]) == []
    solver._greedy_solver = lambda s, l: None
    with pytest.raises(ValueError, match="check_holes"):
        solver.solve_many_hole_free([small.layout])
    solver.check_holes_many = True                                          # ... and through solve_many with the switch set
    with pytest.raises(ValueError, match="check_holes"):
        solver.solve_many([small.layout])


def test_real_network_predict_many_and_solve_many(ring9):
    """Seed-0 weights (no checkpoint is in the tree) on three ring-9 cuts.  `solve_many` keeps its signature (other tests pin
    it): the hole-free loop is `solve_many_hole_free`, and `check_holes_many = True` makes `solve_many` run it."""
    from tilingnn_amd import TilinGNN
    from tilingnn_amd.solver.ml_solver.ml_solver import ML_Solver
    from tilingnn_amd.tiling.brick_layout import detect_holes_many
    from tilingnn_amd.util import algorithms as alg
    from tilingnn_amd.weights import make_state_dict
    fx = ring9
    layouts = [fx.half(11), fx.half(12), fx.half(13)]
    seeds = [3, 1, 8]
    fe, fxd = int(np.asarray(layouts[0].align_edge_features).shape[1]), int(np.asarray(layouts[0].node_feature).shape[1])
    net = TilinGNN(adj_edge_features_dim=fe, network_depth=20, network_width=32, node_features_dim=fxd)
    net.load_state_dict(make_state_dict(fe, 20, 32, 1, fxd, seed=0), strict=True)
    solver = ML_Solver(None, DEV, fx.graph, net.to(DEV).train(), num_prob_maps=1, score_fn=lambda s, l: None)
    many = solver.predict_many([alg.DeviceLayout.upload(l, DEV) for l in layouts])
    for got, layout in zip(many, layouts):
        one = solver.predict(layout)
        assert got.dtype == one.dtype == np.float32 and got.shape == one.shape and got.tobytes() == one.tobytes()
    assert solver.check_holes_many is False
    runs = []
    for attempt in range(2):
        if attempt:                                                         # the switch: solve_many runs the same loop
            solver.check_holes_many = True
        out = solver.solve_many(layouts, seed=seeds) if attempt else solver.solve_many_hole_free(layouts, seed=seeds)
        runs.append([(o.predict.tobytes(), tuple(o.predict_order)) for o, _ in out] + [tuple(alg.solve_many_hole_free.last_rounds),
                                                                                        tuple(alg.solve_many_hole_free.last_vetoes)])
    assert runs[0] == runs[1]
    rounds, vetoes = alg.solve_many_hole_free.last_rounds, alg.solve_many_hole_free.last_vetoes
    for k, (layout, seed) in enumerate(zip(layouts, seeds)):
        np.random.seed(seed)
        solo, _ = solver.solve(layout, check_holes=True, device_sweep=True)
        guard = alg.solve_by_probablistic_greedy.last_guard
        assert np.array_equal(out[k][0].predict, solo.predict) and out[k][0].predict_order == solo.predict_order, k
        assert rounds[k] == guard.launches[0] and vetoes[k] == guard.vetoes[0], k
    assert all(holes == 0 for _, holes in detect_holes_many([o for o, _ in out], DEV))
    solver.check_holes_many = False
    print(f"\nsolve_many_hole_free with the network: tiles {[int(o.predict.sum()) for o, _ in out]}, rounds {rounds}, vetoes {vetoes}")


def test_predict_many_picks_the_best_map_as_predict_does(ring9):
    """A network with three probability maps: one loss call picks every layout's map, and the bits are `predict`'s."""
    from tilingnn_amd import TilinGNN
    from tilingnn_amd.solver.ml_solver.ml_solver import ML_Solver
    from tilingnn_amd.util import algorithms as alg
    from tilingnn_amd.weights import make_state_dict
    layouts = [ring9.half(21), ring9.half(22), ring9.cut([17]), ring9.half(23)]
    fe, fxd = int(np.asarray(layouts[0].align_edge_features).shape[1]), int(np.asarray(layouts[0].node_feature).shape[1])
    net = TilinGNN(adj_edge_features_dim=fe, network_depth=20, network_width=32, output_dim=3, node_features_dim=fxd)
    net.load_state_dict(make_state_dict(fe, 20, 32, 3, fxd, seed=0), strict=True)
    solver = ML_Solver(None, DEV, ring9.graph, net.to(DEV).train(), num_prob_maps=3)
    many = solver.predict_many([alg.DeviceLayout.upload(l, DEV) for l in layouts])
    for got, layout in zip(many, layouts):
        one = solver.predict(layout)
        assert got.dtype == one.dtype == np.float32 and got.shape == one.shape and got.tobytes() == one.tobytes()
    assert many[2].tolist() == [1.0]                                        # one node, no edge: ones without the network
