"""The loops around the greedy kernels -- solve_by_device_greedy, solve_many_by_device_greedy (tilingnn_amd/util/algorithms.py) --
against the restated loop (tests/greedy_restatement.py: solve): the same selection, the same order, the same round count.  What is
checked here is the loops' own glue: which sub-layout a round sees, the round number a draw is keyed with, the hand-over of the
round count to and from the one-launch finish, the budget, the seeds (negative and above 2^63), the per-layout bookkeeping of the
batched loop.

The network is replaced by a STUB whose probabilities exist on the host in advance: round r gives node v (original number)
TABLES[r % 3][v], three fixed float32 tables; like ML_Solver.predict_on_device it answers 1 for a sub-layout without adjacency or
without collision edges (ml_solver.py:31-32).  The last test runs the real network on the real layout, records what it gave each
round and replays that through the restatement.  The comparison rule and the 1e-12 guard: tests/test_greedy_ops.py.
"""
import contextlib
import functools

import numpy as np
import pytest
import torch

from tests import greedy_restatement as gr
from tests.test_solve_many import SIZES_A

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda:0")
N_MAX = 5000
SOLVE_SEEDS = (0, 7, -1, 2 ** 63 + 5)
MANY_SEEDS = (0, 7, -1, 2 ** 63 + 5, 12345, 3, 2 ** 64 - 1, 11, 5, 9)


@functools.lru_cache(maxsize=None)
def tables():
    return np.random.default_rng(31).uniform(0.05, 1.0, size=(3, N_MAX)).astype(np.float32)


def prob_of_round(rnd, inverse):
    return tables()[rnd % 3][inverse]


@functools.lru_cache(maxsize=None)
def solve_layout(name):
    """x, adj, attr, col (numpy) of a synthetic layout: 8 adjacency and 10 collision edges per node, both directions stored."""
    from tilingnn_amd.synth import make_super_graph
    n, seed, drop = {"n300": (300, 1, None), "n3000": (3000, 2, None), "n2000-no-adj": (2000, 3, "adj"), "n2000-no-col": (2000, 4, "col"),
                     "n5000-no-adj": (5000, 5, "adj"), "n1": (1, 6, "one"), "n700-no-col": (700, 7, "col")}.get(name) or (int(name[1:]), 20 + SIZES_A.index(int(name[1:])), None)
    if drop == "one":
        return (np.full((1, 3), 0.5, dtype=np.float32), np.zeros((2, 0), dtype=np.int64), np.zeros((0, 15), dtype=np.float32),
                np.zeros((2, 0), dtype=np.int64))
    sg = make_super_graph(n, 8 * n, 10 * n, tile_count=2, n_edge_types=13, seed=seed)
    x, adj, attr, col = (sg.node_feature.astype(np.float32), sg.align_edge_index.astype(np.int64), sg.align_edge_features.astype(np.float32),
                         sg.collide_edge_index.astype(np.int64))
    if drop == "adj":
        adj, attr = adj[:, :0], attr[:0]
    if drop == "col":
        col = col[:, :0]
    return x, adj, attr, col


SOLVE_LAYOUTS = ("n300", "n3000", "n2000-no-adj", "n2000-no-col", "n5000-no-adj")
MANY_LAYOUTS = tuple(f"n{n}" for n in SIZES_A) + ("n1", "n700-no-col")
# max_rounds cut short: (layout, max_rounds) -- the round path notices at the top of round max_rounds + 1, the finish path inside the launch
BUDGET_CASES = (("n3000", 1), ("n3000", 3), ("n2000-no-adj", 2), ("n2000-no-adj", 1))


@functools.lru_cache(maxsize=None)
def restated(name, seed, finish=True, max_rounds=100000):
    """The restatement's solve of a layout (gr.Solve), or the BudgetExhausted it ends with."""
    x, adj, attr, col = solve_layout(name)
    try:
        return gr.solve(x.shape[0], adj, col, prob_of_round, seed, max_rounds=max_rounds, finish=finish)
    except gr.BudgetExhausted as exc:
        return exc


def _device_layout(name):
    from tilingnn_amd.util.algorithms import DeviceLayout
    x, adj, attr, col = solve_layout(name)
    t = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(DEV)
    return DeviceLayout(t(x), t(adj), t(attr), t(col))


class StubSolver:
    """What the loops ask of a solver: .device, .network (None: no forward_many, the batched loop calls predict_on_device per
    sub-layout) and predict_on_device(sub) -> [n_sub] float32 on the device."""
    network = None

    def __init__(self):
        self.device = DEV
        self.tables = torch.from_numpy(tables()).to(DEV)
        self.round = 0                                        # counted by `rounds_counted`: every round starts with ONE compaction call

    def predict_on_device(self, sub):
        n_sub = int(sub.node_feature.shape[0])
        if sub.align_edge_index.shape[1] == 0 or sub.collide_edge_index.shape[1] == 0:
            return torch.ones(n_sub, dtype=torch.float32, device=DEV)
        return self.tables[self.round % 3][sub.inverse_index].contiguous()


@contextlib.contextmanager
def rounds_counted(stub):
    """The loops do not tell the solver the round; each of them opens a round with exactly one compaction call, so those are
    counted (the library seen through a proxy, as tests/test_device_greedy.py does)."""
    from tilingnn_amd.util import algorithms as alg
    real = alg.lib

    class Proxy:
        def __getattr__(self, k):
            fn = getattr(real, k)
            if k in ("tgnn_sublayout_compact", "tgnn_sublayout_compact_many"):
                def counted(*a):
                    stub.round += 1
                    return fn(*a)
                return counted
            return fn
    stub.round = 0
    alg.lib = Proxy()
    try:
        yield
    finally:
        alg.lib = real


@pytest.mark.parametrize("finish", [True, False])
@pytest.mark.parametrize("seed", SOLVE_SEEDS)
@pytest.mark.parametrize("name", SOLVE_LAYOUTS)
def test_solve_by_device_greedy_is_the_restated_loop(name, seed, finish):
    from tilingnn_amd.util import algorithms as alg
    want = restated(name, seed, finish)
    assert want.margins.undecidable == 0, want.margins
    stub = StubSolver()
    with rounds_counted(stub):
        sel, score, order = alg.solve_by_device_greedy(stub, _device_layout(name), seed=seed, finish=finish)
    print(f"{name}, seed {seed}, finish {finish}: {int(sel.sum())} tiles in {alg.solve_by_device_greedy.last_rounds} rounds "
          f"(restated: {int(want.selection.sum())} in {want.rounds}); {want.margins}")
    assert score is None
    assert np.array_equal(sel, want.selection)
    assert order == want.order
    assert alg.solve_by_device_greedy.last_rounds == want.rounds


@pytest.mark.parametrize("name,max_rounds", BUDGET_CASES)
def test_a_spent_budget_names_the_nodes_the_restatement_leaves(name, max_rounds):
    from tilingnn_amd.util import algorithms as alg
    want = restated(name, 7, True, max_rounds)
    assert isinstance(want, gr.BudgetExhausted) and want.left > 0
    stub = StubSolver()
    with rounds_counted(stub), pytest.raises(RuntimeError, match=rf"\b{want.left} nodes still unlabelled after {max_rounds} rounds"):
        alg.solve_by_device_greedy(stub, _device_layout(name), seed=7, max_rounds=max_rounds)


def test_solve_many_by_device_greedy_is_k_restated_loops():
    from tilingnn_amd.util import algorithms as alg
    layouts = [_device_layout(name) for name in MANY_LAYOUTS]
    stub = StubSolver()
    with rounds_counted(stub):
        got = alg.solve_many_by_device_greedy(stub, layouts, seeds=list(MANY_SEEDS))
    rounds = list(alg.solve_many_by_device_greedy.last_rounds)
    assert len(got) == len(rounds) == len(MANY_LAYOUTS)
    for k, name in enumerate(MANY_LAYOUTS):
        want = restated(name, MANY_SEEDS[k])
        assert want.margins.undecidable == 0, (name, want.margins)
        print(f"layout {k} ({name}, seed {MANY_SEEDS[k]}): {int(got[k][0].sum())} tiles in {rounds[k]} rounds (restated: "
              f"{int(want.selection.sum())} in {want.rounds})")
        assert np.array_equal(got[k][0], want.selection), name
        assert got[k][2] == want.order, name
        assert rounds[k] == want.rounds, name
        assert got[k][1] is None
    assert len(set(rounds)) > 2


@pytest.mark.parametrize("seed", [0, 2 ** 63 + 5])
def test_the_real_network_on_the_real_layout_replays_through_the_restatement(seed):
    """The labyrinth layout (1 254 placements) and the network of the other greedy tests: every round's probabilities are recorded
    as the loop receives them and replayed through the restated loop.  Whether one of THESE probabilities puts a decision within
    1e-12 of flipping can only be known at run time; the replay counts, and a count above 0 fails the test loudly -- it would
    mean the comparison cannot be decided, not that it may be skipped."""
    from tests.golden_util import load_labyrinth_graph
    from tests.test_hip_parity import make_net
    from tilingnn_amd.solver.ml_solver.ml_solver import LayoutArrays, ML_Solver
    from tilingnn_amd.util import algorithms as alg
    g = load_labyrinth_graph()
    net, _ = make_net(DEV)
    solver = ML_Solver(None, DEV, None, net, num_prob_maps=1)
    recorded = []
    predict = solver.predict_on_device

    def recording(sub):
        probs = predict(sub)
        recorded.append(probs.detach().cpu().numpy().copy())
        return probs
    solver.predict_on_device = recording
    sel, _, order = alg.solve_by_device_greedy(solver, LayoutArrays(g["x"], g["adj"], g["adj_attr"], g["col"], g["col_attr"]), seed=seed)
    rounds = alg.solve_by_device_greedy.last_rounds

    def replay(rnd, inverse):
        assert recorded[rnd - 1].shape == inverse.shape and recorded[rnd - 1].dtype == np.float32
        return recorded[rnd - 1]
    want = gr.solve(int(g["x"].shape[0]), np.asarray(g["adj"]), np.asarray(g["col"]), replay, seed)
    print(f"labyrinth, seed {seed}: {int(sel.sum())} tiles in {rounds} rounds, {len(recorded)} of them with the network; {want.margins}")
    assert want.margins.undecidable == 0, f"the recorded probabilities leave a decision within {gr.GUARD:g} of flipping: {want.margins}"
    assert len(recorded) >= 2
    assert np.array_equal(sel, want.selection) and order == want.order and rounds == want.rounds
