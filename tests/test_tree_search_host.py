"""Host side of the tree search (csrc/tree_sweep.hip, util/algorithms.py: solve_by_treesearch): the per-visit rule of
csrc/tree_sweep_step.h with the acceptance steps of csrc/hole_sweep_step.h run on the host under sanitizers as the sweep of one
branch, over EVERY visiting order of three hand-made sets at three rotations with scripted p, draws and collision rows, with and
without the hole veto, against the walk written out again here from the oracle's subset table alone (positions, skips, breaks,
vetoes, draws, acceptances, kills, final selection; d holes at every evaluated visit and the label invariant after every
acceptance are checked by the program).  Then the numpy facts the host side relies on, the self-checks of the restated search
(tests/tree_search_restatement.py) on the small graph, and the refusals that need no GPU."""
import itertools
import math
import os
import random

import numpy as np
import pytest

from tests import hole_delta_cases as hc
from tests import topology_oracle as to
from tests import tree_search_restatement as ts
from tests.golden_util import GOLDEN
from tests.sweep_host_cases import NBR, SETS, build_step_program, run_program

P = (1.0, 0.5, 0.75, 1.25, 0.25, 1.0, 0.5, 1.0, 0.875)          # prob_m by position; one above 1 (the reference's quirk)


@pytest.fixture(scope="module")
def step_program(tmp_path_factory):
    return build_step_program(tmp_path_factory, "tree_sweep_step_test")


def _run(exe, tmp_path, tiles, want, orders, check_holes):
    tail, out = run_program(exe, tmp_path, tiles, want, orders, P, (int(check_holes),))
    assert tail[0::2] == ["orders", "visits", "mismatches", "err"] and tail[5] == "0" and tail[7] == "0", tail
    assert int(tail[1]) == orders.shape[0]
    return out.reshape(-1, 8)


def _walk_from_the_table(n, want, orders, check_holes):
    """The sweep of every order at once from the oracle's table alone: [orders, 8] as the program writes them."""
    count = orders.shape[0]
    row = np.arange(count)
    holes = want[:, 1].astype(np.int64)
    mask = np.zeros(count, dtype=np.int64)
    unl = np.ones((count, n), dtype=bool)
    running = np.ones(count, dtype=bool)
    reached, vetoes, draws, accepted, killed, skipped, breaks = (np.zeros(count, dtype=np.int64) for _ in range(7))
    for step in range(2 * n):                                    # two passes, the second backwards, the state carried over
        pos = step if step < n else 2 * n - 1 - step
        if step == n:
            running[:] = True
        t = orders[:, pos].astype(np.int64)
        reached[running] += 1
        labelled = running & ~unl[row, t]                        # consumes a draw: passed over, or the pass ends
        u = ((7 * row + 13 * draws) % 32) / 32.0
        draws[labelled] += 1
        skip = labelled & (u < P[pos])
        skipped[skip] += 1
        breaks[labelled & ~skip] += 1
        running &= ~(labelled & ~skip)
        live = running & ~labelled
        d = holes[mask | (1 << t)] - holes[mask]
        veto = live & (d > 0) & bool(check_holes)                # no draw
        vetoes[veto] += 1
        acc = live & ~veto                                       # no draw either
        accepted[acc] += 1
        unl[row[acc], t[acc]] = False
        mask[acc] |= 1 << t[acc]
        for node, nbrs in NBR[n].items():
            for v in dict.fromkeys(nbrs):
                hit = acc & (t == node) & unl[:, v]
                killed[hit] += 1
                unl[hit, v] = False
    return np.stack([reached, vetoes, draws, accepted, killed, skipped, breaks, mask], axis=1)


@pytest.mark.parametrize("check_holes", [True, False])
def test_the_branch_sweep_on_the_host_every_visiting_order(step_program, tmp_path, check_holes):
    sets = hc.sets()
    for name in SETS:
        tiles = sets[name]
        n = len(tiles)
        want, _ = hc.subset_table(name, tiles)
        orders = np.array(list(itertools.permutations(range(n))), dtype=np.uint8)
        assert orders.shape[0] == math.factorial(n)
        expect = _walk_from_the_table(n, want, orders, check_holes)
        # kills, skips and breaks in every set; vetoes wherever a tile can close a gap (the plus among its four squares never does)
        assert (expect[:, 4] > 0).any() and (expect[:, 5] > 0).any() and (expect[:, 6] > 0).any()
        assert (expect[:, 1] > 0).any() == (check_holes and name != "plus among four squares")
        assert (expect[:, 2] == expect[:, 5] + expect[:, 6]).all()                      # a draw per labelled node met, no other
        assert (expect[:, 3] + expect[:, 4] <= n).all()
        for angle in to.ROTATIONS:
            got = _run(step_program, tmp_path, to.rotated(tiles, angle), want, orders, check_holes)
            assert np.array_equal(got, expect), (name, angle, np.flatnonzero((got != expect).any(axis=1))[:5])
        print(f"\ntree sweep host ({'veto' if check_holes else 'no veto'}): {name}: {orders.shape[0]} orders, "
              f"{int(expect[:, 0].sum())} positions, {int(expect[:, 1].sum())} vetoes, {int(expect[:, 2].sum())} draws, "
              f"{int(expect[:, 3].sum())} accepted, {int(expect[:, 4].sum())} killed, {int(expect[:, 5].sum())} skipped, "
              f"{int(expect[:, 6].sum())} breaks")


# ------------------------------------------------------------------------------------------------ numpy facts
def _same_state(a, b):
    return a[0] == b[0] and np.array_equal(a[1], b[1]) and a[2:] == b[2:]


@pytest.mark.parametrize("consumed", [0, 1, 7, 50])
def test_branch_generator_batch_draw_and_rewind_is_scalar_draws(consumed):
    """DeviceTreeSweep draws a branch's uniforms in one `uniform(size=n)` call and afterwards rewinds and draws what the walk
    consumed; the restated search draws `random_sample()` one at a time from `RandomState([seed, s])`."""
    scalar = np.random.RandomState([3, 17])
    one_by_one = np.array([scalar.random_sample() for _ in range(50)])
    batch = np.random.RandomState([3, 17])
    state = batch.get_state()
    assert batch.uniform(size=50).tobytes() == one_by_one.tobytes()
    batch.set_state(state)
    batch.uniform(size=consumed)
    after = np.random.RandomState([3, 17])
    for _ in range(consumed):
        after.random_sample()
    assert _same_state(batch.get_state(), after.get_state())
    assert batch.random_sample() == after.random_sample()
    # the global generator (literal mode): np.random.random() is the scalar draw of the reference
    np.random.seed(11)
    singles = np.array([np.random.random() for _ in range(50)])
    np.random.seed(11)
    state = np.random.get_state()
    assert np.random.uniform(size=50).tobytes() == singles.tobytes()
    np.random.set_state(state)
    np.random.uniform(size=consumed)
    a = np.random.get_state()
    np.random.seed(11)
    for _ in range(consumed):
        np.random.random()
    assert _same_state(a, np.random.get_state())


def test_choice_is_complete_before_the_first_collision_draw():
    """The order is drawn first and the collision draws follow it in the stream: a generator that drew the order, then k
    uniforms, is where one that drew the order and k scalars is -- whatever the walk does with the order in between."""
    p = ts.sampling_probabilities(np.random.default_rng(0).random(40))
    assert abs(p.sum() - 1.0) < 1e-12 and (p > 0).all()
    a, b = np.random.RandomState([0, 5]), np.random.RandomState([0, 5])
    order_a = a.choice(40, 40, replace=False, p=p)
    order_b = b.choice(40, 40, replace=False, p=p)
    assert np.array_equal(order_a, order_b) and sorted(order_a.tolist()) == list(range(40))
    assert _same_state(a.get_state(), b.get_state())
    ahead = a.uniform(size=40)
    assert ahead[:6].tolist() == [b.random_sample() for _ in range(6)]


def test_log_probabilities_keep_the_networks_dtype():
    prob = np.array([0.0, 0.25, 1.0], dtype=np.float32)
    log_prob = np.log(np.clip(prob, ts.EPS, 1.0))
    assert log_prob.dtype == np.float32 and (np.ones(3) + log_prob).dtype == np.float64


# ------------------------------------------------------------------------------------------------ the restated search
@pytest.fixture(scope="module")
def small():
    from tilingnn_amd.tiling.tile_graph import TileGraph
    g = TileGraph(2)
    g.load_graph_state(os.path.join(GOLDEN, "complete_graph_small.pkl"), sidecar=False)
    rings = [np.asarray(t.tile_poly.exterior)[:-1] for t in g.tiles]
    col = g.arrays.colli_edges
    assert len(rings) == 150 and np.asarray(col).reshape(2, -1).shape[1] == 1106
    return rings, col


CONFIGS = (dict(top_k=1, n_maps=1, roots=4, beam=4, check_holes=True, max_predictions=1000),
           dict(top_k=2, n_maps=2, roots=1, beam=4, check_holes=True, max_predictions=48),
           dict(top_k=3, n_maps=3, roots=2, beam=8, check_holes=False, max_predictions=64))


def restated(rings, col, config, seed, **kw):
    config = dict(config)
    n_maps = config.pop("n_maps")
    return ts.search(rings, col, ts.recipe_maps(seed, len(rings), n_maps, config["top_k"]), seed=seed,
                     score_fn=lambda sel: float(sel.sum()), **config, **kw)


@pytest.mark.parametrize("config", range(3))
@pytest.mark.parametrize("seed", range(3))
def test_restated_search_results_are_tilings_and_the_inputs_reach_every_code(small, config, seed):
    rings, col = small
    cfg = CONFIGS[config]
    np.random.seed(77)
    random.seed(77)
    before = np.random.get_state(), random.getstate()
    s = restated(rings, col, cfg, seed)
    assert _same_state(before[0], np.random.get_state()) and before[1] == random.getstate()     # neither global generator is touched
    col = np.asarray(col).reshape(2, -1)
    codes = {code for step in s.steps for br in step for code, _ in br.trace}
    assert codes == {ts.ACCEPTED, ts.SKIPPED, ts.BREAK} | ({ts.VETOED} if cfg["check_holes"] else set())
    assert s.predict_cnt <= cfg["max_predictions"] and s.predict_cnt == sum(len(p) for p in s.pops)
    assert max(len(step) for step in s.steps) == min(cfg["beam"], 8) * cfg["top_k"] or config == 0
    assert len(s.results) > 0 and len({r[0].tobytes() for r in s.results}) == len(s.results)
    scores = [r[1] for r in s.results]
    assert scores == sorted(scores, reverse=True)
    for selection, score, order in s.results:
        chosen = selection > 0
        assert sorted(order) == np.flatnonzero(chosen).tolist() and score == chosen.sum()
        assert not (chosen[col[0]] & chosen[col[1]]).any()                               # collision-free
        if cfg["check_holes"]:
            assert to.topology([rings[i] for i in order])[1] == 0
    for step in s.steps:
        for br in step:
            if not br.requeued and br.unlabelled.any():
                assert cfg["check_holes"] and not br.accepted                            # finished with nodes left: every one vetoed
            if not br.requeued and not br.unlabelled.any():
                blocked = np.zeros(len(rings), dtype=bool)
                blocked[br.selected] = True
                blocked[col[1][np.isin(col[0], br.selected)]] = True
                assert blocked.all()                                                     # maximal
    print(f"\nrestated tree search config {config} seed {seed}: {s.predict_cnt} predictions, {len(s.steps)} steps, up to "
          f"{max(len(step) for step in s.steps)} branches a step, {len(s.results)} results")


def test_restated_literal_search_consumes_the_global_streams(small):
    rings, col = small
    runs = []
    for _ in range(2):
        np.random.seed(4)
        random.seed(4)
        s = ts.search(rings, col, ts.recipe_maps(4, len(rings), 2, 2), top_k=2, check_holes=True, max_predictions=12, beam=1, roots=1,
                      literal=True, score_fn=lambda sel: float(sel.sum()))
        runs.append(([b.accepted for step in s.steps for b in step], np.random.get_state()[2], random.getstate()))
    assert runs[0][0] == runs[1][0] and runs[0][1:] == runs[1][1:]
    np.random.seed(4)
    assert np.random.get_state()[2] != runs[0][1]                                        # the stream moved


# ------------------------------------------------------------------------------------------------ refusals that need no GPU
def test_solve_by_treesearch_refusals():
    import torch
    from tilingnn_amd.util.algorithms import DeviceLayout, DeviceTreeSweep, solve_by_treesearch

    class Solver:
        device = torch.device("cpu")

    z = torch.zeros
    bare = DeviceLayout(z(3, 1), z(2, 0, dtype=torch.int64), z(0, 1), z(2, 0, dtype=torch.int64))
    with pytest.raises(ValueError, match="max_predictions or time_limit"):
        solve_by_treesearch(Solver(), bare)
    with pytest.raises(ValueError, match="literal"):
        solve_by_treesearch(Solver(), bare, max_predictions=4, literal=True, beam=2, roots=1)
    with pytest.raises(ValueError, match="literal"):
        solve_by_treesearch(Solver(), bare, max_predictions=4, literal=True, beam=1, roots=2)
    with pytest.raises(ValueError, match="check_holes"):
        solve_by_treesearch(Solver(), bare, max_predictions=4, check_holes=True)
    with pytest.raises(ValueError, match="is_random_network"):
        solve_by_treesearch(Solver(), bare, True, max_predictions=4)
    # the slot contract, on host tables
    DeviceTreeSweep.check_slots([0, 1], [0, 1], 4)               # each reuses its own parent, named once
    DeviceTreeSweep.check_slots([0, 0], [1, 2], 4)               # two children of one parent in fresh slots
    for parents, children in (([0, 0], [0, 1]), ([0, 1], [1, 2]), ([0, 1], [2, 2]), ([0], [4]), ([-1], [0])):
        with pytest.raises(ValueError, match="DeviceTreeSweep"):
            DeviceTreeSweep.check_slots(parents, children, 4)


def test_workspace_formula_and_declared_symbols():
    from tilingnn_amd import _lib
    assert "tgnn_tree_sweep_many" in _lib.EXPORTED_SYMBOLS and "tgnn_tree_sweep_workspace_bytes" in _lib.EXPORTED_SYMBOLS
    assert _lib.lib.tgnn_tree_sweep_workspace_bytes(0) == 0 and _lib.lib.tgnn_tree_sweep_workspace_bytes(-3) == 0
    assert [_lib.lib.tgnn_tree_sweep_workspace_bytes(k) for k in (1, 9, 70000)] == [4, 36, 280000]
