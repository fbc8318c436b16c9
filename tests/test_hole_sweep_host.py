"""Host side of the device hole sweep (csrc/hole_sweep.hip): the per-visit steps of csrc/hole_sweep_step.h run on the host under
sanitizers as the guarded walk of one layout, over EVERY visiting order of three hand-made sets at three rotations with scripted
thresholds and draws, against the subset tables of the loop-tracing oracle (tests/hole_delta_cases.py) -- d holes at every visit,
the label invariant after every acceptance (both checked by the program), and per order the positions reached, vetoes, draws,
acceptances, killed nodes and final selection against the walk written out again here from the table alone.  Then what the
host side of the sweep relies on: numpy's batch draw and rewind against scalar draws, and the restated guarded solve fed
pre-drawn uniforms."""
import itertools
import math
import os

import numpy as np
import pytest

from tests import hole_delta_cases as hc
from tests import hole_guard_restatement as hg
from tests import topology_oracle as to
from tests.golden_util import GOLDEN
from tests.sweep_host_cases import NBR, SETS, build_step_program, run_program

THR = (1.0, 0.5, 0.75, 1.0, 0.25, 1.0, 0.5, 1.0, 0.875)


@pytest.fixture(scope="module")
def step_program(tmp_path_factory):
    return build_step_program(tmp_path_factory, "hole_sweep_step_test")


def _run(exe, tmp_path, tiles, want, orders):
    tail, out = run_program(exe, tmp_path, tiles, want, orders, THR)
    assert tail[0::2] == ["orders", "visits", "evaluated", "mismatches", "err", "hits"] and tail[7] == "0" and tail[9] == "0", tail
    assert int(tail[1]) == orders.shape[0]
    return out.reshape(-1, 6), int(tail[3]), int(tail[5]), int(tail[11])


def _walk_from_the_table(n, want, orders):
    """The guarded walk of every order at once from the oracle's table alone: [orders, 6] as the program writes them."""
    count = orders.shape[0]
    row = np.arange(count)
    holes = want[:, 1].astype(np.int64)
    mask = np.zeros(count, dtype=np.int64)
    unl = np.ones((count, n), dtype=bool)
    running = np.ones(count, dtype=bool)
    reached, vetoes, draws, accepted, killed = (np.zeros(count, dtype=np.int64) for _ in range(5))
    for step in range(2 * n):                                    # two rounds, the second backwards, the state carried over
        pos = step if step < n else 2 * n - 1 - step
        if step == n:
            running[:] = True
        t = orders[:, pos].astype(np.int64)
        reached[running] += 1
        running &= unl[row, t]                                   # the break
        d = holes[mask | (1 << t)] - holes[mask]
        veto = running & (d > 0)
        vetoes[veto] += 1
        draw = running & ~veto
        u = ((7 * row + 13 * draws) % 32) / 32.0
        draws[draw] += 1
        acc = draw & (THR[pos] > u)
        accepted[acc] += 1
        unl[row[acc], t[acc]] = False
        mask[acc] |= 1 << t[acc]
        for node, nbrs in NBR[n].items():
            for v in dict.fromkeys(nbrs):
                hit = acc & (t == node) & unl[:, v]
                killed[hit] += 1
                unl[hit, v] = False
    return np.stack([reached, vetoes, draws, accepted, killed, mask], axis=1)


def test_the_walk_on_the_host_every_visiting_order(step_program, tmp_path):
    sets = hc.sets()
    for name in SETS:
        tiles = sets[name]
        n = len(tiles)
        want, _ = hc.subset_table(name, tiles)
        orders = np.array(list(itertools.permutations(range(n))), dtype=np.uint8)
        assert orders.shape[0] == math.factorial(n)
        expect = _walk_from_the_table(n, want, orders)
        # kills and breaks in every set; vetoes wherever a tile can close a gap (the plus among its four squares never does)
        assert (expect[:, 4] > 0).any() and (expect[:, 0] < 2 * n).any()
        assert (expect[:, 1] > 0).any() == (name != "plus among four squares")
        assert (expect[:, 2] < expect[:, 0]).any() and (expect[:, 3] < expect[:, 2]).any()             # draws saved, rejections
        for angle in to.ROTATIONS:
            got, visits, evaluated, hits = _run(step_program, tmp_path, to.rotated(tiles, angle), want, orders)
            assert np.array_equal(got, expect), (name, angle, np.flatnonzero((got != expect).any(axis=1))[:5])
            assert evaluated > 0 and visits >= evaluated
            assert hits > 0 or n < 9                                  # the cache answered visits (in the small sets every tile touches most others)
        print(f"\nhole sweep host: {name}: {orders.shape[0]} orders, {int(expect[:, 0].sum())} positions, {int(expect[:, 1].sum())} "
              f"vetoes, {int(expect[:, 2].sum())} draws, {int(expect[:, 3].sum())} accepted, {int(expect[:, 4].sum())} killed")


# ------------------------------------------------------------------------------------------------ the RNG hand-over
@pytest.mark.parametrize("consumed", [0, 1, 7, 50])
def test_batch_draw_and_rewind_is_scalar_draws(consumed):
    """DeviceHoleSweep draws a round's uniforms in one call, and afterwards rewinds and draws only what the walk consumed: the
    values and the generator's state afterwards must be those of scalar draws, for the global stream and for RandomState."""
    scalar = np.random.RandomState(11)
    one_by_one = np.array([scalar.uniform() for _ in range(50)])
    batch = np.random.RandomState(11)
    state = batch.get_state()
    assert batch.uniform(size=50).tobytes() == one_by_one.tobytes()
    batch.set_state(state)
    batch.uniform(size=consumed)
    after = np.random.RandomState(11)
    for _ in range(consumed):
        after.uniform()
    assert batch.uniform() == after.uniform()
    a, b = batch.get_state(), after.get_state()
    assert a[0] == b[0] and np.array_equal(a[1], b[1]) and a[2:] == b[2:]
    # the global generator
    np.random.seed(11)
    state = np.random.get_state()
    assert np.random.uniform(size=50).tobytes() == one_by_one.tobytes()
    np.random.set_state(state)
    np.random.uniform(size=consumed)
    a = np.random.get_state()
    np.random.seed(11)
    for _ in range(consumed):
        np.random.uniform()
    b = np.random.get_state()
    assert a[0] == b[0] and np.array_equal(a[1], b[1]) and a[2:] == b[2:]


def test_restated_solve_fed_pre_drawn_uniforms(monkeypatch):
    """tests/hole_guard_restatement.py draws one uniform per test; fed from a batch drawn ahead it gives the same solve."""
    from tilingnn_amd.tiling.tile_graph import TileGraph
    g = TileGraph(2)
    g.load_graph_state(os.path.join(GOLDEN, "complete_graph_small.pkl"), sidecar=False)
    rings = [np.asarray(t.tile_poly.exterior)[:-1] for t in g.tiles]
    col = g.arrays.colli_edges
    want = hg.solve(rings, col, 3)
    real = np.random.RandomState

    class PreDrawn:
        def __init__(self, seed):
            self.values, self.used = real(seed).uniform(size=100000), 0

        def uniform(self):
            self.used += 1
            return self.values[self.used - 1]

    monkeypatch.setattr(np.random, "RandomState", PreDrawn)
    got = hg.solve(rings, col, 3)
    assert np.array_equal(got.selection, want.selection) and got.order == want.order
    assert (got.rounds, got.vetoes, got.topology) == (want.rounds, want.vetoes, want.topology) and want.vetoes > 0


# ------------------------------------------------------------------------------------------------ refusals that need no GPU
def test_device_sweep_needs_check_holes():
    import torch
    from tilingnn_amd.util.algorithms import DeviceLayout, solve_by_probablistic_greedy

    class Solver:
        device = torch.device("cpu")

    z = torch.zeros
    bare = DeviceLayout(z(3, 1), z(2, 0, dtype=torch.int64), z(0, 1), z(2, 0, dtype=torch.int64))
    with pytest.raises(ValueError, match="device_sweep"):
        solve_by_probablistic_greedy(Solver(), bare, device_sweep=True)


def test_workspace_formula_and_declared_symbols():
    from tilingnn_amd import _lib
    assert "tgnn_hole_sweep_many" in _lib.EXPORTED_SYMBOLS and "tgnn_hole_sweep_workspace_bytes" in _lib.EXPORTED_SYMBOLS
    assert _lib.lib.tgnn_hole_sweep_workspace_bytes(0) == 0 and _lib.lib.tgnn_hole_sweep_workspace_bytes(-3) == 0
    assert [_lib.lib.tgnn_hole_sweep_workspace_bytes(k) for k in (1, 9, 70000)] == [4, 36, 280000]
