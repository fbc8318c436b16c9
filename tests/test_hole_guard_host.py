"""The guarded greedy sweep restated on the host (tests/hole_guard_restatement.py) on the small complete graph: what
tests/test_hole_guard_solve.py compares the real loop with, checked here on its own -- the counts measured when the guard was
designed, as a cross-check of the recipe, and the invariant the guard exists for: no hole, whatever the seed.  (Ring 9 costs
about a minute a seed on the host: the GPU test quotes its figures instead.)"""
import os

import numpy as np
import pytest

from tests import hole_guard_restatement as hg
from tests.golden_util import GOLDEN

SEEDS = tuple(range(8))
QUOTED_SELECTED = (42, 40, 43, 42, 41, 43, 40, 40)
QUOTED_ROUNDS = (13, 14, 20, 15, 16, 21, 20, 19)


@pytest.fixture(scope="module")
def small():
    from tilingnn_amd.tiling.tile_graph import TileGraph
    g = TileGraph(2)
    g.load_graph_state(os.path.join(GOLDEN, "complete_graph_small.pkl"), sidecar=False)
    return [np.asarray(t.tile_poly.exterior)[:-1] for t in g.tiles], g.arrays.colli_edges


def test_guarded_sweep_on_the_small_graph(small):
    rings, col = small
    assert len(rings) == 150
    runs = [hg.solve(rings, col, seed) for seed in SEEDS]
    print("\nhole guard restated, small graph: selected", [int(r.selection.sum()) for r in runs], "rounds", [r.rounds for r in runs],
          "vetoes", [r.vetoes for r in runs])
    for seed, r in zip(SEEDS, runs):
        sel = r.selection == 1
        assert r.topology == (1, 0), seed
        assert not (sel[col[0]] & sel[col[1]]).any() and sorted(r.order) == np.flatnonzero(sel).tolist()
        assert 33 <= r.vetoes <= 122, (seed, r.vetoes)
    assert tuple(int(r.selection.sum()) for r in runs) == QUOTED_SELECTED
    assert tuple(r.rounds for r in runs) == QUOTED_ROUNDS


def test_the_unguarded_restatement_draws_the_same_stream(small):
    """guarded=False is the plain sweep: the same code with the veto off selects a maximal collision-free set."""
    rings, col = small
    r = hg.solve(rings, col, 0, guarded=False)
    sel = r.selection == 1
    blocked = sel.copy()
    blocked[col[1][sel[col[0]]]] = True
    assert r.vetoes == 0 and blocked.all() and not (sel[col[0]] & sel[col[1]]).any()
