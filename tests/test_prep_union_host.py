"""tgnn_graph_prep_small_many without a GPU: the exports, their declarations, the Python options, and the planner that gives every
layout its team of blocks and splits the teams of a call into launches (csrc/graph_prep.hip: small_prep_blocks / small_prep_plan
behind tgnn_graph_prep_small_many_plan)."""
import inspect
import os
import re

import pytest

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ("tgnn_graph_prep_small_many", "tgnn_graph_prep_small_many_wait", "tgnn_graph_prep_small_many_plan",
         "tgnn_graph_prep_small_many_counts")


def _plan(layouts, capacity):
    """layouts: (ea, ec, n) each -> (blocks, groups, n_groups)"""
    from tilingnn_amd import _lib
    return _lib.graph_prep_small_many_plan([l[0] for l in layouts], [l[1] for l in layouts], [l[2] for l in layouts], capacity)


def test_the_library_exports_and_the_header_declares_the_four_entries():
    from tilingnn_amd import _lib
    with open(os.path.join(REPO, "include", "tgnn.h")) as f:
        header = f.read()
    for name in NAMES:
        assert getattr(_lib.lib, name) is not None
        assert name in _lib.EXPORTED_SYMBOLS
        assert re.search(r"\b(int|void)\s+" + name + r"\s*\(", header), name
    assert re.search(r"typedef\s+struct\s+tgnn_small_prep_layout\b", header)


def test_the_python_options_exist_and_default_to_off():
    from tilingnn_amd import TilinGNN, ops
    from tilingnn_amd.solver.ml_solver.ml_solver import ML_Solver
    assert inspect.signature(TilinGNN.forward_many).parameters["union_prep"].default is False
    assert ML_Solver(None, "cpu", None, None, num_prob_maps=1).union_prep is False
    assert callable(ops.prepare_graphs_small)


def test_the_pinned_solver_signatures_are_unchanged():
    from tilingnn_amd.solver.ml_solver.ml_solver import ML_Solver
    from tilingnn_amd.util import algorithms as alg
    assert list(inspect.signature(alg.solve_many_by_device_greedy).parameters) == \
        ["ml_solver", "layouts", "seed", "seeds", "score_fn", "max_rounds", "streams"]
    assert list(inspect.signature(ML_Solver.solve_many).parameters) == ["self", "brick_layouts", "seed"]


def test_team_sizes_are_the_solo_launchers():
    """max(ceil(max(ea, ec) / 2048), ceil(ea / 8192), 1), at most 16."""
    cases = [(1, 1), (2048, 0), (2049, 0), (0, 4097), (8193, 10), (131072, 131072)]
    blocks, groups, n_groups = _plan([(ea, ec, 100) for ea, ec in cases], 240)
    assert blocks == [1, 1, 2, 3, 5, 16]
    assert groups == [0] * 6 and n_groups == 1


@pytest.mark.parametrize("bad", [(10, 10, 4097), (131073, 10, 100), (10, 131073, 100)])
def test_a_layout_the_solo_call_rejects_by_size_stays_out_and_does_not_split_its_neighbours(bad):
    blocks, groups, n_groups = _plan([(5000, 10, 300), bad, (5000, 10, 300)], 240)
    assert groups == [0, -1, 0] and n_groups == 1
    assert blocks == [3, 0, 3]


def test_20_layouts_of_16_blocks_at_capacity_240_give_15_and_5():
    blocks, groups, n_groups = _plan([(131072, 0, 4096)] * 20, 240)
    assert blocks == [16] * 20
    assert n_groups == 2 and groups == [0] * 15 + [1] * 5


def test_capacity_16_gives_one_layout_per_group():
    blocks, groups, n_groups = _plan([(131072, 0, 4096), (40000, 40000, 4096), (9, 9, 9), (3000, 100, 50)], 16)
    assert blocks == [16, 16, 1, 2]                              # (20 blocks' worth of edges: capped at 16)
    assert groups == [0, 1, 2, 2] and n_groups == 3              # greedy: 1 + 2 blocks share a launch, a 16-block team never does
    blocks, groups, n_groups = _plan([(131072, 0, 4096)] * 4, 16)
    assert groups == [0, 1, 2, 3] and n_groups == 4


def test_no_layouts_negative_counts_and_a_capacity_below_one_team_are_errors():
    from tilingnn_amd import _lib
    with pytest.raises(ValueError):
        _plan([], 240)
    with pytest.raises(ValueError):
        _plan([(-1, 0, 10)], 240)
    with pytest.raises(ValueError):
        _plan([(10, 10, -3)], 240)
    with pytest.raises(ValueError):
        _plan([(10, 10, 10)], 15)
    assert _lib.lib.tgnn_graph_prep_small_many_plan(None, None, None, 0, 240, None, None) < 0
