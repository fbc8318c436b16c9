"""tgnn_forward_union without a GPU: the exports, their declarations, and the planner that splits the eligible layouts of a
call into persistent launches (csrc/forward_small.hip: small_union_plan behind tgnn_forward_union_plan)."""
import inspect
import os
import re

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ("tgnn_forward_union", "tgnn_forward_union_plan", "tgnn_forward_union_counts")


def test_the_library_exports_and_the_header_declares_the_union_entries():
    from tilingnn_amd import _lib
    with open(os.path.join(REPO, "include", "tgnn.h")) as f:
        header = f.read()
    for name in NAMES:
        assert getattr(_lib.lib, name) is not None
        assert name in _lib.EXPORTED_SYMBOLS
        assert re.search(r"\b(int|void)\s+" + name + r"\s*\(", header), name


def test_the_python_options_exist_and_default_to_off():
    from tilingnn_amd import TilinGNN
    from tilingnn_amd.solver.ml_solver.ml_solver import ML_Solver
    from tilingnn_amd.util import algorithms as alg
    assert inspect.signature(TilinGNN.forward_many).parameters["union"].default is False
    # the solves take the option from the solver (an attribute like device_greedy_seed): their signatures stay as they were
    assert "union_forward" not in inspect.signature(alg.solve_many_by_device_greedy).parameters
    assert "union_forward" not in inspect.signature(ML_Solver.solve_many).parameters
    assert ML_Solver(None, "cpu", None, None, num_prob_maps=1).union_forward is False


def _blocks(n):
    return (n + 15) // 16


def _check(sizes, capacity, groups, n_groups):
    """What every plan must satisfy: order-preserving (non-decreasing, consecutive numbers from 0), within capacity, greedy (a
    layout opens a new group only where it does not fit the current one)."""
    assert len(groups) == len(sizes)
    live = [(g, _blocks(n)) for g, n in zip(groups, sizes) if g >= 0]
    assert [g for g, _ in live] == sorted(g for g, _ in live)
    assert sorted(set(g for g, _ in live)) == list(range(n_groups))
    used = [0] * n_groups
    for g, b in live:
        if used[g] == 0 and g > 0:
            assert used[g - 1] + b > capacity                 # greedy: it did not fit the group before
        used[g] += b
    assert all(0 < u <= capacity for u in used)


def test_24_layouts_of_170_nodes_at_capacity_240():
    """170 nodes are 11 tiles of 16 rows (the team of a union launch is the solo grid), so 21 of them fill 231 of 240 blocks: 21 + 3.
    (Twelve-block layouts give the 20 + 4 split: the next test.)"""
    from tilingnn_amd import _lib
    assert _blocks(170) == 11
    groups, n_groups = _lib.forward_union_plan([170] * 24, 240)
    assert n_groups == 2 and groups == [0] * 21 + [1] * 3
    _check([170] * 24, 240, groups, n_groups)


def test_crop_sized_layouts_of_12_blocks_give_groups_of_20_and_4():
    from tilingnn_amd import _lib
    sizes = [180] * 24                                         # 12 blocks each: 20 x 12 = 240
    assert _blocks(180) == 12
    groups, n_groups = _lib.forward_union_plan(sizes, 240)
    assert n_groups == 2 and groups == [0] * 20 + [1] * 4
    _check(sizes, 240, groups, n_groups)


def test_mixed_sizes_keep_order_and_capacity():
    from tilingnn_amd import _lib
    sizes = [1254, 17, 640, 2, 4096, 3000, 16, 33, 900, 1300, 170, 48]
    for capacity in (240, 256, 300, 80, 1000):
        groups, n_groups = _lib.forward_union_plan(sizes, capacity)
        _check(sizes, capacity, groups, n_groups)
        for n, g in zip(sizes, groups):
            assert (g == -1) == (_blocks(n) > capacity), (n, capacity)


def test_an_ineligible_layout_stays_out_and_does_not_split_its_neighbours():
    from tilingnn_amd import _lib
    assert _lib.lib.tgnn_get_small_layout_limit() >= 4096
    groups, n_groups = _lib.forward_union_plan([170, 4097, 170], 240)
    assert groups == [0, -1, 0] and n_groups == 1
    groups, n_groups = _lib.forward_union_plan([170, 4096, 170], 240)      # 256 tiles: more than the capacity
    assert groups == [0, -1, 0] and n_groups == 1
    groups, n_groups = _lib.forward_union_plan([1, 170, 0, 170], 240)      # train-mode BatchNorm needs two rows
    assert groups == [-1, 0, -1, 0] and n_groups == 1


def test_no_layouts_and_a_capacity_of_one():
    from tilingnn_amd import _lib
    assert _lib.forward_union_plan([], 240) == ([], 0)
    groups, n_groups = _lib.forward_union_plan([16] * 5, 1)
    assert groups == [0, 1, 2, 3, 4] and n_groups == 5
    groups, n_groups = _lib.forward_union_plan([16, 17, 16], 1)            # 17 nodes: two tiles
    assert groups == [0, -1, 1] and n_groups == 2
    assert _lib.forward_union_plan([16, 16], 0) == ([-1, -1], 0)
