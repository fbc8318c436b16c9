"""Host side of the per-candidate hole deltas (csrc/union_hole_delta.hip): the kernel's per-candidate code
(csrc/union_hole_delta_point.h: delta_chi and the label-count rule) run on the host under sanitizers over every subset x every
outside tile of fifteen hand-made sets at three rotations, against the loop-tracing oracle of tests/topology_oracle.py; and the
refusals of the bindings that need no GPU.  The GPU tests (tests/test_union_hole_delta_gpu.py) lean on the same tables."""
import math
import os
import shutil
import struct
import subprocess

import numpy as np
import pytest
import torch

from tests import hole_delta_cases as hc
from tests import topology_oracle as to
from tests.golden_util import GOLDEN


@pytest.fixture(scope="module")
def delta_program(tmp_path_factory):
    """tests/host/union_hole_delta_test.cpp, built with the host compiler alone under AddressSanitizer + UBSan (the sanitizers'
    runtime linked into the program itself), the way tests/test_union_topology_host.py builds its program."""
    repo = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    cxx = os.environ.get("CXX") or shutil.which("g++") or shutil.which("c++") or shutil.which("clang++")
    assert cxx, "no host C++ compiler"
    clang = "clang" in subprocess.run([cxx, "--version"], capture_output=True, text=True).stdout
    static_rt = ["-static-libsan"] if clang else ["-static-libasan", "-static-libubsan"]
    exe = str(tmp_path_factory.mktemp("hole_delta") / "union_hole_delta_test")
    build = subprocess.run([cxx, "-std=c++17", "-O1", "-g", "-Wall", "-Wextra", "-Werror", "-fsanitize=address,undefined",
                            "-fno-sanitize-recover=undefined", *static_rt, "-I", os.path.join(repo, "tilingnn_amd", "csrc"),
                            os.path.join(repo, "tests", "host", "union_hole_delta_test.cpp"), "-o", exe],
                           capture_output=True, text=True)
    assert build.returncode == 0, build.stderr[-4000:]
    return exe


def _run(exe, tmp_path, tiles, masks, delta):
    """{(dc, dh): count} as the host program computed them; it compares every pair with `delta` itself."""
    from tilingnn_amd.tiling.region import UNION_TOL, contact_geometry, sweep_direction, union_geometry
    n = len(tiles)
    ring_xy, ring_ptr, _, _ = union_geometry(tiles, np.zeros((2, 0), dtype=np.int64), n)
    touch_ptr, touch_idx = contact_geometry(ring_xy, ring_ptr)
    theta = sweep_direction(ring_xy, ring_ptr)
    path = str(tmp_path / "case.bin")
    with open(path, "wb") as f:
        f.write(struct.pack("<4q3d", n, ring_xy.shape[0], touch_idx.shape[0], masks.shape[0], UNION_TOL, math.cos(theta),
                            math.sin(theta)))
        for a in (ring_xy, ring_ptr, touch_ptr, touch_idx, masks.astype(np.int32), delta.astype(np.int32)):
            f.write(np.ascontiguousarray(a).tobytes())
    run = subprocess.run([exe, path], capture_output=True, text=True)
    assert run.returncode == 0, (run.stdout + run.stderr)[-4000:]
    lines = run.stdout.strip().split("\n")
    tail = lines[-1].split()
    assert tail[0] == "pairs" and tail[2:] == ["mismatches", "0", "err", "0"], lines[-1]
    seen = {(int(a), int(b)): int(c) for a, b, c in (l.split() for l in lines[:-1])}
    assert sum(seen.values()) == int(tail[1]) == int((masks == 0).sum())
    return seen


def test_new_sets_by_hand():
    """The three sets added for d holes < 0, whole: the counts worked out by hand."""
    sets = hc.sets()
    assert len(sets) == 15 and max(len(t) for t in sets.values()) <= 10
    for angle in to.ROTATIONS:
        assert to.topology(to.rotated(sets["3x3 full"], angle)) == (1, 0)
        assert to.topology(to.rotated(sets["plus among four squares"], angle)) == (1, 0)
        assert to.topology(to.rotated(sets["frame with a plus inside"], angle)) == (1, 4)     # the plus cuts the 3 x 3 inside in four
    ring = [t for i, t in enumerate(sets["3x3 full"]) if i != 4]
    assert to.topology(ring) == (1, 1)                                                   # ... whose centre closes the hole
    want, delta = hc.subset_table("3x3 full", sets["3x3 full"])
    assert delta[0b111101111, 4].tolist() == [0, -1]


def test_delta_chi_and_label_rule_on_the_host_every_subset(delta_program, tmp_path):
    total, seen_all = 0, {}
    for name, tiles in hc.sets().items():
        n = len(tiles)
        masks = hc.all_subsets(n)
        want, delta = hc.subset_table(name, tiles)
        table = hc.pair_counts(delta, masks)
        for angle in to.ROTATIONS:
            seen = _run(delta_program, tmp_path, to.rotated(tiles, angle), masks, delta)
            assert seen == table, (name, angle)
        total += sum(table.values())
        for pair, count in table.items():
            seen_all[pair] = seen_all.get(pair, 0) + count
    print(f"\nunion_hole_delta host: {total} (subset, tile) pairs per rotation, {dict(sorted(seen_all.items()))}")
    twelve = set()
    for name, (tiles, _) in to.hand_sets().items():
        twelve |= set(hc.pair_counts(hc.subset_table(name, tiles)[1], hc.all_subsets(len(tiles))))
    assert min(dh for _, dh in twelve) == 0                  # the twelve alone never close a hole: why three sets were added
    assert set(seen_all) == hc.PAIRS
    # sum over the sets of n 2^(n - 1): every set of two tiles or more gives an even count and exactly one set has one tile
    assert total == sum(len(t) * 2 ** (len(t) - 1) for t in hc.sets().values()) == 12365


# ------------------------------------------------------------------------------------------------ no GPU, no answer
def _small_graph():
    from tilingnn_amd.tiling.tile_graph import TileGraph
    g = TileGraph(2)
    g.load_graph_state(os.path.join(GOLDEN, "complete_graph_small.pkl"), sidecar=False)
    return g


def test_hole_deltas_refuses_without_a_gpu(monkeypatch):
    from tilingnn_amd.tiling.brick_layout import BrickLayout
    from tilingnn_amd.util import data_util as du
    g = _small_graph()
    layout = BrickLayout(g, *du.create_brick_layout_from_super_set(g, [0, 1, 2, 3]))
    monkeypatch.setattr(torch.cuda, "is_available", lambda: False)              # (on a GPU box too: the refusal is what is tested)
    with pytest.raises(RuntimeError, match="no host fallback"):
        layout.hole_deltas()
    with pytest.raises(RuntimeError, match="no host fallback"):
        layout.hole_deltas(selection=np.zeros(4))


def test_check_holes_needs_the_complete_graph():
    """A DeviceLayout has no complete graph: check_holes=True is refused before anything runs (no GPU needed to say so)."""
    from tilingnn_amd.util.algorithms import DeviceLayout, solve_by_probablistic_greedy

    class Solver:
        device = torch.device("cpu")

    z = torch.zeros
    bare = DeviceLayout(z(3, 1), z(2, 0, dtype=torch.int64), z(0, 1), z(2, 0, dtype=torch.int64))
    with pytest.raises(ValueError, match="complete graph"):
        solve_by_probablistic_greedy(Solver(), bare, check_holes=True)
