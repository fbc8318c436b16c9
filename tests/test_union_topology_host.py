"""Host side of the union topology (csrc/union_topology.hip): the loop-tracing oracle of tests/topology_oracle.py against counts
worked out by hand and on the lattice fixtures, the contact relation against an all-pairs brute force, the sweep-direction
picker, the kernel's per-vertex code (csrc/union_topology_point.h) and the steps the union kernels share
(csrc/union_components.h) run on the host under sanitizers, and the refusal to run without a GPU.  The GPU tests (tests/test_union_topology_gpu.py) lean on every one of these."""
import gzip
import math
import os
import shutil
import struct
import subprocess

import numpy as np
import pytest
import torch

from tests import topology_oracle as to
from tests.golden_util import GOLDEN


def _load(which, tmp_path_factory):
    from tilingnn_amd.tiling.tile_graph import TileGraph
    g = TileGraph(2)
    if which == "small":
        g.load_graph_state(os.path.join(GOLDEN, "complete_graph_small.pkl"), sidecar=False)
    else:
        path = str(tmp_path_factory.mktemp("labyrinth") / "complete_graph_ring9.pkl")
        with gzip.open(os.path.join(GOLDEN, "complete_graph_ring9.pkl.gz"), "rb") as src, open(path, "wb") as dst:
            shutil.copyfileobj(src, dst)
        g.load_graph_state(path, sidecar=False)
    return g


@pytest.fixture(scope="module")
def graphs(tmp_path_factory):
    return {which: _load(which, tmp_path_factory) for which in ("small", "ring9")}


def _rings(g):
    return [np.asarray(t.tile_poly.exterior)[:-1] for t in g.tiles]


# ------------------------------------------------------------------------------------------------ the oracle
@pytest.mark.parametrize("angle", to.ROTATIONS)
def test_oracle_gives_the_hand_counts(angle):
    sets = to.hand_sets()
    assert len(sets) == 12
    for name, (tiles, want) in sets.items():
        assert to.topology(to.rotated(tiles, angle)) == want, (name, angle)


def test_oracle_is_indifferent_to_orientation_closing_and_order():
    tiles, want = to.hand_sets()["block ring, hexagon bridging the hole"]
    shuffled = [np.concatenate([t[::-1], t[-1:]]) for t in tiles[::-1]]          # clockwise, closed, reversed order
    assert to.topology(shuffled) == want
    assert to.topology([]) == (0, 0)


def test_oracle_refuses_overlapping_tiles():
    box = lambda x0, y0, x1, y1: np.array([[x0, y0], [x1, y0], [x1, y1], [x0, y1]], dtype=float)
    with pytest.raises(ValueError):
        to.topology([box(0, 0, 2, 1), box(0, 0, 1, 1)])                         # the side (0,0) -> (1,0) twice


@pytest.mark.parametrize("which", ["small", "ring9"])
@pytest.mark.parametrize("kind", ["independent", "thinned"])
def test_oracle_on_the_lattice_recipes(which, kind, graphs):
    """The counts quoted where the kernel was designed (topology_oracle.QUOTED), as a cross-check of the mask recipes."""
    g = graphs[which]
    rings, col = _rings(g), g.arrays.colli_edges
    make = to.independent_set if kind == "independent" else to.thinned_set
    got = [to.topology([rings[i] for i in np.flatnonzero(make(len(rings), col, seed))]) for seed in to.SEEDS]
    holes, comps = to.QUOTED[(which, kind)]
    print(f"\nunion_topology oracle {which} {kind}: holes {[h for _, h in got]}, components {[c for c, _ in got]}")
    assert tuple(h for _, h in got) == holes and tuple(c for c, _ in got) == comps


# ------------------------------------------------------------------------------------------------ the contact relation
def _brute_contacts(rings, tol):
    from tests.union_oracle import point_segment_distance
    n = len(rings)
    lo = np.array([r.min(axis=0) for r in rings]) - 1.0                           # (a generous box: this is the brute force)
    hi = np.array([r.max(axis=0) for r in rings]) + 1.0
    pairs = set()
    for i in range(n):
        for j in range(i + 1, n):
            if (lo[i] > hi[j]).any() or (lo[j] > hi[i]).any():
                continue
            near = False
            for u, v in ((i, j), (j, i)):
                a, b = rings[u], np.roll(rings[u], -1, axis=0)
                near = near or any(point_segment_distance(p, a[e], b[e]) <= tol for p in rings[v] for e in range(a.shape[0]))
            if near:
                pairs.update([(i, j), (j, i)])
    return pairs


def test_contact_geometry_against_brute_force(graphs):
    from tilingnn_amd.tiling.region import UNION_TOL, contact_geometry, union_geometry
    g = graphs["small"]
    n = len(g.tiles)
    ring_xy, ring_ptr, _, _ = union_geometry([t.tile_poly.exterior for t in g.tiles], g.arrays.colli_edges, n)
    touch_ptr, touch_idx = contact_geometry(ring_xy, ring_ptr)
    assert touch_ptr.dtype == np.int32 and touch_idx.dtype == np.int32 and touch_ptr.shape == (n + 1,)
    assert touch_ptr[0] == 0 and touch_ptr[-1] == touch_idx.shape[0] and (np.diff(touch_ptr) >= 0).all()
    rows = np.repeat(np.arange(n), np.diff(touch_ptr))
    got = set(zip(rows.tolist(), touch_idx.tolist()))
    assert len(got) == touch_idx.shape[0] and all(i != j for i, j in got) and all((j, i) in got for i, j in got)
    for i in range(n):
        row = touch_idx[touch_ptr[i]:touch_ptr[i + 1]]
        assert (np.diff(row) > 0).all()
    rings = [ring_xy[ring_ptr[i]:ring_ptr[i + 1]] for i in range(n)]
    assert got == _brute_contacts(rings, UNION_TOL)
    adj = g.arrays.adj_edges
    assert adj.shape[1] > 0 and all((int(a), int(b)) in got for a, b in adj.T if a != b)
    # ... and the two edge lists together are NOT the contact relation: corner contacts are in neither
    col = g.arrays.colli_edges
    listed = set(zip(adj[0].tolist(), adj[1].tolist())) | set(zip(col[0].tolist(), col[1].tolist()))
    assert got - listed


def test_contact_geometry_degenerate_inputs():
    from tilingnn_amd.tiling.region import contact_geometry
    ptr, idx = contact_geometry(np.zeros((0, 2)), np.zeros(1, dtype=np.int32))
    assert ptr.tolist() == [0] and idx.shape == (0,)
    tri = np.array([[0, 0], [1, 0], [0, 1]], dtype=float)
    ptr, idx = contact_geometry(np.concatenate([tri, tri + [5, 5], tri + [1, 0]]), np.array([0, 3, 6, 9], dtype=np.int32))
    assert ptr.tolist() == [0, 1, 1, 2] and idx.tolist() == [2, 0]               # 0 and 2 share the corner (1, 0)
    with pytest.raises(ValueError):
        contact_geometry(tri[:2], np.array([0, 2], dtype=np.int32))


# ------------------------------------------------------------------------------------------------ the sweep direction
def _geometry(tiles):
    from tilingnn_amd.tiling.region import union_geometry
    return union_geometry(tiles, np.zeros((2, 0), dtype=np.int64), len(tiles))[:2]


def test_sweep_direction_accepts_the_first_candidate_for_both_fixtures(graphs):
    from tilingnn_amd.tiling.region import SWEEP_CANDIDATES, side_directions, sweep_direction
    assert SWEEP_CANDIDATES[0] == 0.1234
    for which in ("small", "ring9"):
        ring_xy, ring_ptr = _geometry(_rings(graphs[which]))
        dirs = side_directions(ring_xy, ring_ptr)
        off = np.mod(dirs - 0.1234, math.pi)
        nearest = float(np.minimum(off, math.pi - off).min())
        print(f"\nunion_topology {which}: {dirs.size} side directions (mod pi), the nearest {nearest:.4f} rad from 0.1234")
        # the lattice's sides run along the multiples of 30 degrees: the nearest is the one along 0
        assert np.allclose(np.mod(dirs + 1e-3, math.pi / 6), 1e-3, atol=1e-6)
        assert 0.123 < nearest < 0.124 and sweep_direction(ring_xy, ring_ptr) == 0.1234


def test_sweep_direction_moves_on_and_gives_up():
    from tilingnn_amd.tiling.region import SWEEP_CANDIDATES, SWEEP_MIN_GAP, sweep_direction
    square = [np.array([[0, 0], [1, 0], [1, 1], [0, 1]], dtype=float)]
    assert sweep_direction(*_geometry(square)) == SWEEP_CANDIDATES[0]
    for miss in (0.0, 0.5 * SWEEP_MIN_GAP, -0.5 * SWEEP_MIN_GAP):               # a side on, or nearly on, the first level lines
        assert sweep_direction(*_geometry(to.rotated(square, SWEEP_CANDIDATES[0] + miss))) == SWEEP_CANDIDATES[1]
    assert sweep_direction(*_geometry(to.rotated(square, SWEEP_CANDIDATES[0] + 2.0 * SWEEP_MIN_GAP))) == SWEEP_CANDIDATES[0]
    # the square's other side direction blocks too
    assert sweep_direction(*_geometry(to.rotated(square, SWEEP_CANDIDATES[0] - math.pi / 2))) == SWEEP_CANDIDATES[1]
    # one thin triangle along every candidate: nothing is left
    fan = [np.array([[0, 0], [math.cos(t), math.sin(t)], [math.cos(t + 0.05), math.sin(t + 0.05)]]) for t in SWEEP_CANDIDATES]
    with pytest.raises(ValueError, match="candidate"):
        sweep_direction(*_geometry(fan))
    with pytest.raises(ValueError, match="candidate"):
        sweep_direction(*_geometry(square), candidates=(0.0, math.pi / 2))


def test_side_directions_too_close_are_refused():
    from tilingnn_amd.tiling.region import sweep_direction
    a = np.array([[0, 0], [1, 0], [0, 1]], dtype=float)
    b = to.rotated([a], 2e-4)[0] + [5.0, 0.0]
    with pytest.raises(ValueError, match="apart"):
        sweep_direction(*_geometry([a, b]))
    same = to.rotated([a], 1e-7)[0] + [5.0, 0.0]                                  # within the tolerance: one direction
    assert sweep_direction(*_geometry([a, same])) == 0.1234


# ------------------------------------------------------------------------------------------------ the kernel's local term
def _build_host_program(tmp_path_factory, name):
    """tests/host/<name>.cpp built with the host compiler alone under AddressSanitizer + UBSan (the sanitizers' runtime linked
    into the program itself)."""
    repo = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    cxx = os.environ.get("CXX") or shutil.which("g++") or shutil.which("c++") or shutil.which("clang++")
    assert cxx, "no host C++ compiler"
    clang = "clang" in subprocess.run([cxx, "--version"], capture_output=True, text=True).stdout
    static_rt = ["-static-libsan"] if clang else ["-static-libasan", "-static-libubsan"]
    exe = str(tmp_path_factory.mktemp(name) / name)
    build = subprocess.run([cxx, "-std=c++17", "-O1", "-g", "-Wall", "-Wextra", "-Werror", "-fsanitize=address,undefined",
                            "-fno-sanitize-recover=undefined", *static_rt, "-I", os.path.join(repo, "tilingnn_amd", "csrc"),
                            os.path.join(repo, "tests", "host", name + ".cpp"), "-o", exe],
                           capture_output=True, text=True)
    assert build.returncode == 0, build.stderr[-4000:]
    return exe


@pytest.fixture(scope="module")
def point_program(tmp_path_factory):
    """tests/host/union_topology_point_test.cpp: the header the kernel runs per vertex."""
    return _build_host_program(tmp_path_factory, "union_topology_point_test")


@pytest.fixture(scope="module")
def components_program(tmp_path_factory):
    """tests/host/union_components_test.cpp: the collision-row test and the labelling step the union kernels share."""
    return _build_host_program(tmp_path_factory, "union_components_test")


def _run_on_case(exe, tmp_path, tiles, masks):
    """Writes tiles, contact rows and masks to a file, runs the host program on it; (output words, masks, touch_ptr, touch_idx)."""
    from tilingnn_amd.tiling.region import UNION_TOL, contact_geometry, sweep_direction, union_geometry
    n = len(tiles)
    ring_xy, ring_ptr, _, _ = union_geometry(tiles, np.zeros((2, 0), dtype=np.int64), n)
    touch_ptr, touch_idx = contact_geometry(ring_xy, ring_ptr)
    theta = sweep_direction(ring_xy, ring_ptr)
    masks = np.ascontiguousarray(np.asarray(masks).reshape(-1, n), dtype=np.int32)
    path = str(tmp_path / "case.bin")
    with open(path, "wb") as f:
        f.write(struct.pack("<4q3d", n, ring_xy.shape[0], touch_idx.shape[0], masks.shape[0], UNION_TOL, math.cos(theta),
                            math.sin(theta)))
        for a in (ring_xy, ring_ptr, touch_ptr, touch_idx, masks):
            f.write(np.ascontiguousarray(a).tobytes())
    run = subprocess.run([exe, path], capture_output=True, text=True)
    assert run.returncode == 0, (run.stdout + run.stderr)[-4000:]
    return run.stdout.split(), masks, touch_ptr, touch_idx


def _components(m, touch_ptr, touch_idx):
    """The components of mask m by a union-find over the contact rows."""
    parent = list(range(m.shape[0]))

    def find(a):
        while parent[a] != a:
            parent[a] = parent[parent[a]]
            a = parent[a]
        return a
    for i in np.flatnonzero(m):
        for j in touch_idx[touch_ptr[i]:touch_ptr[i + 1]]:
            if m[j]:
                parent[find(i)] = find(int(j))
    return len({find(i) for i in np.flatnonzero(m)})


def _host_topology(exe, tmp_path, tiles, masks):
    """[(components, holes)] per mask: chi from the host program, components by a union-find over the contact rows."""
    lines, masks, touch_ptr, touch_idx = _run_on_case(exe, tmp_path, tiles, masks)
    assert lines[-2:] == ["err", "0"], lines[-2:]
    chi = [int(v) for v in lines[:-2]]
    assert len(chi) == masks.shape[0]
    out = []
    for m, c in zip(masks, chi):
        comps = _components(m, touch_ptr, touch_idx)
        out.append((comps, comps - c))
    return out


def test_local_euler_terms_on_the_host_hand_sets(point_program, tmp_path):
    for name, (tiles, want) in to.hand_sets().items():
        for angle in to.ROTATIONS:
            assert _host_topology(point_program, tmp_path, to.rotated(tiles, angle), [np.ones(len(tiles))]) == [want], (name, angle)


@pytest.mark.parametrize("which", ["small", "ring9"])
def test_local_euler_terms_on_the_host_lattice(which, graphs, point_program, tmp_path):
    g = graphs[which]
    rings, col = _rings(g), g.arrays.colli_edges
    masks = [make(len(rings), col, seed) for make in (to.independent_set, to.thinned_set) for seed in to.SEEDS]
    holes = to.QUOTED[(which, "independent")][0] + to.QUOTED[(which, "thinned")][0]
    comps = to.QUOTED[(which, "independent")][1] + to.QUOTED[(which, "thinned")][1]
    assert _host_topology(point_program, tmp_path, rings, masks) == list(zip(comps, holes))


# ------------------------------------------------------------------------------------------------ the kernels' shared steps
def _host_labelling(exe, tmp_path, tiles, masks):
    """Runs tests/host/union_components_test.cpp; checks the component count of every mask against the union-find and the number
    of sweeps against the round cap of the kernels (n_tiles + 1).  Returns the sweep counts and the program's `collides` lines."""
    lines, masks, touch_ptr, touch_idx = _run_on_case(exe, tmp_path, tiles, masks)
    k, n = masks.shape
    assert lines[2 * k:2 * k + 2] == ["err", "0"], lines[2 * k:2 * k + 2]
    comps, sweeps = [int(v) for v in lines[0:2 * k:2]], [int(v) for v in lines[1:2 * k:2]]
    assert comps == [_components(m, touch_ptr, touch_idx) for m in masks]
    assert all(1 <= s <= n + 1 for s in sweeps), (max(sweeps), n)
    rest = lines[2 * k + 2:]
    assert len(rest) % 6 == 0 and set(rest[0::6]) == {"collides"}
    return sweeps, [tuple(int(v) for v in rest[q + 1:q + 6]) for q in range(0, len(rest), 6)]


def test_labelling_step_on_the_host_hand_sets(components_program, tmp_path):
    for name, (tiles, want) in to.hand_sets().items():
        n = len(tiles)
        subsets = ((np.arange(2 ** n)[:, None] >> np.arange(n)[None, :]) & 1).astype(np.int32)
        _host_labelling(components_program, tmp_path, tiles, subsets)
        lines, _, _, _ = _run_on_case(components_program, tmp_path, tiles, [np.ones(n)])
        assert int(lines[0]) == want[0], name                               # all tiles: the count worked out by hand


@pytest.mark.parametrize("which", ["small", "ring9"])
def test_labelling_step_on_the_host_lattice(which, graphs, components_program, tmp_path):
    g = graphs[which]
    rings, col = _rings(g), g.arrays.colli_edges
    masks = [make(len(rings), col, seed) for make in (to.independent_set, to.thinned_set) for seed in to.SEEDS]
    masks += [np.ones(len(rings)), np.zeros(len(rings))]                     # (labelling does not ask whether tiles overlap)
    sweeps, _ = _host_labelling(components_program, tmp_path, rings, masks)
    print(f"\nunion_components {which}: sweeps per mask {sweeps} (cap {len(rings) + 1})")
    assert sweeps[-1] == 1 and max(sweeps) >= 2


def test_collision_row_test_on_the_host(components_program, tmp_path):
    """`collides` on the program's own four rows {1, 2^31 - 1}, {0, -1}, {2}, {2} with tile 1 dead: (row, first, stride, answer,
    error word).  An entry out of range sets the index bit and is passed over; the row's own tile and a dead tile do not count;
    with stride 2 a call sees every second entry only."""
    tri = np.array([[0, 0], [1, 0], [0, 1]], dtype=float)
    _, got = _host_labelling(components_program, tmp_path, [tri], [np.ones(1)])
    assert got == [(0, 0, 1, 0, 1), (0, 0, 2, 0, 0), (0, 1, 2, 0, 1),
                   (1, 0, 1, 1, 1), (1, 0, 2, 1, 0), (1, 1, 2, 0, 1),
                   (2, 0, 1, 0, 0), (2, 0, 2, 0, 0), (2, 1, 2, 0, 0),
                   (3, 0, 1, 1, 0), (3, 0, 2, 1, 0), (3, 1, 2, 0, 0)]


# ------------------------------------------------------------------------------------------------ no GPU, no answer
def test_detect_holes_refuses_without_a_gpu(graphs, monkeypatch):
    from tilingnn_amd.tiling.brick_layout import BrickLayout, detect_holes_many
    from tilingnn_amd.util import data_util as du
    g = graphs["small"]
    layout = BrickLayout(g, *du.create_brick_layout_from_super_set(g, [0, 1, 2, 3]))
    layout.predict[0] = 1
    assert layout.selected_tiles().tolist() == [0]
    monkeypatch.setattr(torch.cuda, "is_available", lambda: False)              # (on a GPU box too: the refusal is what is tested)
    for call in (layout.detect_holes, layout.count_holes, lambda: detect_holes_many([layout])):
        with pytest.raises(RuntimeError, match="no host fallback"):
            call()
