"""Host side of the union contour (csrc/union_contour.hip): the ring-returning loop walk of tests/contour_oracle.py against rings
written out by hand and on the lattice fixtures, the kernels' per-piece code (csrc/union_contour_piece.h) run on the host under
sanitizers as a stand-alone program, and the refusal to run without a GPU.  The GPU tests (tests/test_union_contour_gpu.py) lean
on every one of these."""
import gzip
import os
import shutil
import struct
import subprocess

import numpy as np
import pytest
import torch

from tests import contour_oracle as co
from tests import topology_oracle as to
from tests.golden_util import GOLDEN

# points per ring of the twelve hand sets as given, measured where the kernel was designed
QUOTED_POINTS = ([4], [4, 4], [6, 4], [8], [4, 4], [4, 4], [8], [4, 4, 4], [4, 6], [4, 3, 3], [8, 4], [24, 4, 4])


def _max_splits():
    from tilingnn_amd.tiling.region import CONTOUR_MAX_SPLITS
    return CONTOUR_MAX_SPLITS


def _tile_area(tiles):
    return sum(abs(to._signed_area(to._open(t))) for t in tiles)


def _check_properties(tiles, want_topology, label):
    """What holds for every set: exteriors / holes = the (components, holes) given, the signed areas sum to the tiles' areas, the
    rings list at most 2 x the tiles' vertices.  Returns points / vertices."""
    got = co.contours(tiles)
    ext, holes = sum(r.area > 0 for r in got), sum(r.area < 0 for r in got)
    assert (ext, holes) == tuple(want_topology), label
    area = _tile_area(tiles)
    assert abs(sum(r.area for r in got) - area) <= 1e-9 * max(area, 1.0), label
    points, verts = sum(r.xy.shape[0] for r in got), sum(to._open(t).shape[0] for t in tiles)
    assert points <= 2 * verts, label
    assert [r.leader for r in got] == sorted(r.leader for r in got), label
    return got, points / verts


# ------------------------------------------------------------------------------------------------ the oracle
def test_constant_and_new_sets():
    assert _max_splits() >= 8
    extra = co.extra_sets(_max_splits())
    assert list(extra) == ["tip on a bar", "comb", "comb past the limit"]
    assert len(extra["comb"][0]) == 9 and len(extra["comb past the limit"][0]) == _max_splits() + 3
    assert all(len(t) <= 10 for name, (t, _) in extra.items() if name != "comb past the limit")


@pytest.mark.parametrize("angle", to.ROTATIONS)
def test_oracle_gives_the_hand_rings(angle):
    sets, want = co.all_sets(_max_splits()), co.hand_rings(_max_splits())
    assert len(sets) == 15 and set(sets) == set(want)
    ratios = {}
    for name, (tiles, topo) in sets.items():
        turned = to.rotated(tiles, angle)
        got, ratios[name] = _check_properties(turned, topo, (name, angle))
        assert to.topology(turned) == topo, name
        assert len(got) == len(want[name]), (name, [r.xy.tolist() for r in got])
        for q, (ring, hand) in enumerate(zip(got, want[name])):                 # the same order: ascending leaders
            hand = to.rotated([np.asarray(hand, dtype=float)], angle)[0]
            assert co.same_ring(ring.xy, hand), (name, angle, q, ring.xy.tolist(), hand.tolist())
            assert (ring.area > 0) == (to._signed_area(hand) > 0)
    assert [[len(r) for r in want[name]] for name in to.hand_sets()] == list(QUOTED_POINTS)
    assert max(ratios[name] for name in to.hand_sets()) == 1.0                    # the twelve reach exactly 1 ...
    assert ratios["tip on a bar"] == 8 / 7 and max(ratios.values()) == 8 / 7      # ... tip on a bar is the set that exceeds it


def test_ring_starts_at_the_first_corner_after_the_leader():
    tiles = co.extra_sets(_max_splits())["comb"][0]
    (ring,) = co.contours(tiles)
    assert ring.leader == (0, 0, 0) and ring.pieces == 3 + 8 + 2 and ring.xy.tolist() == [[0, 0], [8, 0], [8, 2], [0, 2]]
    (ring,) = co.contours(tiles[1:3])                                              # two squares side by side: leader (0, 0, 0)
    assert ring.xy.tolist() == [[0, 1], [2, 1], [2, 2], [0, 2]] and ring.pieces == 6
    assert co.contours([]) == []
    with pytest.raises(ValueError):
        co.contours([to._box(0, 0, 2, 1), to._box(0, 0, 1, 1)])


# ------------------------------------------------------------------------------------------------ the lattice fixtures
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


@pytest.mark.parametrize("which", ["small", "ring9"])
def test_oracle_on_the_lattice_recipes(which, graphs):
    g = graphs[which]
    rings, col = _rings(g), g.arrays.colli_edges
    assert any(r.shape[0] == 3 for r in rings)                                    # both graphs have triangular tiles
    seen = []
    for kind, make in (("independent", to.independent_set), ("thinned", to.thinned_set)):
        for seed in range(4):
            tiles = [rings[i] for i in np.flatnonzero(make(len(rings), col, seed))]
            want = (to.QUOTED[(which, kind)][1][seed], to.QUOTED[(which, kind)][0][seed])
            got, _ = _check_properties(tiles, want, (which, kind, seed))
            seen.append((kind, sum(r.area > 0 for r in got), sum(r.area < 0 for r in got), max(r.xy.shape[0] for r in got)))
    print(f"\nunion_contour oracle {which}: (kind, exteriors, holes, longest ring) {seen}")
    if which == "ring9":
        thinned = [s for s in seen if s[0] == "thinned"]
        assert all(e == 1 and 37 <= h <= 40 and 76 <= longest <= 87 for _, e, h, longest in thinned)


# ------------------------------------------------------------------------------------------------ the kernels' per-piece code
@pytest.fixture(scope="module")
def piece_program(tmp_path_factory):
    """tests/host/union_contour_piece_test.cpp: the header the kernels run per tile and per piece, built with the host compiler
    alone under AddressSanitizer + UBSan (the sanitizers' runtime linked into the program itself), run directly."""
    repo = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    cxx = os.environ.get("CXX") or shutil.which("g++") or shutil.which("c++") or shutil.which("clang++")
    assert cxx, "no host C++ compiler"
    clang = "clang" in subprocess.run([cxx, "--version"], capture_output=True, text=True).stdout
    static_rt = ["-static-libsan"] if clang else ["-static-libasan", "-static-libubsan"]
    exe = str(tmp_path_factory.mktemp("contour_piece") / "union_contour_piece_test")
    build = subprocess.run([cxx, "-std=c++17", "-O1", "-g", "-Wall", "-Wextra", "-Werror", "-fsanitize=address,undefined",
                            "-fno-sanitize-recover=undefined", *static_rt, "-I", os.path.join(repo, "tilingnn_amd", "csrc"),
                            os.path.join(repo, "tests", "host", "union_contour_piece_test.cpp"), "-o", exe],
                           capture_output=True, text=True)
    assert build.returncode == 0, build.stderr[-4000:]
    return exe


def _host_contours(exe, tmp_path, tiles, masks):
    """Per mask (pieces, most splits on one side, [ring as pts_src list]), and the error word, from the host program; also the
    ring_xy the indices point into."""
    from tilingnn_amd.tiling.region import UNION_TOL, contact_geometry, union_geometry
    n = len(tiles)
    ring_xy, ring_ptr, _, _ = union_geometry(tiles, np.zeros((2, 0), dtype=np.int64), n)
    touch_ptr, touch_idx = contact_geometry(ring_xy, ring_ptr)
    masks = np.ascontiguousarray(np.asarray(masks).reshape(-1, n), dtype=np.int32)
    path = str(tmp_path / "case.bin")
    with open(path, "wb") as f:
        f.write(struct.pack("<4q1d", n, ring_xy.shape[0], touch_idx.shape[0], masks.shape[0], UNION_TOL))
        for a in (ring_xy, ring_ptr, touch_ptr, touch_idx, masks):
            f.write(np.ascontiguousarray(a).tobytes())
    run = subprocess.run([exe, path], capture_output=True, text=True)
    assert run.returncode == 0, (run.stdout + run.stderr)[-4000:]
    out, err = [], None
    for line in run.stdout.splitlines():
        words = line.split()
        if words[0] == "mask":
            out.append((int(words[1]), int(words[2]), []))
        elif words[0] == "ring":
            out[-1][2].append([int(w) for w in words[1:]])
        else:
            assert words[0] == "err"
            err = int(words[1])
    assert len(out) == masks.shape[0] and err is not None
    return out, err, ring_xy, ring_ptr


def _assert_rings_match(got_src, ring_xy, want, label):
    assert len(got_src) == len(want), (label, len(got_src), len(want))
    for q, (src, ring) in enumerate(zip(got_src, want)):
        assert co.same_ring(ring_xy[src], ring.xy), (label, q, ring_xy[src].tolist(), ring.xy.tolist())


def test_piece_code_on_the_host_hand_sets(piece_program, tmp_path):
    limit = _max_splits()
    most = {"tip on a bar": 1, "comb": 7}
    for name, (tiles, _) in co.all_sets(limit).items():
        for angle in to.ROTATIONS:
            turned = to.rotated(tiles, angle)
            (mask,), err, ring_xy, _ = _host_contours(piece_program, tmp_path, turned, [np.ones(len(tiles))])
            if name == "comb past the limit":
                assert err & 4 and not err & ~(4 | 16), (name, angle)              # SPLITS (and the open ring it leaves): reported
                continue
            want = co.contours(turned)
            assert err == 0 and mask[0] == sum(r.pieces for r in want), (name, angle, err, mask[0])
            assert mask[1] <= 1 or name == "comb", name
            assert mask[1] == most.get(name, mask[1])
            _assert_rings_match(mask[2], ring_xy, want, (name, angle))


def test_piece_code_on_the_host_every_subset_of_three_sets(piece_program, tmp_path):
    """Every subset, the empty one too, of the checkerboard (pinches everywhere), the block ring with the hexagon (splits and
    twins on slanted sides) and tip on a bar."""
    for name in ("checkerboard", "block ring, hexagon bridging the hole", "tip on a bar"):
        tiles = co.all_sets(_max_splits())[name][0]
        n = len(tiles)
        masks = ((np.arange(2 ** n)[:, None] >> np.arange(n)[None, :]) & 1).astype(np.int32)
        got, err, ring_xy, ring_ptr = _host_contours(piece_program, tmp_path, tiles, masks)
        assert err == 0 and got[0] == (0, 0, [])
        tile_of = np.repeat(np.arange(n), np.diff(ring_ptr))
        for m, (_, _, rings) in zip(masks, got):
            _assert_rings_match(rings, ring_xy, co.contours([tiles[i] for i in np.flatnonzero(m)]), (name, m.tolist()))
            assert all(m[tile_of[src]].all() for src in rings)                    # every point is a vertex of an alive tile


@pytest.mark.parametrize("which", ["small", "ring9"])
def test_piece_code_on_the_host_lattice(which, graphs, piece_program, tmp_path):
    g = graphs[which]
    rings, col = _rings(g), g.arrays.colli_edges
    masks = [make(len(rings), col, seed) for make in (to.independent_set, to.thinned_set) for seed in range(2)]
    got, err, ring_xy, _ = _host_contours(piece_program, tmp_path, rings, masks)
    assert err == 0
    for m, (_, most, found) in zip(masks, got):
        assert most == 0                                                          # no foreign vertex inside a side on the lattices
        _assert_rings_match(found, ring_xy, co.contours([rings[i] for i in np.flatnonzero(m)]), which)


# ------------------------------------------------------------------------------------------------ no GPU, no answer
def test_union_polygon_refuses_without_a_gpu(graphs, monkeypatch):
    from tilingnn_amd.tiling.brick_layout import BrickLayout, union_polygons_many
    from tilingnn_amd.util import data_util as du
    g = graphs["small"]
    layout = BrickLayout(g, *du.create_brick_layout_from_super_set(g, [0, 1, 2, 3]))
    layout.predict[0] = 1
    monkeypatch.setattr(torch.cuda, "is_available", lambda: False)              # (on a GPU box too: the refusal is what is tested)
    for call in (layout.get_selected_tiles_union_polygon, lambda: union_polygons_many([layout])):
        with pytest.raises(RuntimeError, match="no host fallback"):
            call()
