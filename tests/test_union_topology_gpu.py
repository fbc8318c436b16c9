"""Components and holes of a union of tiles on the GPU (csrc/union_topology.hip: tgnn_union_topology) against the loop-tracing
oracle of tests/topology_oracle.py -- another method than the kernel's sum of local Euler terms -- and `BrickLayout.detect_holes`
/ `count_holes` / `detect_holes_many` built on it.  Every comparison is exact integer equality.  The oracle itself, the contact
relation and the sweep-direction picker are checked on the host (tests/test_union_topology_host.py)."""
import gzip
import math
import os
import shutil

import numpy as np
import pytest
import torch

from tests import topology_oracle as to
from tests.golden_util import GOLDEN, load_npz

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
TOL = 1e-6


def _box(x0, y0, x1, y1):
    return np.array([[x0, y0], [x1, y0], [x1, y1], [x0, y1]], dtype=float)


def _abi(tiles, masks, pairs=None, touch=None, theta=None, ws_fill=None):
    """tgnn_union_topology straight from arrays.  pairs: collision pairs [2, E] (default none); touch: (touch_ptr, touch_idx)
    (default contact_geometry); theta: the sweep direction (default sweep_direction); ws_fill: a byte the workspace is filled with
    first.  Returns (out [K, 3], error word)."""
    from tilingnn_amd import _lib
    from tilingnn_amd._lib import check, lib, ptr
    from tilingnn_amd.tiling.region import contact_geometry, sweep_direction, union_geometry
    n = len(tiles)
    geo = union_geometry(tiles, np.zeros((2, 0), dtype=np.int64) if pairs is None else pairs, n)
    touch = contact_geometry(geo[0], geo[1]) if touch is None else touch
    theta = sweep_direction(geo[0], geo[1]) if theta is None else theta
    dev = [torch.from_numpy(a if a.size else np.zeros(1, dtype=a.dtype)).to(DEV) for a in tuple(geo) + tuple(touch)]
    masks = torch.from_numpy(np.ascontiguousarray(np.asarray(masks).reshape(-1, n), dtype=np.int32)).to(DEV)
    k = int(masks.shape[0])
    out = torch.full((k, 3), -7, dtype=torch.int32, device=DEV)
    err = torch.zeros(1, dtype=torch.int32, device=DEV)
    ws_bytes = int(lib.tgnn_union_topology_workspace_bytes(k, n))
    ws = torch.zeros(max(ws_bytes, 1), dtype=torch.uint8, device=DEV)
    if ws_fill is not None:
        ws.fill_(ws_fill)
    check(lib.tgnn_union_topology(ptr(dev[0]), ptr(dev[1]), n, *(ptr(a) for a in dev[2:]), ptr(masks), k, TOL, math.cos(theta),
                                  math.sin(theta), ptr(out), ptr(err), ptr(ws), ws_bytes, _lib.current_stream(torch.device(DEV))))
    torch.cuda.synchronize()
    return out.cpu().numpy(), int(err.item())


def _all_subsets(n):
    return ((np.arange(2 ** n)[:, None] >> np.arange(n)[None, :]) & 1).astype(np.int32)


# ------------------------------------------------------------------------------------------------ 1. hand-made sets, every subset
_SUBSET_ORACLE = {}


def _subset_oracle(name, tiles):
    """[2^n, 2] (components, holes) of every subset by the oracle, made once per set from the tiles AS GIVEN and shared by the
    rotations: a rotation changes no count (the oracle at the three rotations is itself checked on the host)."""
    if name not in _SUBSET_ORACLE:
        want = np.array([to.topology([tiles[i] for i in np.flatnonzero(m)]) for m in _all_subsets(len(tiles))], dtype=np.int32)
        want.setflags(write=False)
        _SUBSET_ORACLE[name] = want
    return _SUBSET_ORACLE[name]


@pytest.mark.parametrize("angle", to.ROTATIONS)
def test_hand_sets_every_subset(angle):
    sets = to.hand_sets()
    assert len(sets) == 12
    for name, (tiles, whole) in sets.items():
        n = len(tiles)
        assert n <= 10
        want = _subset_oracle(name, tiles)
        assert tuple(want[-1]) == whole, name                              # all tiles: the count worked out by hand
        got, err = _abi(to.rotated(tiles, angle), _all_subsets(n))
        assert err == 0, name
        assert got[0].tolist() == [0, 0, 0], name                          # the empty mask
        bad = np.flatnonzero((got[:, :2] != want).any(axis=1) | (got[:, 2] != 0))
        assert bad.size == 0, (name, angle, int(bad[0]), got[bad[0]].tolist(), want[bad[0]].tolist())


@pytest.mark.parametrize("angle", to.ROTATIONS)
def test_overlapping_tiles_are_reported_not_answered(angle):
    """The 3 x 3 ring of squares and two rectangles that overlap each other (one of them touching the ring): a subset with both
    gets status 1 and counts of -1, every other subset its counts."""
    tiles = to.hand_sets()["3x3 without the centre"][0] + [_box(3, 0, 5, 1), _box(4, 0, 6, 1)]
    assert len(tiles) == 10
    masks = _all_subsets(10)
    both = (masks[:, 8] & masks[:, 9]) != 0
    if "overlap" not in _SUBSET_ORACLE:
        want = np.array([(-1, -1) if b else to.topology([tiles[i] for i in np.flatnonzero(m)]) for m, b in zip(masks, both)],
                        dtype=np.int32)
        want.setflags(write=False)
        _SUBSET_ORACLE["overlap"] = want
    want = _SUBSET_ORACLE["overlap"]
    got, err = _abi(to.rotated(tiles, angle), masks, pairs=np.array([[8], [9]]))
    assert err == 0 and both.sum() == 256
    assert (got[:, 2] == both).all() and (got[both, :2] == -1).all()
    assert (got[:, :2] == want).all()
    assert {tuple(w) for w in want[~both]} >= {(1, 1), (2, 1), (1, 0), (3, 0)}     # the others are no trivial lot


# ------------------------------------------------------------------------------------------------ the lattice fixtures
class Fixture:
    def __init__(self, graph):
        from tilingnn_amd.util.data_util import graph_on_device
        self.graph = graph
        self.rings = [np.asarray(t.tile_poly.exterior)[:-1] for t in graph.tiles]
        self.n = len(self.rings)
        self.col = graph.arrays.colli_edges
        self.on_device = graph_on_device(graph, DEV)

    def gpu(self, masks):
        masks = np.ascontiguousarray(np.asarray(masks).reshape(-1, self.n), dtype=np.int32)
        return self.on_device.union_topology(torch.from_numpy(masks).to(DEV)).cpu().numpy()

    def oracle(self, mask):
        return to.topology([self.rings[i] for i in np.flatnonzero(mask)])


@pytest.fixture(scope="module")
def ring9(tmp_path_factory):
    from tilingnn_amd.tiling.tile_graph import TileGraph
    path = str(tmp_path_factory.mktemp("labyrinth") / "complete_graph_ring9.pkl")
    with gzip.open(os.path.join(GOLDEN, "complete_graph_ring9.pkl.gz"), "rb") as src, open(path, "wb") as dst:
        shutil.copyfileobj(src, dst)
    g = TileGraph(2)
    g.load_graph_state(path, sidecar=False)
    return Fixture(g)


@pytest.fixture(scope="module")
def small():
    from tilingnn_amd.tiling.tile_graph import TileGraph
    g = TileGraph(2)
    g.load_graph_state(os.path.join(GOLDEN, "complete_graph_small.pkl"), sidecar=False)
    return Fixture(g)


@pytest.mark.parametrize("which", ["ring9", "small"])
def test_single_tile_masks(which, request):
    fx = request.getfixturevalue(which)
    assert which != "ring9" or fx.n == 1254
    got = fx.gpu(np.eye(fx.n, dtype=np.int32))
    assert got.shape == (fx.n, 3) and got.dtype == np.int32 and (got == np.array([1, 0, 0])).all()


def _lattice_masks(fx):
    return [make(fx.n, fx.col, seed) for make in (to.independent_set, to.thinned_set) for seed in to.SEEDS]


def test_lattice_masks_match_the_oracle(ring9, small):
    """16 collision-free masks per fixture (8 maximal independent sets, 8 thinned ones) and the reference-made selections of
    tests/golden (ref_scores.npz on the small graph, ref_greedy.npz on ring 9): 40 masks, none skipped."""
    ref, greedy = load_npz("ref_scores.npz"), load_npz("ref_greedy.npz")
    cases = [(small, m) for m in _lattice_masks(small)] + [(ring9, m) for m in _lattice_masks(ring9)]
    for case in ["all", "first80", "random60", "shuffled40", "single", "no_adj"]:
        m = np.zeros(small.n, dtype=bool)
        m[ref[f"{case}.super_tiles"][np.asarray(ref[f"{case}.predict"]) > 0]] = True
        cases.append((small, m))
    cases += [(ring9, np.asarray(greedy[f"{k}.selection"]) == 1) for k in ("greedy0", "greedy7")]
    assert len(cases) == 40
    seen = []
    for fx in (small, ring9):
        masks = [m for f, m in cases if f is fx]
        assert all(m.any() and not (m[fx.col[0]] & m[fx.col[1]]).any() for m in masks)
        got = fx.gpu(masks)
        want = np.array([fx.oracle(m) for m in masks])
        print(f"\nunion_topology lattice masks ({fx.n} tiles): holes {got[:, 1].tolist()}, components {got[:, 0].tolist()}")
        assert (got[:, 2] == 0).all() and (got[:, :2] == want).all(), (got.tolist(), want.tolist())
        seen.append(got)
    seen = np.concatenate(seen)
    assert seen[:, 1].min() == 0 and seen[:, 1].max() > 30 and set(seen[:, 0].tolist()) >= {1, 2}


# ------------------------------------------------------------------------------------------------ bits, shapes, slices
def test_same_bits_on_a_second_call_and_on_a_dirty_workspace(ring9):
    masks = [to.thinned_set(ring9.n, ring9.col, seed) for seed in to.SEEDS] + [np.zeros(ring9.n, dtype=bool)]
    a, b = ring9.gpu(masks), ring9.gpu(masks)
    assert a.tobytes() == b.tobytes() and a[-1].tolist() == [0, 0, 0]
    for k in (0, 7):                                                        # a row does not depend on its neighbours in the batch
        assert ring9.gpu(masks[k]).tobytes() == a[k:k + 1].tobytes()
    clean, err0 = _abi(ring9.rings, masks, pairs=ring9.col, theta=0.1234)
    dirty, err1 = _abi(ring9.rings, masks, pairs=ring9.col, theta=0.1234, ws_fill=0x7F)
    again, err2 = _abi(ring9.rings, masks, pairs=ring9.col, theta=0.1234, ws_fill=0xFF)
    assert err0 == err1 == err2 == 0
    assert clean.tobytes() == dirty.tobytes() == again.tobytes() == a.tobytes()
    none = ring9.on_device.union_topology(torch.zeros(0, ring9.n, dtype=torch.int32, device=DEV))
    assert none.shape == (0, 3) and none.dtype == torch.int32
    assert ring9.on_device.union_topology(torch.from_numpy(masks[0]).to(DEV)).shape == (1, 3)     # a bool mask, one row
    with pytest.raises(ValueError):
        ring9.on_device.union_topology(torch.zeros(2, ring9.n + 1, dtype=torch.int32, device=DEV))


def test_more_masks_than_one_grid_holds(small):
    """K = 65 535 + 5: single tiles repeated, and masks with known counts on both sides of the slice boundary."""
    k = 65535 + 5
    alive = torch.zeros(k, small.n, dtype=torch.int32, device=DEV)
    rows = torch.arange(k, device=DEV)
    alive[rows, rows % small.n] = 1
    special = {65533: to.thinned_set(small.n, small.col, 3), 65534: to.thinned_set(small.n, small.col, 1),
               65535: to.thinned_set(small.n, small.col, 3), 65536: to.thinned_set(small.n, small.col, 1),
               65539: to.thinned_set(small.n, small.col, 5)}
    for row, m in special.items():
        alive[row] = torch.from_numpy(m.astype(np.int32)).to(DEV)
    got = small.on_device.union_topology(alive).cpu().numpy()
    plain = np.ones(k, dtype=bool)
    plain[list(special)] = False
    assert (got[plain] == np.array([1, 0, 0])).all()
    for row, m in special.items():
        assert got[row].tolist() == list(small.oracle(m)) + [0], row
    assert got[65535].tolist() == [1, 4, 0] and got[65536].tolist() == [2, 2, 0]     # (topology_oracle.QUOTED, seeds 3 and 1)


@pytest.mark.parametrize("extra", [0, 1])
def test_graphs_either_side_of_the_lds_limit(extra):
    """The component labels live in LDS for graphs of up to 6 144 tiles and in the workspace beyond: a 96 x 64 grid of unit
    squares (6 144 tiles, the last size of the first path) and the same grid with one more square far away (the first size of the
    second).  Counts by reasoning on the cells: a removed cell strictly inside is a hole of its own when its four neighbours
    stay, and the cells of a checkerboard hang together by their corners."""
    w, h = 96, 64
    x, y = [c.reshape(-1) for c in np.meshgrid(np.arange(w), np.arange(h))]
    tiles = [_box(a, b, a + 1, b + 1) for a, b in zip(x, y)] + [_box(200, 0, 201, 1)] * extra
    inside = (x >= 1) & (x <= w - 2) & (y >= 1) & (y <= h - 2)
    sieve = ~((x % 2 == 1) & (y % 2 == 1) & inside)
    dots = (x % 2 == 0) & (y % 2 == 0)
    checker = (x + y) % 2 == 0
    masks = np.stack([sieve, dots, checker, np.ones(w * h, dtype=bool)]).astype(np.int32)
    masks = np.concatenate([masks, np.ones((4, extra), dtype=np.int32)], axis=1)
    want = [[1 + extra, int((~sieve).sum()), 0], [int(dots.sum()) + extra, 0, 0],
            [1 + extra, int((~checker & inside).sum()), 0], [1 + extra, 0, 0]]
    assert want[0][1] == 47 * 31 and want[1][0] == 48 * 32 + extra and want[2][1] == 94 * 62 // 2
    got, err = _abi(tiles, masks, ws_fill=0x55)
    assert err == 0 and got.tolist() == want


def test_abi_rejects_bad_arguments():
    from tilingnn_amd._lib import lib
    args = lambda *a: lib.tgnn_union_topology(*a)
    assert args(None, None, 4, None, None, None, None, None, 2, TOL, 1.0, 0.0, None, None, None, 0, None) == -1
    assert b"tgnn_union_topology" in lib.tgnn_last_error()
    assert args(None, None, 4, None, None, None, None, None, 0, TOL, 1.0, 0.0, None, None, None, 0, None) == 0
    assert args(None, None, -1, None, None, None, None, None, 0, TOL, 1.0, 0.0, None, None, None, 0, None) == -1
    f64 = torch.zeros(64, dtype=torch.float64, device=DEV)
    i32 = torch.zeros(64, dtype=torch.int32, device=DEV)
    p = lambda t: t.data_ptr()
    full = lambda tol, dx, dy, ws_bytes: args(p(f64), p(i32), 4, p(i32), p(i32), p(i32), p(i32), p(i32), 2, tol, dx, dy, p(i32),
                                              p(i32), p(i32), ws_bytes, None)
    assert full(TOL, 1.0, 0.0, 8) == -1                                     # a workspace that is too small
    assert full(-1.0, 1.0, 0.0, 256) == -1 and full(TOL, 0.5, 0.5, 256) == -1 and full(TOL, float("nan"), 0.0, 256) == -1
    assert lib.tgnn_union_topology_workspace_bytes(2, 4) == 2 * (4 + 2) * 4 and lib.tgnn_union_topology_workspace_bytes(0, 4) == 0


# ------------------------------------------------------------------------------------------------ error bits
def _fan(count):
    """Thin triangles fanned around the origin, which is a vertex of every one."""
    return [np.array([[0, 0], [math.cos(t), math.sin(t)], [math.cos(t + 0.2), math.sin(t + 0.2)]]) for t in 0.3 + 0.36 * np.arange(count)]


def test_error_bits_index_and_wedge_overflow():
    from tilingnn_amd._lib import TgnnError
    from tilingnn_amd.tiling.region import contact_geometry, union_geometry
    from tilingnn_amd.util.data_util import CompleteGraphOnDevice
    tiles = to.hand_sets()["pinwheel"][0]
    geo = union_geometry(tiles, np.zeros((2, 0), dtype=np.int64), 4)
    touch_ptr, touch_idx = contact_geometry(geo[0], geo[1])
    got, err = _abi(tiles, [np.ones(4)], touch=(touch_ptr, touch_idx))
    assert err == 0 and got[0].tolist() == [1, 1, 0]
    for wrong in (4, -1, 2 ** 31 - 1):
        broken = touch_idx.copy()
        broken[1] = wrong
        _, err = _abi(tiles, [np.ones(4)], touch=(touch_ptr, broken))
        assert err == 1, wrong
    # 16 tiles around one point fit the wedge list, 17 do not
    fan = _fan(17)
    got, err = _abi(fan, [np.array([1] * 16 + [0]), np.array([0] + [1] * 16)], theta=0.1234)
    assert err == 0 and got.tolist() == [[1, 0, 0], [1, 0, 0]]
    got, err = _abi(fan, [np.array([1] * 16 + [0]), np.ones(17)], theta=0.1234)
    assert err == 2
    # ... which the binding raises on
    geo = union_geometry(fan, np.zeros((2, 0), dtype=np.int64), 17)
    od = CompleteGraphOnDevice.__new__(CompleteGraphOnDevice)
    od.device, od.n_tiles = torch.device(DEV), 17
    up = lambda a: torch.from_numpy(a if a.size else np.zeros(1, dtype=a.dtype)).to(DEV)
    od._union = tuple(up(a) for a in geo)
    od._topology = tuple(up(a) for a in contact_geometry(geo[0], geo[1])) + (math.cos(0.1234), math.sin(0.1234))
    assert od.union_topology(torch.tensor([1] * 16 + [0], device=DEV)).cpu().tolist() == [[1, 0, 0]]
    with pytest.raises(TgnnError, match="wedge"):
        od.union_topology(torch.ones(17, dtype=torch.int32, device=DEV))


# ------------------------------------------------------------------------------------------------ the longest way for a label
CHAIN = 193                                                                 # one more than three waves of 64 lanes
# tile index by position along the chain, the lowest index at position 0.  "descending": the indices fall by one per step
# towards it, the slowest a permutation can (every tile's first label points one step on, and the walk to the root is as long
# as the chain).  "against": past position 0 they RISE towards it, so every tile first joins the far end's tile 1 and the
# label 0 comes one position per round, the most rounds a chain can take.
CHAIN_ORDERS = {"descending": np.arange(CHAIN), "against": np.concatenate([[0], np.arange(CHAIN - 1, 0, -1)])}


@pytest.mark.parametrize("order", sorted(CHAIN_ORDERS))
def test_chain_of_squares_through_the_three_calls(order):
    """193 unit squares end to end, all alive / the middle one dead / every second one dead, through union_topology,
    union_contours and hole_deltas: the three kernels that label components must agree on a label that has the whole chain to
    travel, and give the same bytes on a second call."""
    from tilingnn_amd.tiling.region import contact_geometry, union_geometry
    from tilingnn_amd.util.data_util import CompleteGraphOnDevice
    index = CHAIN_ORDERS[order]
    assert sorted(index.tolist()) == list(range(CHAIN)) and index[0] == 0
    place = np.argsort(index)                                               # position of tile t
    tiles = [_box(p, 0, p + 1, 1) for p in place.tolist()]
    geo = union_geometry(tiles, np.zeros((2, 0), dtype=np.int64), CHAIN)
    od = CompleteGraphOnDevice.__new__(CompleteGraphOnDevice)
    od.device, od.n_tiles = torch.device(DEV), CHAIN
    up = lambda a: torch.from_numpy(a if a.size else np.zeros(1, dtype=a.dtype)).to(DEV)
    od._union = tuple(up(a) for a in geo)
    od._topology = tuple(up(a) for a in contact_geometry(geo[0], geo[1])) + (math.cos(0.1234), math.sin(0.1234))
    here = np.arange(CHAIN)
    by_place = np.stack([np.ones(CHAIN, dtype=bool), here != CHAIN // 2, here % 2 == 0])
    masks = np.zeros((3, CHAIN), dtype=np.int32)
    masks[:, index] = by_place
    assert masks.sum(axis=1).tolist() == [193, 192, 97]
    alive = torch.from_numpy(masks).to(DEV)

    def run():
        topo = od.union_topology(alive)
        rings = od.union_contours(alive)
        delta, state = od.hole_deltas(alive)
        return [t.cpu().numpy() for t in (topo, rings.mask, rings.ring, rings.ring_area, rings.pts_xy, rings.pts_src, delta, state)]
    first, again = run(), run()
    topo, ring_mask, delta, state = first[0], first[1], first[6], first[7]
    assert topo.tolist() == [[1, 0, 0], [2, 0, 0], [97, 0, 0]]
    assert ring_mask[:, 0].tolist() == [1, 2, 97] and (ring_mask[:, 3] == 0).all()
    middle = int(index[CHAIN // 2])
    assert masks[1, middle] == 0 and delta[1, middle].tolist() == [-1, 0] and state[1, middle] == 0
    assert all(a.tobytes() == b.tobytes() for a, b in zip(first, again))


# ------------------------------------------------------------------------------------------------ BrickLayout
def _solved_layout(fx, selection, seed):
    """A layout cut from the complete graph around `selection` (the selected tiles and a random half of the others), with
    `predict` = the selection."""
    from tilingnn_amd.tiling.brick_layout import BrickLayout
    from tilingnn_amd.util import data_util as du
    keep = selection | (np.random.default_rng(seed).random(fx.n) < 0.5)
    tiles = np.flatnonzero(keep)
    layout = BrickLayout(fx.graph, *du.create_brick_layout_from_super_set(fx.graph, tiles.tolist()))
    assert len(layout.node_feature) == tiles.size < fx.n
    layout.predict = np.array([1.0 if selection[layout.inverse_index[i]] else 0.0 for i in range(tiles.size)])
    return layout


def test_brick_layout_detect_holes_and_count_holes(ring9):
    closed, holed = to.independent_set(ring9.n, ring9.col, 0), to.thinned_set(ring9.n, ring9.col, 7)
    want = ring9.gpu([closed, holed])
    assert want[0].tolist() == [1, 0, 0] and want[1].tolist() == [2, 44, 0]
    a, b = _solved_layout(ring9, closed, 1), _solved_layout(ring9, holed, 2)
    assert np.array_equal(np.sort(b.selected_tiles()), np.flatnonzero(holed))
    assert a.count_holes(DEV) == (1, 0) and a.detect_holes(DEV) is False
    assert b.count_holes() == (2, 44) and b.detect_holes() is True
    unsolved = _solved_layout(ring9, closed, 3)
    unsolved.predict[:] = 0
    assert unsolved.count_holes() == (0, 0) and unsolved.detect_holes() is False
    # two selected tiles that collide: no answer
    i, j = ring9.col[:, 0]
    clash = np.zeros(ring9.n, dtype=bool)
    clash[[i, j]] = True
    with pytest.raises(ValueError, match="collide"):
        _solved_layout(ring9, clash, 4).detect_holes()
    with pytest.raises(ValueError, match="collide"):
        _solved_layout(ring9, clash, 4).count_holes()


def test_detect_holes_many_equals_the_single_calls(ring9, small):
    from tilingnn_amd.tiling.brick_layout import detect_holes_many
    layouts = [_solved_layout(ring9, to.thinned_set(ring9.n, ring9.col, s), s) for s in (0, 5, 7)]
    layouts.append(_solved_layout(ring9, to.independent_set(ring9.n, ring9.col, 2), 9))
    many = detect_holes_many(layouts, DEV)
    assert many == [l.count_holes(DEV) for l in layouts] == [(1, 40), (1, 44), (2, 44), (1, 1)]
    assert [h > 0 for _, h in many] == [l.detect_holes() for l in layouts]
    assert detect_holes_many([]) == []
    with pytest.raises(ValueError, match="one complete graph"):
        detect_holes_many([layouts[0], _solved_layout(small, to.independent_set(small.n, small.col, 0), 0)])
    clash = np.zeros(ring9.n, dtype=bool)
    clash[ring9.col[:, 0]] = True
    with pytest.raises(ValueError, match="layout 1"):
        detect_holes_many([layouts[0], _solved_layout(ring9, clash, 4)])
