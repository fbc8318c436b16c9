"""The outline of a union of tiles on the GPU (csrc/union_contour.hip: tgnn_union_contour) against the ring-returning loop walk
of tests/contour_oracle.py -- points identified on a snap grid where the kernel names them by canonical vertices -- and against
two kernels with unrelated methods: the ring counts must equal what tgnn_union_topology reports, the ring areas must sum to what
tgnn_union_area reports.  Then `UnionContours.polygons`, `BrickLayout.get_selected_tiles_union_polygon` and
`union_polygons_many` built on it.  The oracle, the hand-written rings and the per-piece code are checked on the host
(tests/test_union_contour_host.py).

The contract fixes the order of a mask's rings (ascending leader) and where each ring starts (the first corner at or after its
leader's start), and the oracle follows both: a mask is compared as ONE list of points, which is the match under a cyclic
rotation the rings must pass anyway, with the rotation and the order pinned."""
import gzip
import math
import os
import shutil

import numpy as np
import pytest
import torch

from tests import contour_oracle as co
from tests import topology_oracle as to
from tests import union_oracle as uo
from tests.golden_util import GOLDEN, load_npz

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
TOL = 1e-6
CANARY = -1234567


class Result:
    pass


def _abi(tiles, masks, pairs=None, touch=None, ws_fill=None, cap=None, max_pieces=None, geo=None):
    """tgnn_union_contour straight from arrays.  pairs: collision pairs [2, E] (default none); touch: (touch_ptr, touch_idx)
    (default contact_geometry); ws_fill: a byte the workspace is filled with first; cap: (cap_rings, cap_points) (default: the
    bound, 2 x the vertices of the alive tiles); 16 canary entries follow every output."""
    from tilingnn_amd import _lib
    from tilingnn_amd._lib import check, lib, ptr
    from tilingnn_amd.tiling.region import contact_geometry, union_geometry
    n = len(tiles)
    geo = union_geometry(tiles, np.zeros((2, 0), dtype=np.int64) if pairs is None else pairs, n) if geo is None else geo
    touch = contact_geometry(geo[0], geo[1]) if touch is None else touch
    dev = [torch.from_numpy(a if a.size else np.zeros(1, dtype=a.dtype)).to(DEV) for a in tuple(geo) + tuple(touch)]
    masks = np.ascontiguousarray(np.asarray(masks).reshape(-1, n), dtype=np.int32)
    k = int(masks.shape[0])
    bound = 2 * int(((masks != 0).astype(np.int64) @ np.diff(geo[1]).astype(np.int64)).sum()) if k else 0
    cap_rings, cap_points = (bound // 3 + 1, bound) if cap is None else cap
    max_pieces = bound if max_pieces is None else max_pieces
    r = Result()
    r.ring_xy, r.ring_ptr, r.cap = geo[0], geo[1], (cap_rings, cap_points)
    full = lambda shape, dt: torch.full(shape, CANARY, dtype=dt, device=DEV)
    mask_out = full((k + 16, 4), torch.int32)
    ring_out, ring_area = full((cap_rings + 16, 4), torch.int32), full((cap_rings + 16,), torch.float64)
    pts_xy, pts_src = full((cap_points + 16, 2), torch.float64), full((cap_points + 16,), torch.int32)
    total = full((2 + 16,), torch.int64)
    err = torch.zeros(1, dtype=torch.int32, device=DEV)
    ws_bytes = int(lib.tgnn_union_contour_workspace_bytes(k, n, max_pieces))
    ws = torch.zeros(ws_bytes // 8 + 1, dtype=torch.int64, device=DEV)
    if ws_fill is not None:
        ws.view(torch.uint8).fill_(ws_fill)
    check(lib.tgnn_union_contour(ptr(dev[0]), ptr(dev[1]), n, *(ptr(a) for a in dev[2:]), ptr(torch.from_numpy(masks).to(DEV)), k,
                                 TOL, cap_rings, cap_points, ptr(mask_out), ptr(ring_out), ptr(ring_area), ptr(pts_xy),
                                 ptr(pts_src), ptr(total), ptr(err), ptr(ws), ws_bytes, _lib.current_stream(torch.device(DEV))))
    torch.cuda.synchronize()
    r.all = [t.cpu().numpy() for t in (mask_out, ring_out, ring_area, pts_xy, pts_src)]
    r.mask, r.ring, r.area, r.xy, r.src = r.all
    r.total, r.err = total.cpu().numpy(), int(err.item())
    for a, used in ((r.mask, k), (r.ring, cap_rings), (r.area, cap_rings), (r.xy, cap_points), (r.src, cap_points), (r.total, 2)):
        assert (a[used:] == CANARY).all(), "a canary behind an output was overwritten"
    r.mask, r.total = r.mask[:k], r.total[:2]
    return r


def _bytes(r):
    rings, points = int(r.total[0]), int(r.total[1])
    return b"".join(a[:c].tobytes() for a, c in zip(r.all, (len(r.mask), rings, rings, points, points)))


def _all_subsets(n):
    return ((np.arange(2 ** n)[:, None] >> np.arange(n)[None, :]) & 1).astype(np.int32)


class Want:
    """The oracle's answer for one mask: the points of all rings as one list, points per ring, sign per ring, area per ring."""

    def __init__(self, tiles):
        rings = co.contours(tiles)
        self.xy = np.concatenate([r.xy for r in rings]) if rings else np.zeros((0, 2))
        self.counts = [r.xy.shape[0] for r in rings]
        self.signs = [1 if r.area > 0 else -1 for r in rings]
        self.areas = [r.area for r in rings]
        # two lists of points within SNAP of each other enclose areas that differ by at most SNAP x the perimeter
        self.area_tol = [to.SNAP * uo.perimeter(r.xy) + 1e-12 for r in rings]


def _check_mask(r, k, want, alive, label, angle=0.0):
    """Mask k of the result against the oracle: the same number of rings, the same points per ring, every point within SNAP of
    the oracle's in the same order (ascending leaders, each ring from its first corner), the signs; pts_xy = ring_xy[pts_src] bit
    for bit and every source tile alive; rings laid out back to back."""
    rings, first, points, status = (int(v) for v in r.mask[k])
    assert status == 0 and rings == len(want.counts), (label, rings, len(want.counts))
    rows = r.ring[first:first + rings]
    assert rows[:, 1].tolist() == want.counts and rows[:, 3].tolist() == want.signs, (label, rows.tolist(), want.counts)
    assert points == sum(want.counts)
    if rings == 0:
        return
    p0 = int(rows[0, 0])
    assert rows[:, 0].tolist() == (p0 + np.concatenate([[0], np.cumsum(want.counts)[:-1]])).tolist(), label
    xy, src = r.xy[p0:p0 + points], r.src[p0:p0 + points]
    turned = to.rotated([want.xy], angle)[0]
    assert np.hypot(*(xy - turned).T).max() <= to.SNAP, (label, xy.tolist(), turned.tolist())
    assert xy.tobytes() == r.ring_xy[src].tobytes(), label
    tile_of = np.searchsorted(r.ring_ptr, src, side="right") - 1
    assert (np.asarray(alive)[tile_of] != 0).all(), label
    assert (np.sign(r.area[first:first + rings]) == want.signs).all(), label
    assert (np.abs(r.area[first:first + rings] - want.areas) <= want.area_tol).all(), label
    assert set(rows[:, 2].tolist()) <= set(np.flatnonzero(alive).tolist()), label


def _max_splits():
    from tilingnn_amd.tiling.region import CONTOUR_MAX_SPLITS
    return CONTOUR_MAX_SPLITS


# ------------------------------------------------------------------------------------------------ 1. hand-made sets, every subset
_SUBSET_ORACLE = {}


def _subset_oracle(name, tiles):
    """The oracle for every subset, made once per set from the tiles AS GIVEN and shared by the rotations (the oracle at the
    three rotations is itself checked on the host)."""
    if name not in _SUBSET_ORACLE:
        _SUBSET_ORACLE[name] = [Want([tiles[i] for i in np.flatnonzero(m)]) for m in _all_subsets(len(tiles))]
    return _SUBSET_ORACLE[name]


@pytest.mark.parametrize("angle", to.ROTATIONS)
def test_hand_sets_every_subset(angle):
    sets = {name: tiles for name, (tiles, _) in co.all_sets(_max_splits()).items() if name != "comb past the limit"}
    assert len(sets) == 14
    for name, tiles in sets.items():
        n = len(tiles)
        assert n <= 10
        want, masks = _subset_oracle(name, tiles), _all_subsets(n)
        r = _abi(to.rotated(tiles, angle), masks)
        assert r.err == 0, (name, r.err)
        assert r.mask[0, [0, 2, 3]].tolist() == [0, 0, 0], name                 # the empty mask
        assert r.total.tolist() == [sum(len(w.counts) for w in want), sum(sum(w.counts) for w in want)], name
        assert r.mask[:, 1].tolist() == np.concatenate([[0], np.cumsum(r.mask[:-1, 0])]).tolist()
        for k, (m, w) in enumerate(zip(masks, want)):
            _check_mask(r, k, w, m, (name, angle, k), angle)


@pytest.mark.parametrize("angle", to.ROTATIONS)
def test_overlapping_tiles_are_reported_not_answered(angle):
    """The 3 x 3 ring of squares and two rectangles that overlap each other (one of them touching the ring): a subset with both
    gets status 1 and no rings, every other subset its rings."""
    tiles = to.hand_sets()["3x3 without the centre"][0] + [to._box(3, 0, 5, 1), to._box(4, 0, 6, 1)]
    assert len(tiles) == 10
    masks = _all_subsets(10)
    both = (masks[:, 8] & masks[:, 9]) != 0
    if "overlap" not in _SUBSET_ORACLE:
        _SUBSET_ORACLE["overlap"] = [None if b else Want([tiles[i] for i in np.flatnonzero(m)]) for m, b in zip(masks, both)]
    want = _SUBSET_ORACLE["overlap"]
    r = _abi(to.rotated(tiles, angle), masks, pairs=np.array([[8], [9]]))
    assert r.err == 0 and both.sum() == 256
    assert (r.mask[:, 3] == both).all() and (r.mask[both][:, [0, 2]] == 0).all()
    for k in np.flatnonzero(~both):
        _check_mask(r, k, want[k], masks[k], ("overlap", angle, k), angle)


# ------------------------------------------------------------------------------------------------ the lattice fixtures
class Fixture:
    def __init__(self, graph):
        from tilingnn_amd.util.data_util import graph_on_device
        self.graph = graph
        self.rings = [np.asarray(t.tile_poly.exterior)[:-1] for t in graph.tiles]
        self.n = len(self.rings)
        self.col = graph.arrays.colli_edges
        self.on_device = graph_on_device(graph, DEV)
        a = graph.arrays
        self.delta = uo.noise_width(self.rings, np.concatenate([a.colli_edges, a.adj_edges], axis=1), TOL)
        self._want = {}

    def dev(self, masks):
        masks = np.ascontiguousarray(np.asarray(masks).reshape(-1, self.n), dtype=np.int32)
        return torch.from_numpy(masks).to(DEV)

    def gpu(self, masks):
        """A Result-like view of on_device.union_contours."""
        c = self.on_device.union_contours(self.dev(masks))
        r = Result()
        r.all = list(c.host())
        r.mask, r.ring, r.area, r.xy, r.src = r.all
        r.total = np.array([r.ring.shape[0], r.xy.shape[0]])
        r.ring_xy, r.ring_ptr = c.ring_xy.cpu().numpy(), c.ring_ptr.cpu().numpy()
        r.contours = c
        return r

    def want(self, mask):
        key = np.asarray(mask, dtype=bool).tobytes()
        if key not in self._want:
            self._want[key] = Want([self.rings[i] for i in np.flatnonzero(mask)])
        return self._want[key]


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


def _lattice_masks(fx):
    return [make(fx.n, fx.col, seed) for make in (to.independent_set, to.thinned_set) for seed in to.SEEDS]


def test_lattice_masks_match_the_oracle_and_the_two_sibling_kernels(ring9, small):
    """The 40 masks of test_union_topology_gpu.py::test_lattice_masks_match_the_oracle.  From the same masks: exteriors and holes
    = union_topology's components and holes, one exterior per component label and every hole's label has one, and the ring areas
    sum to union_areas within union_oracle.gate (delta: the fixture's measured noise, as the union area's tests take it)."""
    ref, greedy = load_npz("ref_scores.npz"), load_npz("ref_greedy.npz")
    cases = [(small, m) for m in _lattice_masks(small)] + [(ring9, m) for m in _lattice_masks(ring9)]
    for case in ["all", "first80", "random60", "shuffled40", "single", "no_adj"]:
        m = np.zeros(small.n, dtype=bool)
        m[ref[f"{case}.super_tiles"][np.asarray(ref[f"{case}.predict"]) > 0]] = True
        cases.append((small, m))
    cases += [(ring9, np.asarray(greedy[f"{k}.selection"]) == 1) for k in ("greedy0", "greedy7")]
    assert len(cases) == 40
    longest = 0
    for fx in (small, ring9):
        masks = [m for f, m in cases if f is fx]
        assert all(m.any() and not (m[fx.col[0]] & m[fx.col[1]]).any() for m in masks)
        r = fx.gpu(masks)
        topo = fx.on_device.union_topology(fx.dev(masks)).cpu().numpy()
        areas = fx.on_device.union_areas(fx.dev(masks)).cpu().numpy()
        worst = 0.0
        for k, m in enumerate(masks):
            _check_mask(r, k, fx.want(m), m, (fx.n, k))
            rings, first = int(r.mask[k, 0]), int(r.mask[k, 1])
            rows, area = r.ring[first:first + rings], r.area[first:first + rings]
            assert topo[k].tolist() == [int((rows[:, 3] > 0).sum()), int((rows[:, 3] < 0).sum()), 0], (fx.n, k)
            ext = rows[rows[:, 3] > 0][:, 2]
            assert np.unique(ext).size == ext.size and set(rows[:, 2].tolist()) == set(ext.tolist()), (fx.n, k)
            gate = uo.gate([fx.rings[i] for i in np.flatnonzero(m)], fx.delta)
            worst = max(worst, abs(float(area.sum()) - float(areas[k])) / gate)
            assert abs(float(area.sum()) - float(areas[k])) <= gate, (fx.n, k, float(area.sum()), float(areas[k]), gate)
            assert r.mask[k, 2] <= 2 * sum(fx.rings[i].shape[0] for i in np.flatnonzero(m))
            longest = max(longest, int(rows[:, 1].max()))
        print(f"\nunion_contour lattice masks ({fx.n} tiles): rings {r.mask[:, 0].tolist()}, points {r.mask[:, 2].tolist()}, "
              f"worst |sum of ring areas - union area| / gate {worst:.3g}")
    assert longest >= 76


# ------------------------------------------------------------------------------------------------ bits, shapes, slices
def test_same_bits_on_a_second_call_and_on_a_dirty_workspace(ring9):
    masks = [to.thinned_set(ring9.n, ring9.col, seed) for seed in to.SEEDS] + [np.zeros(ring9.n, dtype=bool)]
    a, b = ring9.gpu(masks), ring9.gpu(masks)
    assert _bytes(a) == _bytes(b) and a.mask[-1, [0, 2, 3]].tolist() == [0, 0, 0]
    for k in (0, 7):                                                        # a mask's rings do not depend on its neighbours
        one = ring9.gpu(masks[k])
        rings, first, points = int(a.mask[k, 0]), int(a.mask[k, 1]), int(a.mask[k, 2])
        p0 = int(a.ring[first, 0])
        assert one.mask[0].tolist() == [rings, 0, points, 0]
        assert (one.ring[:, 1:] == a.ring[first:first + rings, 1:]).all() and (one.ring[:, 0] == a.ring[first:first + rings, 0] - p0).all()
        assert one.area.tobytes() == a.area[first:first + rings].tobytes()
        assert one.xy.tobytes() == a.xy[p0:p0 + points].tobytes() and one.src.tobytes() == a.src[p0:p0 + points].tobytes()
    clean = _abi(ring9.rings, masks, pairs=ring9.col)
    dirty = _abi(ring9.rings, masks, pairs=ring9.col, ws_fill=0x7F)
    again = _abi(ring9.rings, masks, pairs=ring9.col, ws_fill=0xFF)
    assert clean.err == dirty.err == again.err == 0
    assert _bytes(clean) == _bytes(dirty) == _bytes(again) == _bytes(a)
    none = ring9.on_device.union_contours(torch.zeros(0, ring9.n, dtype=torch.int32, device=DEV))
    assert len(none) == 0 and none.mask.shape == (0, 4) and none.pts_xy.shape == (0, 2)
    assert len(ring9.on_device.union_contours(torch.from_numpy(masks[0]).to(DEV))) == 1        # a bool mask, one row
    with pytest.raises(ValueError):
        ring9.on_device.union_contours(torch.zeros(2, ring9.n + 1, dtype=torch.int32, device=DEV))


def test_more_masks_than_one_grid_holds(small):
    """K = 65 535 + 5: single tiles repeated, and five thinned masks on both sides of the 65 535 boundary."""
    k = 65535 + 5
    alive = torch.zeros(k, small.n, dtype=torch.int32, device=DEV)
    rows = torch.arange(k, device=DEV)
    alive[rows, rows % small.n] = 1
    special = {65533: to.thinned_set(small.n, small.col, 3), 65534: to.thinned_set(small.n, small.col, 1),
               65535: to.thinned_set(small.n, small.col, 3), 65536: to.thinned_set(small.n, small.col, 1),
               65539: to.thinned_set(small.n, small.col, 5)}
    for row, m in special.items():
        alive[row] = torch.from_numpy(m.astype(np.int32)).to(DEV)
    r = small.gpu(alive.cpu().numpy())
    plain = np.ones(k, dtype=bool)
    plain[list(special)] = False
    verts = np.array([ring.shape[0] for ring in small.rings])[np.arange(k) % small.n]
    assert (r.mask[plain, 0] == 1).all() and (r.mask[plain, 2] == verts[plain]).all() and (r.mask[:, 3] == 0).all()
    assert r.mask[:, 1].tolist() == np.concatenate([[0], np.cumsum(r.mask[:-1, 0])]).tolist()
    single = np.flatnonzero(plain)[[0, 1, small.n + 3, -1]]
    for row in single:                                                      # a single tile is its own ring, vertex for vertex
        first = int(r.mask[row, 1])
        p0, count, label, sign = r.ring[first].tolist()
        t = row % small.n
        assert (label, sign, count) == (t, 1, small.rings[t].shape[0])
        assert r.src[p0:p0 + count].tolist() == list(range(r.ring_ptr[t], r.ring_ptr[t + 1]))
    for row, m in special.items():
        _check_mask(r, row, small.want(m), m, row)
    a, b = (r.ring[int(r.mask[row, 1]):int(r.mask[row, 1]) + int(r.mask[row, 0]), 1:] for row in (65533, 65535))
    assert (a == b).all()


# ------------------------------------------------------------------------------------------------ capacity
def test_capacity_one_point_short_then_sized_from_the_totals(ring9):
    masks = [to.thinned_set(ring9.n, ring9.col, seed) for seed in (0, 1)] + [to.independent_set(ring9.n, ring9.col, 0)]
    full = _abi(ring9.rings, masks, pairs=ring9.col)
    rings, points = (int(v) for v in full.total)
    assert full.err == 0 and rings > 70 and points > 400 and points < full.cap[1]
    bound = full.cap[1]
    short = _abi(ring9.rings, masks, pairs=ring9.col, cap=(rings, points - 1), max_pieces=bound)    # (_abi checks the canaries)
    assert short.err == 8
    assert short.total.tolist() == [rings, points] and short.mask.tobytes() == full.mask.tobytes()
    assert short.xy[:points - 1].tobytes() == full.xy[:points - 1].tobytes()
    few = _abi(ring9.rings, masks, pairs=ring9.col, cap=(rings - 1, points), max_pieces=bound)
    assert few.err == 8 and few.total.tolist() == [rings, points] and few.ring[:rings - 1].tobytes() == full.ring[:rings - 1].tobytes()
    exact = _abi(ring9.rings, masks, pairs=ring9.col, cap=(rings, points), max_pieces=bound)
    assert exact.err == 0 and _bytes(exact) == _bytes(full)


# ------------------------------------------------------------------------------------------------ limits
def _fan(count):
    """Thin triangles fanned around the origin, which is a vertex of every one."""
    return [np.array([[0, 0], [math.cos(t), math.sin(t)], [math.cos(t + 0.2), math.sin(t + 0.2)]]) for t in 0.3 + 0.36 * np.arange(count)]


def test_error_bits_splits_wedges_index():
    from tilingnn_amd._lib import TgnnError
    from tilingnn_amd.tiling.region import contact_geometry, union_geometry
    from tilingnn_amd.util.data_util import CompleteGraphOnDevice
    limit = _max_splits()
    tiles = co.extra_sets(limit)["comb past the limit"][0]
    r = _abi(tiles, [np.ones(len(tiles))])
    assert r.err & 4 and not r.err & ~(4 | 16)                              # SPLITS (and the ring the dropped split leaves open)
    fewer = np.ones(len(tiles), dtype=np.int32)
    fewer[-2:] = 0                                                          # two squares less: `limit` splits, which fit
    r = _abi(tiles, [fewer])
    assert r.err == 0 and r.mask[0].tolist() == [1, 0, 6, 0]
    # 16 tiles around one point fit the list of leaving pieces, 17 do not
    fan = _fan(17)
    r = _abi(fan, [np.array([1] * 16 + [0]), np.array([0] + [1] * 16)])
    assert r.err == 0 and r.mask[:, [0, 2, 3]].tolist() == [[1, 48, 0], [1, 48, 0]]
    _check_mask(r, 0, Want(fan[:16]), [1] * 16 + [0], "fan")
    r = _abi(fan, [np.array([1] * 16 + [0]), np.ones(17)])
    assert r.err & 2 and not r.err & ~(2 | 16)
    # an index out of range
    tiles = to.hand_sets()["pinwheel"][0]
    geo = union_geometry(tiles, np.zeros((2, 0), dtype=np.int64), 4)
    touch_ptr, touch_idx = contact_geometry(geo[0], geo[1])
    for wrong in (4, -1, 2 ** 31 - 1):
        broken = touch_idx.copy()
        broken[1] = wrong
        assert _abi(tiles, [np.ones(4)], touch=(touch_ptr, broken)).err & 1, wrong
    # ... and the binding raises on a bit, naming it
    geo = union_geometry(fan, np.zeros((2, 0), dtype=np.int64), 17)
    od = CompleteGraphOnDevice.__new__(CompleteGraphOnDevice)
    od.device, od.n_tiles = torch.device(DEV), 17
    up = lambda a: torch.from_numpy(a if a.size else np.zeros(1, dtype=a.dtype)).to(DEV)
    od._union = tuple(up(a) for a in geo)
    od._topology = tuple(up(a) for a in contact_geometry(geo[0], geo[1])) + (math.cos(0.1234), math.sin(0.1234))
    assert od.union_contours(torch.tensor([1] * 16 + [0], device=DEV)).mask.cpu().tolist() == [[1, 0, 48, 0]]
    with pytest.raises(TgnnError, match="wedge"):
        od.union_contours(torch.ones(17, dtype=torch.int32, device=DEV))


@pytest.mark.parametrize("extra", [0, 1])
def test_masks_either_side_of_the_lds_limit(extra):
    """The trace's working arrays live in LDS for masks of up to CONTOUR_LDS_PIECES boundary pieces and in the workspace beyond:
    a row of separated unit squares, four pieces each, with exactly that many pieces (the last size of the first path), and one
    more square (the first size of the second).  By hand: n rings of 4 points, area 1 each, in tile order."""
    from tilingnn_amd.tiling.region import CONTOUR_LDS_PIECES
    assert CONTOUR_LDS_PIECES % 4 == 0
    n = CONTOUR_LDS_PIECES // 4 + extra
    tiles = [to._box(2 * x, 0, 2 * x + 1, 1) for x in range(n)]
    half = (np.arange(n) % 2 == 0).astype(np.int32)
    r = _abi(tiles, [np.ones(n, dtype=np.int32), half], ws_fill=0x55)
    assert r.err == 0 and r.mask.tolist() == [[n, 0, 4 * n, 0], [(n + 1) // 2, n, 4 * ((n + 1) // 2), 0]]
    assert r.ring[:n].tolist() == [[4 * t, 4, t, 1] for t in range(n)] and (r.area[:n] == 1.0).all()
    assert r.src[:4 * n].tolist() == list(range(4 * n)) and r.xy[:4 * n].tobytes() == r.ring_xy.tobytes()
    assert r.ring[n:n + (n + 1) // 2, 2].tolist() == list(range(0, n, 2))


def test_abi_rejects_bad_arguments():
    from tilingnn_amd._lib import lib
    args = lambda *a: lib.tgnn_union_contour(*a)
    none = (None,) * 7
    assert args(None, None, 4, None, None, None, None, None, 2, TOL, 0, 0, *none, None, 0, None) == -1
    assert b"tgnn_union_contour" in lib.tgnn_last_error()
    assert args(None, None, 4, None, None, None, None, None, 0, TOL, 0, 0, *none, None, 0, None) == 0
    assert args(None, None, -1, None, None, None, None, None, 0, TOL, 0, 0, *none, None, 0, None) == -1
    f64 = torch.zeros(64, dtype=torch.float64, device=DEV)
    i32 = torch.zeros(64, dtype=torch.int32, device=DEV)
    p = lambda t: t.data_ptr()
    full = lambda tol, cap, ws_bytes: args(p(f64), p(i32), 4, p(i32), p(i32), p(i32), p(i32), p(i32), 2, tol, cap, cap, p(i32),
                                           p(i32), p(f64), p(f64), p(i32), p(f64), p(i32), p(f64), ws_bytes, None)
    assert full(TOL, 4, 8) == -1                                            # a workspace that is too small
    assert full(-1.0, 4, 512) == -1 and full(float("nan"), 4, 512) == -1 and full(TOL, -1, 512) == -1
    assert lib.tgnn_union_contour_workspace_bytes(2, 4, 10) == 2 * (3 * 8 + 4 * 4 + 9 * 4) + 10 * 13 * 4
    assert lib.tgnn_union_contour_workspace_bytes(0, 4, 10) == 0


# ------------------------------------------------------------------------------------------------ BrickLayout
def _solved_layout(fx, selection, seed):
    """A layout cut from the complete graph around `selection` (the selected tiles and a random half of the others), with
    `predict` = the selection."""
    from tilingnn_amd.tiling.brick_layout import BrickLayout
    from tilingnn_amd.util import data_util as du
    keep = selection | (np.random.default_rng(seed).random(fx.n) < 0.5)
    tiles = np.flatnonzero(keep)
    layout = BrickLayout(fx.graph, *du.create_brick_layout_from_super_set(fx.graph, tiles.tolist()))
    layout.predict = np.array([1.0 if selection[layout.inverse_index[i]] else 0.0 for i in range(tiles.size)])
    return layout


def _reference_selections(ring9, small):
    ref, greedy = load_npz("ref_scores.npz"), load_npz("ref_greedy.npz")
    out = [(ring9, np.asarray(greedy[f"{k}.selection"]) == 1) for k in ("greedy0", "greedy7")]
    for case in ["all", "first80", "random60"]:
        m = np.zeros(small.n, dtype=bool)
        m[ref[f"{case}.super_tiles"][np.asarray(ref[f"{case}.predict"]) > 0]] = True
        out.append((small, m))
    return out


def test_brick_layout_union_polygon_on_reference_selections(ring9, small):
    from tilingnn_amd.tiling.brick_layout import union_polygons_many
    from tilingnn_amd.tiling.region import Region
    for fx in (ring9, small):
        picks = [m for f, m in _reference_selections(ring9, small) if f is fx]
        layouts = [_solved_layout(fx, m, 11 + q) for q, m in enumerate(picks)]
        many = union_polygons_many(layouts, DEV)
        areas = fx.on_device.union_areas(fx.dev(picks)).cpu().numpy()
        for q, (layout, m, polys) in enumerate(zip(layouts, picks, many)):
            single = layout.get_selected_tiles_union_polygon(DEV)
            assert len(single) == len(polys) and all(isinstance(p, Region) for p in polys)
            for a, b in zip(single, polys):
                assert a.exterior.tobytes() == b.exterior.tobytes() and len(a.interiors) == len(b.interiors)
                assert all(x.tobytes() == y.tobytes() for x, y in zip(a.interiors, b.interiors))
            comps, holes = layout.count_holes(DEV)
            assert len(polys) == comps and sum(len(p.interiors) for p in polys) == holes, (fx.n, q)
            gate = uo.gate([fx.rings[i] for i in np.flatnonzero(m)], fx.delta)
            assert abs(sum(p.area for p in polys) - float(areas[q])) <= gate, (fx.n, q)
            want = fx.want(m)
            assert sorted(p.exterior.shape[0] for p in polys) == sorted(c for c, s in zip(want.counts, want.signs) if s > 0)
    assert union_polygons_many([]) == []
    with pytest.raises(ValueError, match="one complete graph"):
        union_polygons_many([_solved_layout(ring9, to.independent_set(ring9.n, ring9.col, 0), 0),
                             _solved_layout(small, to.independent_set(small.n, small.col, 0), 0)])


def test_brick_layout_union_polygon_refuses_a_colliding_selection(ring9):
    from tilingnn_amd.tiling.brick_layout import union_polygons_many
    clash = np.zeros(ring9.n, dtype=bool)
    clash[ring9.col[:, 0]] = True
    with pytest.raises(ValueError, match="collide"):
        _solved_layout(ring9, clash, 4).get_selected_tiles_union_polygon()
    good = _solved_layout(ring9, to.thinned_set(ring9.n, ring9.col, 0), 0)
    with pytest.raises(ValueError, match="layout 1"):
        union_polygons_many([good, _solved_layout(ring9, clash, 4)])
    polys = good.get_selected_tiles_union_polygon()
    assert len(polys) == 1 and len(polys[0].interiors) == 40                # (topology_oracle.QUOTED, ring 9 thinned, seed 0)
    unsolved = _solved_layout(ring9, clash, 3)
    unsolved.predict[:] = 0
    assert unsolved.get_selected_tiles_union_polygon() == []
