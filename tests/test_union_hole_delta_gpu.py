"""What every candidate tile would do to the components and holes of a selection, on the GPU (csrc/union_hole_delta.hip:
tgnn_union_hole_delta, `CompleteGraphOnDevice.hole_deltas`), against its definition -- tgnn_union_topology(mask + {t}) -
tgnn_union_topology(mask) -- taken three ways: from the loop-tracing oracle's table of every subset of fifteen hand-made sets
(tests/hole_delta_cases.py), by brute force on the device (one union_topology call over all (mask + t) rows), and from the host
oracle on two ring-9 masks.  Every comparison is exact integer equality.  The per-candidate code itself runs on the host under
sanitizers in tests/test_union_hole_delta_host.py."""
import gzip
import math
import os
import shutil

import numpy as np
import pytest
import torch

from tests import hole_delta_cases as hc
from tests import topology_oracle as to
from tests.golden_util import GOLDEN

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
TOL = 1e-6
CANDIDATE, ALIVE, BLOCKED, REFUSED = 0, 1, 2, 3


def _abi(tiles, masks, pairs=None, touch=None, theta=None, ws_fill=None):
    """tgnn_union_hole_delta straight from arrays (the arguments of tests/test_union_topology_gpu.py: _abi).  Returns
    (delta [K, n, 2], state [K, n], error word); both outputs are filled with -7 first: every word must be written."""
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
    delta = torch.full((k, n, 2), -7, dtype=torch.int32, device=DEV)
    state = torch.full((k, n), -7, dtype=torch.int32, device=DEV)
    err = torch.zeros(1, dtype=torch.int32, device=DEV)
    ws_bytes = int(lib.tgnn_union_hole_delta_workspace_bytes(k, n))
    assert ws_bytes == 4 * k * (n + 1)
    ws = torch.zeros(max(ws_bytes, 1), dtype=torch.uint8, device=DEV)
    if ws_fill is not None:
        ws.fill_(ws_fill)
    check(lib.tgnn_union_hole_delta(ptr(dev[0]), ptr(dev[1]), n, *(ptr(a) for a in dev[2:]), ptr(masks), k, TOL, math.cos(theta),
                                    math.sin(theta), ptr(delta), ptr(state), ptr(err), ptr(ws), ws_bytes,
                                    _lib.current_stream(torch.device(DEV))))
    torch.cuda.synchronize()
    return delta.cpu().numpy(), state.cpu().numpy(), int(err.item())


# ------------------------------------------------------------------------------------------------ 1. hand-made sets, every subset
@pytest.mark.parametrize("angle", to.ROTATIONS)
def test_hand_sets_every_subset(angle):
    seen = set()
    for name, tiles in hc.sets().items():
        n = len(tiles)
        masks = hc.all_subsets(n)
        _, want = hc.subset_table(name, tiles)
        delta, state, err = _abi(to.rotated(tiles, angle), masks)
        assert err == 0, name
        assert (state == masks).all(), name                                # no collision: alive 1, every other tile a candidate
        assert (delta[0] == np.array([1, 0])).all(), name                  # the empty mask
        bad = np.argwhere((delta != want).any(axis=2))
        assert bad.size == 0, (name, angle, bad[0].tolist(), delta[tuple(bad[0])].tolist(), want[tuple(bad[0])].tolist())
        seen |= set(hc.pair_counts(delta, masks))
    assert seen == hc.PAIRS


_OVERLAP = {}


def _overlap_case():
    """The 3 x 3 ring of squares and two rectangles that overlap each other (tests/test_union_topology_gpu.py:
    test_overlapping_tiles_are_reported_not_answered): masks, the 256 with both, and the oracle's (components, holes) of the rest."""
    if not _OVERLAP:
        tiles = to.hand_sets()["3x3 without the centre"][0] + [hc.box(3, 0, 5, 1), hc.box(4, 0, 6, 1)]
        masks = hc.all_subsets(10)
        both = (masks[:, 8] & masks[:, 9]) != 0
        want = np.array([(0, 0) if b else to.topology([tiles[i] for i in np.flatnonzero(m)]) for m, b in zip(masks, both)],
                        dtype=np.int32)
        want.setflags(write=False)
        _OVERLAP.update(tiles=tiles, masks=masks, both=both, want=want)
    return _OVERLAP["tiles"], _OVERLAP["masks"], _OVERLAP["both"], _OVERLAP["want"]


@pytest.mark.parametrize("angle", to.ROTATIONS)
def test_overlapping_tiles_refused_and_blocked(angle):
    tiles, masks, both, want = _overlap_case()
    delta, state, err = _abi(to.rotated(tiles, angle), masks, pairs=np.array([[8], [9]]))
    assert err == 0 and both.sum() == 256
    assert (state[both] == REFUSED).all() and (delta[both] == 0).all()     # the whole row
    ok = ~both
    expect = masks.copy()
    expect[ok & (masks[:, 8] != 0), 9] = BLOCKED                           # the partner of an alive one
    expect[ok & (masks[:, 9] != 0), 8] = BLOCKED
    assert (state[ok] == expect[ok]).all()
    assert (state[ok] == BLOCKED).sum() == 512
    for m in np.flatnonzero(ok):
        for t in range(10):
            if state[m, t] == CANDIDATE:
                assert delta[m, t].tolist() == (want[m | (1 << t)] - want[m]).tolist(), (m, t)
            else:
                assert delta[m, t].tolist() == [0, 0], (m, t)


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
        delta, state = self.on_device.hole_deltas(torch.from_numpy(masks).to(DEV))
        assert delta.dtype == torch.int32 and state.dtype == torch.int32
        assert delta.shape == (masks.shape[0], self.n, 2) and state.shape == (masks.shape[0], self.n)
        return delta.cpu().numpy(), state.cpu().numpy()

    def topology(self, masks):
        masks = np.ascontiguousarray(np.asarray(masks).reshape(-1, self.n), dtype=np.int32)
        return self.on_device.union_topology(torch.from_numpy(masks).to(DEV)).cpu().numpy()

    def expected_state(self, mask):
        """By the collision edge list: alive 1, a collision neighbour of an alive tile 2, else 0."""
        state = np.zeros(self.n, dtype=np.int32)
        state[self.col[1][mask[self.col[0]]]] = BLOCKED
        assert not state[mask].any()
        state[mask] = ALIVE
        return state

    def half_solution(self, seed):
        idx = np.flatnonzero(to.independent_set(self.n, self.col, seed))
        mask = np.zeros(self.n, dtype=bool)
        mask[np.random.default_rng(200 + seed).permutation(idx)[:len(idx) // 2]] = True
        return mask

    def sparse(self):
        mask = np.zeros(self.n, dtype=bool)
        mask[np.flatnonzero(to.independent_set(self.n, self.col, 0))[:5]] = True
        return mask


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
    """8 maximal independent sets, 8 thinned ones, 8 half solutions, a very sparse mask, the empty mask: 26."""
    masks = [make(fx.n, fx.col, seed) for make in (to.independent_set, to.thinned_set) for seed in to.SEEDS]
    masks += [fx.half_solution(seed) for seed in to.SEEDS] + [fx.sparse(), np.zeros(fx.n, dtype=bool)]
    assert len(masks) == 26
    return masks


@pytest.mark.parametrize("which", ["small", "ring9"])
def test_lattice_masks_against_the_definition_on_the_device(which, request):
    """delta == union_topology(mask + t) - union_topology(mask) for every candidate of 26 masks, the right side by ONE
    union_topology call over all the (mask + t) rows."""
    fx = request.getfixturevalue(which)
    masks = _lattice_masks(fx)
    delta, state = fx.gpu(masks)
    for k, m in enumerate(masks):
        assert (state[k] == fx.expected_state(m)).all(), k
    assert (delta[state != CANDIDATE] == 0).all()
    assert np.isin(state[:8], (ALIVE, BLOCKED)).all()                      # a maximal independent set has no candidate at all
    assert (state[25] == CANDIDATE).all() and (delta[25] == np.array([1, 0])).all()     # the empty mask
    ks, ts = np.nonzero(state == CANDIDATE)
    rows = np.stack(masks).astype(np.int32)[ks]
    rows[np.arange(ks.size), ts] = 1
    base = fx.topology(masks)
    after = fx.topology(rows)
    assert (base[:, 2] == 0).all() and (after[:, 2] == 0).all()
    want = after[:, :2] - base[ks, :2]
    got = delta[ks, ts]
    bad = np.flatnonzero((got != want).any(axis=1))
    assert bad.size == 0, (which, int(ks[bad[0]]), int(ts[bad[0]]), got[bad[0]].tolist(), want[bad[0]].tolist())
    lonely = (got == np.array([1, 0])).all(axis=1)
    print(f"\nunion_hole_delta {which}: {ks.size} candidates over 26 masks, d holes {dict(zip(*np.unique(got[:, 1], return_counts=True)))}, "
          f"{int(lonely[ks == 24].sum())} of the sparse mask's {int((ks == 24).sum())} are {{+1, 0}}")
    # the sparse mask: on ring 9 most candidates touch nothing (counted on the host from the contact rows alone)
    assert (int(lonely[ks == 24].sum()), int((ks == 24).sum())) == {"ring9": (1136, 1221), "small": (34, 113)}[which]
    assert got[:, 1].min() < 0 < got[:, 1].max()


@pytest.mark.parametrize("kind,count,hist", [("thinned", 119, {-1: 27, 0: 66, 1: 24, 2: 2}),
                                             ("half", 335, {-1: 15, 0: 138, 1: 143, 2: 39})])
def test_ring9_against_the_host_oracle(kind, count, hist, ring9):
    """Every candidate of two ring-9 masks against the loop-tracing oracle; the counts were measured with the oracle on the host
    when the kernel was designed and are quoted as a cross-check of the recipes."""
    fx = ring9
    mask = to.thinned_set(fx.n, fx.col, 0) if kind == "thinned" else fx.half_solution(0)
    delta, state = fx.gpu(mask)
    cands = np.flatnonzero(state[0] == CANDIDATE)
    assert cands.size == count
    chosen = [fx.rings[i] for i in np.flatnonzero(mask)]
    base = np.array(to.topology(chosen))
    for t in cands:
        want = np.array(to.topology(chosen + [fx.rings[t]])) - base
        assert delta[0, t].tolist() == want.tolist(), (kind, int(t))
    values, counts = np.unique(delta[0, cands, 1], return_counts=True)
    assert dict(zip(values.tolist(), counts.tolist())) == hist


# ------------------------------------------------------------------------------------------------ bits, shapes, slices
def test_same_bytes_on_a_second_call_and_on_a_dirty_workspace(ring9):
    masks = [to.thinned_set(ring9.n, ring9.col, seed) for seed in to.SEEDS] + [np.zeros(ring9.n, dtype=bool)]
    a, b = ring9.gpu(masks), ring9.gpu(masks)
    assert a[0].tobytes() == b[0].tobytes() and a[1].tobytes() == b[1].tobytes()
    for k in (0, 7):                                                        # a row does not depend on its neighbours in the batch
        one = ring9.gpu(masks[k])
        assert one[0].tobytes() == a[0][k:k + 1].tobytes() and one[1].tobytes() == a[1][k:k + 1].tobytes()
    runs = [_abi(ring9.rings, masks, pairs=ring9.col, theta=0.1234, ws_fill=fill) for fill in (None, 0x7F, 0xFF)]
    for delta, state, err in runs:
        assert err == 0 and delta.tobytes() == a[0].tobytes() and state.tobytes() == a[1].tobytes()
    none = ring9.on_device.hole_deltas(torch.zeros(0, ring9.n, dtype=torch.int32, device=DEV))
    assert none[0].shape == (0, ring9.n, 2) and none[1].shape == (0, ring9.n)
    one = ring9.on_device.hole_deltas(torch.from_numpy(masks[0]).to(DEV))  # a bool mask, one row
    assert one[0].shape == (1, ring9.n, 2) and one[1].shape == (1, ring9.n)
    with pytest.raises(ValueError):
        ring9.on_device.hole_deltas(torch.zeros(2, ring9.n + 1, dtype=torch.int32, device=DEV))


def test_more_masks_than_one_grid_holds(small):
    """K = 65 535 + 5: single tiles repeated, and masks with known rows on both sides of the slice boundary."""
    k = 65535 + 5
    alive = torch.zeros(k, small.n, dtype=torch.int32, device=DEV)
    rows = torch.arange(k, device=DEV)
    alive[rows, rows % small.n] = 1
    special = {65533: to.thinned_set(small.n, small.col, 3), 65534: to.thinned_set(small.n, small.col, 1),
               65535: small.half_solution(3), 65536: to.thinned_set(small.n, small.col, 1), 65539: small.half_solution(5)}
    for row, m in special.items():
        alive[row] = torch.from_numpy(m.astype(np.int32)).to(DEV)
    delta, state = small.on_device.hole_deltas(alive)
    singles = small.gpu(np.eye(small.n, dtype=np.int32))
    known = {row: small.gpu(m) for row, m in special.items()}
    delta, state = delta.cpu().numpy(), state.cpu().numpy()
    plain = np.ones(k, dtype=bool)
    plain[list(special)] = False
    which = np.arange(k) % small.n
    assert (delta[plain] == singles[0][which[plain]]).all() and (state[plain] == singles[1][which[plain]]).all()
    for row, (d, s) in known.items():
        assert (delta[row] == d[0]).all() and (state[row] == s[0]).all(), row
    assert (state[65535] == CANDIDATE).any() and (state[65536] == CANDIDATE).any()


@pytest.mark.parametrize("extra", [0, 1])
def test_graphs_either_side_of_the_lds_limit(extra):
    """The labels live in LDS for graphs of up to 6 144 tiles and in the workspace beyond: a 96 x 64 grid of unit squares and the
    same grid with one more (alive) square far away.  By reasoning on the cells: under `sieve` (every interior (odd, odd) cell
    removed, each a hole of its own) a removed cell plugs its hole, {0, -1}; under `dots` (the (even, even) cells alone, no two
    touching) an interior (odd, odd) cell joins its four corner neighbours, {-3, 0}, an interior (odd, even) or (even, odd) cell
    its two side neighbours, {-1, 0}."""
    w, h = 96, 64
    x, y = [c.reshape(-1) for c in np.meshgrid(np.arange(w), np.arange(h))]
    tiles = [hc.box(a, b, a + 1, b + 1) for a, b in zip(x, y)] + [hc.box(200, 0, 201, 1)] * extra
    inside = (x >= 1) & (x <= w - 2) & (y >= 1) & (y <= h - 2)
    sieve = ~((x % 2 == 1) & (y % 2 == 1) & inside)
    dots = (x % 2 == 0) & (y % 2 == 0)
    masks = np.stack([sieve, dots]).astype(np.int32)
    masks = np.concatenate([masks, np.ones((2, extra), dtype=np.int32)], axis=1)
    delta, state, err = _abi(tiles, masks, ws_fill=0x55)
    assert err == 0 and (state == masks).all()
    g = w * h
    assert (~sieve).sum() == 47 * 31 and (delta[0, :g][~sieve] == np.array([0, -1])).all() and (delta[0][masks[0] != 0] == 0).all()
    odd_odd = (x % 2 == 1) & (y % 2 == 1) & inside
    mixed = ((x + y) % 2 == 1) & inside
    assert odd_odd.sum() == 47 * 31 and mixed.sum() == 94 * 62 // 2
    assert (delta[1, :g][odd_odd] == np.array([-3, 0])).all() and (delta[1, :g][mixed] == np.array([-1, 0])).all()
    assert (delta[1][masks[1] != 0] == 0).all()


def test_abi_rejects_bad_arguments():
    from tilingnn_amd._lib import lib
    args = lambda *a: lib.tgnn_union_hole_delta(*a)
    assert args(None, None, 4, None, None, None, None, None, 2, TOL, 1.0, 0.0, None, None, None, None, 0, None) == -1
    assert b"tgnn_union_hole_delta" in lib.tgnn_last_error()
    assert args(None, None, 4, None, None, None, None, None, 0, TOL, 1.0, 0.0, None, None, None, None, 0, None) == 0
    assert args(None, None, -1, None, None, None, None, None, 0, TOL, 1.0, 0.0, None, None, None, None, 0, None) == -1
    f64 = torch.zeros(64, dtype=torch.float64, device=DEV)
    i32 = torch.zeros(64, dtype=torch.int32, device=DEV)
    p = lambda t: t.data_ptr()
    full = lambda tol, dx, dy, ws_bytes: args(p(f64), p(i32), 4, p(i32), p(i32), p(i32), p(i32), p(i32), 2, tol, dx, dy, p(i32),
                                              p(i32), p(i32), p(i32), ws_bytes, None)
    assert full(TOL, 1.0, 0.0, 8) == -1                                     # a workspace that is too small
    assert full(-1.0, 1.0, 0.0, 256) == -1 and full(TOL, 0.5, 0.5, 256) == -1 and full(TOL, float("nan"), 0.0, 256) == -1
    assert lib.tgnn_union_hole_delta_workspace_bytes(2, 4) == 2 * (4 + 1) * 4
    assert lib.tgnn_union_hole_delta_workspace_bytes(0, 4) == 0


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
    masks = [np.ones(4), np.array([1, 1, 1, 0])]
    delta, state, err = _abi(tiles, masks, touch=(touch_ptr, touch_idx))
    assert err == 0 and delta[1, 3].tolist() == [0, 1] and state[1].tolist() == [1, 1, 1, 0]     # the fourth arm closes the pinwheel
    for wrong in (4, -1, 2 ** 31 - 1):
        broken = touch_idx.copy()
        broken[1] = wrong
        _, _, err = _abi(tiles, masks, touch=(touch_ptr, broken))
        assert err == 1, wrong
    # with the candidate counted, 16 tiles around one point fit the wedge list and 17 do not.  15 alive + 1: the candidate joins
    # the one component it touches and a fan around a point encloses nothing: {0, 0}, worked out by hand
    fan = _fan(17)
    delta, state, err = _abi(fan, [np.array([1] * 15 + [0, 0]), np.array([0, 0] + [1] * 15)], theta=0.1234)
    assert err == 0 and state.tolist() == [[1] * 15 + [0, 0], [0, 0] + [1] * 15] and (delta == 0).all()
    _, _, err = _abi(fan, [np.array([1] * 15 + [0, 0]), np.array([1] * 16 + [0])], theta=0.1234)
    assert err == 2
    # ... which the binding raises on
    geo = union_geometry(fan, np.zeros((2, 0), dtype=np.int64), 17)
    od = CompleteGraphOnDevice.__new__(CompleteGraphOnDevice)
    od.device, od.n_tiles = torch.device(DEV), 17
    up = lambda a: torch.from_numpy(a if a.size else np.zeros(1, dtype=a.dtype)).to(DEV)
    od._union = tuple(up(a) for a in geo)
    od._topology = tuple(up(a) for a in contact_geometry(geo[0], geo[1])) + (math.cos(0.1234), math.sin(0.1234))
    delta, state = od.hole_deltas(torch.tensor([1] * 15 + [0, 0], device=DEV))
    assert (delta == 0).all().item() and state.cpu().tolist() == [[1] * 15 + [0, 0]]
    with pytest.raises(TgnnError, match="wedge"):
        od.hole_deltas(torch.tensor([1] * 16 + [0], device=DEV))
