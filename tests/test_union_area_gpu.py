"""The area of a union of tiles on the GPU (csrc/union_area.hip: tgnn_union_area) against exact properties and the slab-sweep
oracle of tests/union_oracle.py, and the crop coverage / crop scores built on it.

Gate (groups 1-5, 7): |gpu - expected| <= delta * P + 64 eps R^2 n_edges, with P the summed perimeter of the alive tiles, R the
largest coordinate magnitude, eps = 2^-53 and delta the largest vertex-to-side distance below the tolerance among the
fixture's colliding and adjacent tiles, measured here from the fixture (3.12e-8 for ring 9, 7.5e-9 for the small graph, 0 for
the synthetic tiles): two correct treatments of nearly coincident sides differ by slivers at most delta wide.  Derived, not
tuned; one missed overlap moves 0.018.  Every group prints its worst gap and worst gap / gate before it asserts
(profiles/union_area_gaps.txt records them)."""
import copy
import gzip
import os
import random
import shutil

import numpy as np
import pytest
import torch

from tests import region_oracle as orc
from tests import union_oracle as uo
from tests.golden_util import GOLDEN, load_npz

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
SIL = os.path.join(GOLDEN, "silhouettes")
TOL = 1e-6
CROP_KW = dict(start_angle=0.0, end_angle=60.0, num_of_angle=3, movement_delta_ratio=[0, 0.5], margin_padding_ratios=[0.5, 0.05])


class Fixture:
    def __init__(self, graph):
        from tilingnn_amd.util.data_util import graph_on_device
        self.graph = graph
        self.rings = [np.asarray(t.tile_poly.exterior)[:-1] for t in graph.tiles]
        self.n = len(self.rings)
        self.areas = graph.arrays.tile_areas
        self.on_device = graph_on_device(graph, DEV)
        a = graph.arrays
        self.delta = uo.noise_width(self.rings, np.concatenate([a.colli_edges, a.adj_edges], axis=1), TOL)

    def gpu(self, masks):
        masks = np.ascontiguousarray(np.asarray(masks).reshape(-1, self.n), dtype=np.int32)
        return self.on_device.union_areas(torch.from_numpy(masks).to(DEV)).cpu().numpy()

    def gate(self, mask):
        return uo.gate([self.rings[i] for i in np.flatnonzero(mask)], self.delta)

    def oracle(self, mask):
        return uo.union_area([self.rings[i] for i in np.flatnonzero(mask)])


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


def _report(name, gaps, gates):
    gaps, gates = np.asarray(gaps, dtype=float), np.asarray(gates, dtype=float)
    k = int(np.argmax(gaps / gates))
    print(f"\nunion_area {name}: {gaps.size} cases, worst gap {gaps.max():.3e}, worst gap/gate {gaps[k] / gates[k]:.3e} "
          f"(gap {gaps[k]:.3e}, gate {gates[k]:.3e})")
    assert (gaps <= gates).all(), (name, k, float(gaps[k]), float(gates[k]))


def test_measured_noise_width(ring9, small):
    print(f"\nunion_area delta: ring 9 {ring9.delta:.4e}, small graph {small.delta:.4e}")
    assert 0 < ring9.delta < TOL / 10 and 0 < small.delta < TOL / 10


# ------------------------------------------------------------------------------------------------ 1. single tiles
@pytest.mark.parametrize("which", ["ring9", "small"])
def test_single_tile_masks_give_the_tile_area(which, request):
    fx = request.getfixturevalue(which)
    got = fx.gpu(np.eye(fx.n, dtype=np.int32))
    _report(f"1 single tiles {which}", np.abs(got - fx.areas), [fx.gate(m) for m in np.eye(fx.n, dtype=bool)])


# ------------------------------------------------------------------------------------------------ 2. collision-free selections
def _independent_set(fx, seed):
    col = fx.graph.arrays.colli_edges
    rng = np.random.default_rng(seed)
    blocked, mask = np.zeros(fx.n, dtype=bool), np.zeros(fx.n, dtype=bool)
    order = np.argsort(col[0], kind="stable")
    starts = np.searchsorted(col[0][order], np.arange(fx.n + 1))
    for i in rng.permutation(fx.n):
        if not blocked[i]:
            mask[i] = True
            blocked[i] = True
            blocked[col[1][order[starts[i]:starts[i + 1]]]] = True
    assert not (mask[col[0]] & mask[col[1]]).any() and blocked.all()
    return mask


def test_collision_free_selections_give_the_sum_of_areas(ring9, small):
    ref = load_npz("ref_scores.npz")
    col = small.graph.arrays.colli_edges
    masks = []
    for case in ["all", "first80", "random60", "shuffled40", "single", "no_adj"]:
        m = np.zeros(small.n, dtype=bool)
        m[ref[f"{case}.super_tiles"][np.asarray(ref[f"{case}.predict"]) > 0]] = True
        assert m.any() and not (m[col[0]] & m[col[1]]).any(), case
        masks.append(m)
    masks += [_independent_set(small, s) for s in (0, 1, 2)]
    got = small.gpu(masks)
    gaps = [abs(g - small.areas[m].sum()) for g, m in zip(got, masks)]
    gates = [small.gate(m) for m in masks]
    big = [_independent_set(ring9, s) for s in (0, 1, 2, 3)]
    assert min(int(m.sum()) for m in big) > 250
    got = ring9.gpu(big)
    gaps += [abs(g - ring9.areas[m].sum()) for g, m in zip(got, big)]
    gates += [ring9.gate(m) for m in big]
    _report("2 collision-free selections", gaps, gates)


# ------------------------------------------------------------------------------------------------ 3. every colliding pair
def test_every_colliding_pair_of_ring9_in_one_call(ring9):
    """area_i + area_j - union = area(T_i n T_j) of tests/region_oracle with T_i as the region, in its rational arithmetic:
    the pairs share sides that lie 1e-8 apart and nearly parallel, where the oracle's fp64 split parameters are ill-conditioned
    (region_oracle.areas_for_region: `exact`) -- its fp64 form misplaces a piece for 4 of the 5 236 pairs (-0.27 .. -0.60)."""
    col = ring9.graph.arrays.colli_edges
    pairs = col[:, col[0] < col[1]].T
    assert pairs.shape == (5236, 2)
    masks = np.zeros((pairs.shape[0], ring9.n), dtype=np.int32)
    masks[np.arange(pairs.shape[0]), pairs[:, 0]] = 1
    masks[np.arange(pairs.shape[0]), pairs[:, 1]] = 1
    got = ring9.gpu(masks)
    overlap = ring9.areas[pairs[:, 0]] + ring9.areas[pairs[:, 1]] - got
    want = np.array([orc.intersection_area_exact(orc.oriented_rings(ring9.rings[i]), ring9.rings[j]) for i, j in pairs])
    assert set(np.round(want, 3).tolist()) == {0.018, 0.036, 0.054}
    _report("3 colliding pairs", np.abs(overlap - want), [uo.gate([ring9.rings[i], ring9.rings[j]], ring9.delta) for i, j in pairs])


# ------------------------------------------------------------------------------------------------ 4. general masks, slab oracle
def _against_oracle(name, fx, masks):
    masks = np.asarray(masks).reshape(-1, fx.n) != 0
    got = fx.gpu(masks)
    _report(name, [abs(g - fx.oracle(m)) for g, m in zip(got, masks)], [max(fx.gate(m), 1e-300) for m in masks])
    return got


@pytest.mark.parametrize("which", ["ring9", "small"])
def test_all_tiles_and_random_subsets_match_the_slab_oracle(which, request):
    fx = request.getfixturevalue(which)
    rng = np.random.default_rng(7 if which == "ring9" else 8)
    masks = [np.ones(fx.n, dtype=bool)]
    for share in np.linspace(0.02, 0.98, 32):                          # 32 per graph: 64 seeded subsets of assorted sizes
        masks.append(rng.random(fx.n) < share)
    got = _against_oracle(f"4 all tiles + 32 random subsets {which}", fx, masks)
    assert got[0] > 0.9 * got.max()


def test_silhouette_crops_match_the_slab_oracle(ring9):
    from tilingnn_amd.tiling import tile_factory as tf
    from tilingnn_amd.util.shape_processor import load_polygons
    for name in ("bunny", "house", "instagram"):
        ext, holes = load_polygons(os.path.join(SIL, f"{name}.txt"))
        regions = tf.crop_variants(ext, holes, ring9.graph, 0.0, 60.0, 3, [0, 0.5], [0.5, 0.05])
        alive = ring9.on_device.tiles_in_regions(regions)
        masks = alive.cpu().numpy()
        filled = masks.any(axis=1)
        assert masks.shape[0] == 24 and (name != "bunny" or filled.sum() >= 12)
        got = ring9.on_device.union_areas(alive).cpu().numpy()          # the int32 masks of tgnn_tiles_in_region as they are
        assert (got[~filled] == 0.0).all()
        _report(f"4 crops {name}", [abs(g - ring9.oracle(m)) for g, m in zip(got[filled], masks[filled])],
                [ring9.gate(m) for m in masks[filled]])


def test_random_star_crops_match_the_slab_oracle(ring9):
    from tilingnn_amd.tiling import tile_factory as tf
    from tilingnn_amd.tiling.region import Region
    rng = random.Random(21)
    bound = tf.get_graph_bound(ring9.graph)
    regions = [Region(tf.draw_random_polygon(bound, rng=rng, max_vertices=10, low=0.2, high=0.9), validate=False) for _ in range(300)]
    alive = ring9.on_device.tiles_in_regions(regions)
    masks = alive.cpu().numpy()
    filled = masks.any(axis=1)
    assert filled.sum() >= 100                                          # at least a third: the test cannot pass by skipping
    got = ring9.on_device.union_areas(alive).cpu().numpy()
    assert (got[~filled] == 0.0).all()
    _report("4 random stars", [abs(g - ring9.oracle(m)) for g, m in zip(got[filled], masks[filled])],
            [ring9.gate(m) for m in masks[filled]])


# ------------------------------------------------------------------------------------------------ 5. synthetic tiles, raw ABI
def _abi(tiles, masks, tol=TOL, pairs=None):
    """tgnn_union_area straight from arrays.  pairs: collision pairs [2, E]; default every pair (a pair that does not collide
    costs time, never area).  Returns (areas, error word)."""
    from tilingnn_amd import _lib
    from tilingnn_amd._lib import check, lib, ptr
    from tilingnn_amd.tiling.region import union_geometry
    n = len(tiles)
    if pairs is None:
        pairs = np.array([(i, j) for i in range(n) for j in range(n) if i != j], dtype=np.int64).reshape(-1, 2).T
    geo = [torch.from_numpy(a if a.size else np.zeros(1, dtype=a.dtype)).to(DEV) for a in union_geometry(tiles, pairs, n)]
    masks = torch.from_numpy(np.ascontiguousarray(np.asarray(masks).reshape(-1, n), dtype=np.int32)).to(DEV)
    k = int(masks.shape[0])
    area = torch.full((k,), np.nan, dtype=torch.float64, device=DEV)
    err = torch.zeros(1, dtype=torch.int32, device=DEV)
    ws_bytes = int(lib.tgnn_union_area_workspace_bytes(k, n))
    ws = torch.empty(max(ws_bytes // 8, 1), dtype=torch.float64, device=DEV)
    check(lib.tgnn_union_area(ptr(geo[0]), ptr(geo[1]), n, ptr(geo[2]), ptr(geo[3]), ptr(masks), k, tol, ptr(area), ptr(err),
                              ptr(ws), ws_bytes, _lib.current_stream(torch.device(DEV))))
    torch.cuda.synchronize()
    return area.cpu().numpy(), int(err.item())


@pytest.mark.parametrize("angle", [0.0, 0.5235987755982988])
def test_abi_synthetic_non_convex_tiles_every_subset(angle):
    """L and U shapes that interlock, a tile strictly inside another, sides shared from the same side with j < i and j > i,
    a tile touching another from outside along a side while overlapping it elsewhere (union_oracle.synthetic_tiles): all 256
    subsets, as given and rotated by 30 degrees.  No noise here (delta = 0): the gate is its rounding term."""
    c, s = np.cos(angle), np.sin(angle)
    tiles = [t @ np.array([[c, s], [-s, c]]) for t in uo.synthetic_tiles()]
    n = len(tiles)
    masks = ((np.arange(2 ** n)[:, None] >> np.arange(n)[None, :]) & 1).astype(np.int32)
    got, err = _abi(tiles, masks)
    assert err == 0 and got[0] == 0.0
    want = np.array([uo.union_area([tiles[i] for i in np.flatnonzero(m)]) for m in masks])
    _report(f"5 synthetic tiles, angle {angle:.2f}", np.abs(got - want)[1:],
            [uo.gate([tiles[i] for i in np.flatnonzero(m)], 0.0) for m in masks[1:]])


# ------------------------------------------------------------------------------------------------ 6. bits, edges of the ABI
def test_two_calls_give_the_same_bits_and_empty_inputs(ring9):
    rng = np.random.default_rng(5)
    masks = (rng.random((512, ring9.n)) < rng.random((512, 1))).astype(np.int32)
    masks[17] = 0
    a, b = ring9.gpu(masks), ring9.gpu(masks)
    assert a.tobytes() == b.tobytes() and a[17] == 0.0 and np.signbit(a[17]) == False     # noqa: E712
    for k in (0, 17, 300, 511):                                         # a row does not depend on its neighbours in the batch
        assert ring9.gpu(masks[k]).tobytes() == a[k:k + 1].tobytes()
    none = ring9.on_device.union_areas(torch.zeros(0, ring9.n, dtype=torch.int32, device=DEV))
    assert none.shape == (0,) and none.dtype == torch.float64
    with pytest.raises(ValueError):
        ring9.on_device.union_areas(torch.zeros(2, ring9.n + 1, dtype=torch.int32, device=DEV))


def test_abi_rejects_bad_arguments():
    from tilingnn_amd._lib import lib
    assert lib.tgnn_union_area(None, None, 4, None, None, None, 2, TOL, None, None, None, 0, None) == -1
    assert b"tgnn_union_area" in lib.tgnn_last_error()
    assert lib.tgnn_union_area(None, None, 4, None, None, None, 0, TOL, None, None, None, 0, None) == 0
    assert lib.tgnn_union_area(None, None, -1, None, None, None, 0, TOL, None, None, None, 0, None) == -1
    one = torch.zeros(64, dtype=torch.float64, device=DEV)
    i32 = torch.zeros(64, dtype=torch.int32, device=DEV)
    p = lambda t: t.data_ptr()
    # a workspace that is too small, a negative tolerance
    assert lib.tgnn_union_area(p(one), p(i32), 4, p(i32), p(i32), p(i32), 2, TOL, p(one), p(i32), p(one), 8, None) == -1
    assert lib.tgnn_union_area(p(one), p(i32), 4, p(i32), p(i32), p(i32), 2, -1.0, p(one), p(i32), p(one), 512, None) == -1
    assert lib.tgnn_union_area_workspace_bytes(2, 4) == 3 * 2 * 4 * 8 and lib.tgnn_union_area_workspace_bytes(0, 4) == 0


def test_interval_overflow_is_an_error_not_a_fault():
    """A star of thin tiles across one side of a big tile: 8 separate covered stretches fit the kernel's list, 10 do not."""
    from tilingnn_amd._lib import TgnnError
    from tilingnn_amd.util.data_util import CompleteGraphOnDevice
    from tilingnn_amd.tiling.region import union_geometry
    big = np.array([[0, 0], [40, 0], [40, 10], [0, 10]], dtype=float)
    thin = [np.array([[3 * k + 1, -1], [3 * k + 1.5, -1], [3 * k + 1.5, 1], [3 * k + 1, 1]], dtype=float) for k in range(10)]
    tiles = [big] + thin
    pairs = np.array([[0] * 10, list(range(1, 11))])
    fits = np.array([1] * 9 + [0, 0], dtype=np.int32)
    got, err = _abi(tiles, [fits], pairs=pairs)
    assert err == 0 and abs(got[0] - (400 + 8 * 0.5)) < 1e-11
    got, err = _abi(tiles, [np.ones(11, dtype=np.int32), fits], pairs=pairs)
    assert err == 2
    # ... which the binding raises on
    od = CompleteGraphOnDevice.__new__(CompleteGraphOnDevice)
    od.device, od.n_tiles = torch.device(DEV), 11
    od._union = tuple(torch.from_numpy(a).to(DEV) for a in union_geometry(tiles, pairs, 11))
    assert abs(float(od.union_areas(torch.from_numpy(fits).to(DEV))[0]) - 404.0) < 1e-11
    with pytest.raises(TgnnError, match="interval"):
        od.union_areas(torch.ones(11, dtype=torch.int32, device=DEV))


# ------------------------------------------------------------------------------------------------ 7. end to end
def test_crop_coverage_and_scores_end_to_end(ring9, tmp_path):
    from tilingnn_amd import TilinGNN
    from tilingnn_amd.solver.ml_solver.losses import Losses, loss_weights
    from tilingnn_amd.solver.ml_solver.ml_solver import ML_Solver
    from tilingnn_amd.tiling import tile_factory as tf
    from tilingnn_amd.util import data_util as du
    from tilingnn_amd.util.shape_processor import load_polygons
    from tilingnn_amd.weights import make_state_dict
    graph = ring9.graph
    ext, holes = load_polygons(os.path.join(SIL, "bunny.txt"))
    crops = tf.crop_multiple_layouts_from_contour(ext, holes, graph, device=DEV, coverage=True, **CROP_KW)
    plain = tf.crop_multiple_layouts_from_contour(ext, holes, graph, device=DEV, **CROP_KW)
    assert 12 <= len(crops) == len(plain) < 24 and all(c is None and l.super_contour_area is None for l, c in plain)
    gaps, gates, oracle_area = [], [], []
    for (layout, coverage), (other, _) in zip(crops, plain):
        assert dict(layout.re_index) == dict(other.re_index)
        mask = np.zeros(ring9.n, dtype=bool)
        mask[list(layout.re_index.keys())] = True
        want, gate = ring9.oracle(mask), ring9.gate(mask)
        region_area = layout.target_polygon.area
        assert isinstance(coverage, float) and 0.0 < coverage <= 1.0 + gate / region_area, coverage
        assert coverage == layout.super_contour_area / region_area
        gaps.append(abs(layout.super_contour_area - want))
        gates.append(gate)
        oracle_area.append(want)
    _report("7 bunny crops, coverage=True", gaps, gates)
    # the DeviceLayout route carries the same areas
    regions = tf.crop_variants(ext, holes, graph, 0.0, 60.0, 3, [0, 0.5], [0.5, 0.05])
    dls = [d for d in ring9.on_device.layouts_in_regions(regions, with_area=True) if d.node_feature.shape[0]]
    assert [d.super_contour_area for d in dls] == [l.super_contour_area for l, _ in crops]
    assert all(d.super_contour_area is None for d in ring9.on_device.layouts_in_regions(regions[:2]))
    # a crop scores with no further step
    net = TilinGNN(adj_edge_features_dim=15, network_depth=20, network_width=32, node_features_dim=3)
    net.load_state_dict(make_state_dict(15, 20, 32, 1, 3, seed=0), strict=True)
    net = net.to(DEV).train()
    idx = int(np.argmax([c[0].node_feature.shape[0] for c in crops]))
    layout = crops[idx][0]
    out, score = ML_Solver(None, torch.device(DEV), graph, net, num_prob_maps=1).solve(layout)
    want = Losses.solution_score(out.predict, layout, super_contour_area=oracle_area[idx], device=torch.device(DEV))
    wa = loss_weights()[2]
    bound = wa * (1 + 1e-7) * gates[idx] / oracle_area[idx] * 1.001 + 1e-15      # d(wa * filled * A0 / A) with filled <= 1 + 1e-7
    print(f"\nunion_area 7 score: {score!r} against {want!r}, gap {abs(score - want):.3e}, bound {bound:.3e}")
    assert isinstance(score, float) and abs(score - want) <= bound
    # a layout file without features, read back: scores after compute_super_contour_area()
    bare = copy.deepcopy(out)
    bare.target_polygon = None                                          # (a Region is not part of the reference's file schema)
    du.write_bricklayout(str(tmp_path), "crop.pkl", bare, with_features=False)
    back = du.load_bricklayout(str(tmp_path / "crop.pkl"), graph)
    assert back.super_contour_area is None
    with pytest.raises(ValueError, match="super contour"):
        Losses.solution_score(back.predict, back, device=torch.device(DEV))
    assert back.compute_super_contour_area(DEV) == layout.super_contour_area == back.super_contour_area
    assert Losses.solution_score(back.predict, back, device=torch.device(DEV)) == score
