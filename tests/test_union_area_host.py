"""Host side of the union-area path: the slab-sweep oracle (tests/union_oracle.py) against closed forms, the packing that
tgnn_union_area takes (tilingnn_amd/tiling/region.py: union_geometry, check_tolerance_gap), and the refusal to run without a
GPU."""
import os

import numpy as np
import pytest

from tests import union_oracle as uo
from tests.golden_util import GOLDEN
from tilingnn_amd.tiling.region import check_tolerance_gap, signed_area, union_geometry, vertex_side_distances

SMALL = os.path.join(GOLDEN, "complete_graph_small.pkl")


def _box(x0, y0, x1, y1):
    return np.array([[x0, y0], [x1, y0], [x1, y1], [x0, y1]], dtype=float)


def _small_graph():
    from tilingnn_amd.tiling.tile_graph import TileGraph
    g = TileGraph(2)
    g.load_graph_state(SMALL, sidecar=False)
    return g


def test_oracle_against_closed_forms():
    assert uo.union_area([]) == 0.0
    assert abs(uo.union_area([_box(0, 0, 2, 2), _box(1, 1, 3, 3)]) - 7.0) < 1e-14            # two offset squares
    assert abs(uo.union_area([_box(0, 0, 2, 2), _box(1, 1, 3, 3)[::-1]]) - 7.0) < 1e-14      # orientation does not matter
    ell = np.array([[1, 1], [4, 1], [4, 2], [2, 2], [2, 4], [1, 4]], dtype=float)
    assert abs(uo.union_area([ell]) - 5.0) < 1e-14
    assert abs(uo.union_area([ell, _box(0, 0, 5, 5)]) - 25.0) < 1e-14                         # an L inside a square
    assert abs(uo.union_area([_box(0, 0, 1, 1), _box(3, 0, 4, 2), _box(0, 5, 0.5, 5.5)]) - 3.25) < 1e-14   # disjoint pieces
    # a ring of six triangles touching along their sides: a regular hexagon of side 1
    ang = np.arange(7) * np.pi / 3
    tris = [np.array([[0, 0], [np.cos(ang[k]), np.sin(ang[k])], [np.cos(ang[k + 1]), np.sin(ang[k + 1])]]) for k in range(6)]
    assert abs(uo.union_area(tris) - 1.5 * np.sqrt(3)) < 1e-14
    assert abs(uo.union_area(tris + tris[:3]) - 1.5 * np.sqrt(3)) < 1e-14                     # duplicates: coincident edges
    # the synthetic tiles of the GPU test
    t = uo.synthetic_tiles()
    area = lambda bits: uo.union_area([t[i] for i in range(8) if (bits >> i) & 1])
    assert abs(area(0b1) - 5.0) < 1e-13 and abs(area(0b10) - 7.5) < 1e-13 and abs(area(0b11) - 10.0) < 1e-13
    assert abs(area(0b100) - 49.0) < 1e-13 and abs(area(0b111) - 49.0) < 1e-13
    assert abs(area(0b111000) - 6.0) < 1e-13 and abs(area(0b11000000) - 7.5) < 1e-13


def test_oracle_sum_of_areas_on_a_collision_free_selection():
    g = _small_graph()
    a = g.arrays
    rings = [t.tile_poly.exterior for t in g.tiles]
    rng = np.random.default_rng(0)
    blocked, pick = np.zeros(a.n_tiles, dtype=bool), []
    for i in rng.permutation(a.n_tiles):
        if not blocked[i]:
            pick.append(int(i))
            blocked[i] = True
            blocked[a.colli_edges[1][a.colli_edges[0] == i]] = True
    assert len(pick) > 20
    want = float(a.tile_areas[pick].sum())
    assert abs(uo.union_area([rings[i] for i in pick]) - want) <= uo.gate([rings[i] for i in pick], 1e-8)


def test_gate_and_noise_width():
    a, b = _box(0, 0, 1, 1), _box(1 + 3e-9, 0, 2, 1)                                          # sides 3e-9 apart
    assert abs(uo.noise_width([a, b], [[0], [1]], 1e-6) - 3e-9) < 1e-15
    assert uo.noise_width([a, _box(1.5, 0, 2, 1)], [[0], [1]], 1e-6) == 0.0
    assert abs(uo.gate([a, b], 1e-8) - (1e-8 * (8 - 3e-9 * 2) + 64 * 2.0 ** -53 * 4 * 8)) < 1e-20
    assert uo.perimeter(np.vstack([a, a[:1]])) == 4.0                                         # closed rings too


def test_union_geometry_orients_rings_and_builds_a_symmetric_csr():
    cw, ccw = _box(0, 0, 1, 1)[::-1], _box(2, 0, 3, 1)
    closed = np.vstack([_box(4, 0, 5, 1), _box(4, 0, 5, 1)[:1]])
    ring_xy, ring_ptr, col_ptr, col_idx = union_geometry([cw, ccw, closed], [[0, 2, 2, 1], [2, 0, 1, 1]])
    assert ring_ptr.tolist() == [0, 4, 8, 12] and ring_xy.dtype == np.float64 and ring_ptr.dtype == np.int32
    for k in range(3):
        assert signed_area(ring_xy[ring_ptr[k]:ring_ptr[k + 1]]) == 1.0
    assert np.array_equal(ring_xy[0:4], cw[::-1]) and np.array_equal(ring_xy[4:8], ccw)
    # one direction given for (2, 1), both for (0, 2), a self loop: rows are symmetric, sorted, without the loop
    assert col_ptr.tolist() == [0, 1, 2, 4] and col_idx.tolist() == [2, 2, 0, 1] and col_idx.dtype == np.int32
    empty = union_geometry([cw], np.zeros((2, 0), dtype=np.int64))
    assert empty[2].tolist() == [0, 0] and empty[3].shape == (0,)
    with pytest.raises(ValueError):
        union_geometry([cw], [[0], [1]])
    with pytest.raises(ValueError):
        union_geometry([cw[:2]], np.zeros((2, 0)))


def test_fixture_graph_packs_and_passes_the_tolerance_check():
    g = _small_graph()
    a = g.arrays
    geo = union_geometry([t.tile_poly.exterior for t in g.tiles], a.colli_edges, a.n_tiles)
    ring_xy, ring_ptr, col_ptr, col_idx = geo
    assert ring_ptr[-1] == sum(t.get_edge_num() for t in g.tiles) and col_ptr[-1] == a.colli_edges.shape[1]
    for i in (0, 7, a.n_tiles - 1):
        assert signed_area(ring_xy[ring_ptr[i]:ring_ptr[i + 1]]) > 0
        assert sorted(col_idx[col_ptr[i]:col_ptr[i + 1]].tolist()) == sorted(a.colli_edges[1][a.colli_edges[0] == i].tolist())
    check_tolerance_gap(*geo)
    d = vertex_side_distances(ring_xy, ring_ptr, a.colli_edges)
    assert d[d < 1e-6].max() < 1e-7 and d[d >= 1e-6].min() > 0.1                              # noise here, geometry there
    # a doctored graph: one vertex moved 2e-5 off the side it lay on
    near = d[d < 1e-6].size
    assert near > 0
    doctored = ring_xy.copy()
    u = int(a.colli_edges[0][0])
    doctored[ring_ptr[u]] += np.array([2e-5, 1.1e-5])
    with pytest.raises(ValueError, match="tolerance"):
        check_tolerance_gap(doctored, ring_ptr, col_ptr, col_idx)


def test_compute_super_contour_area_needs_a_gpu():
    import torch
    from tilingnn_amd.tiling.brick_layout import BrickLayout
    from tilingnn_amd.util import data_util as du
    g = _small_graph()
    layout = BrickLayout(g, *du.create_brick_layout_from_super_set(g, [0, 1, 2, 3]))
    assert layout.super_contour_area is None and not hasattr(layout, "get_super_contour_poly")
    if torch.cuda.is_available():                                       # (run on a GPU box: the method works instead)
        assert layout.compute_super_contour_area() == layout.super_contour_area > 0
        return
    with pytest.raises(RuntimeError, match="GPU"):
        layout.compute_super_contour_area()
    assert layout.super_contour_area is None
