"""The tile-in-region predicate on the GPU (csrc/region.hip: tgnn_tiles_in_region, tgnn_region_edge_counts) against the host
oracle of tests/region_oracle.py, and the crop path and `Trainer.create_data` built on it."""
import gzip
import os
import random
import shutil

import numpy as np
import pytest
import torch

from tests import region_oracle as orc
from tests.golden_util import GOLDEN

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
SIL = os.path.join(GOLDEN, "silhouettes")


@pytest.fixture(scope="module")
def graph(tmp_path_factory):
    from tilingnn_amd.tiling.tile_graph import TileGraph
    path = str(tmp_path_factory.mktemp("labyrinth") / "complete_graph_ring9.pkl")
    with gzip.open(os.path.join(GOLDEN, "complete_graph_ring9.pkl.gz"), "rb") as src, open(path, "wb") as dst:
        shutil.copyfileobj(src, dst)
    g = TileGraph(2)
    g.load_graph_state(path, sidecar=False)
    return g


@pytest.fixture(scope="module")
def on_device(graph):
    from tilingnn_amd.util.data_util import graph_on_device
    return graph_on_device(graph, DEV)


@pytest.fixture(scope="module")
def tile_rings(graph):
    return [t.tile_poly.exterior for t in graph.tiles]


def _oracle(regions, tile_rings, exact=False):
    return np.stack([orc.areas_for_region(orc.oriented_rings(r.exterior, r.interiors), tile_rings, exact) for r in regions])


def _check(regions, on_device, graph, tile_rings, tol=1e-12, exact=False):
    alive, area = on_device.tiles_in_regions(regions, with_area=True)
    alive, area = alive.cpu().numpy(), area.cpu().numpy()
    want = _oracle(regions, tile_rings, exact)
    t_area = graph.arrays.tile_areas
    gap = np.abs(area - want)
    assert gap.max() <= tol, (float(gap.max()), np.unravel_index(np.argmax(gap), gap.shape))
    near = np.abs(t_area[None, :] - want - 1e-6) < 1e-12
    assert not near.any(), np.argwhere(near)                 # no pair sits on the threshold
    assert np.array_equal(alive.astype(bool), orc.contained(want, t_area[None, :]))
    return alive, area


def _stars(graph, seeds, per_seed, **kw):
    from tilingnn_amd.tiling import tile_factory as tf
    from tilingnn_amd.tiling.region import Region
    bound = tf.get_graph_bound(graph)
    out = []
    for s in seeds:
        rng = random.Random(s)
        out += [Region(tf.draw_random_polygon(bound, rng=rng, **kw), validate=False) for _ in range(per_seed)]
    return out


def test_random_stars_match_the_oracle(graph, on_device, tile_rings):
    regions = _stars(graph, [0, 1, 2], 40, max_vertices=10, low=0.4, high=0.8) + \
        _stars(graph, [3, 4], 40, max_vertices=30, low=0.1, high=0.9) + _stars(graph, [5], 40, max_vertices=4, low=0.2, high=0.7)
    alive, _ = _check(regions, on_device, graph, tile_rings)
    assert len(regions) >= 200 and 0 < alive.sum() < alive.size


def test_silhouettes_match_the_oracle_in_one_launch(graph, on_device, tile_rings):
    from tilingnn_amd.tiling import tile_factory as tf
    from tilingnn_amd.util.shape_processor import load_polygons
    regions = []
    for name in ("house", "instagram", "bunny"):
        ext, holes = load_polygons(os.path.join(SIL, f"{name}.txt"))
        regions += tf.crop_variants(ext, holes, graph, 0.0, 50.0, 3, [0, 0.37], [0.35, 0.7])
    assert len(regions) == 72
    alive, _ = _check(regions, on_device, graph, tile_rings)
    assert alive.sum(axis=1).min() > 0


def test_special_regions(graph, on_device, tile_rings):
    from tilingnn_amd.tiling.region import Region
    t_area = graph.arrays.tile_areas
    ring = np.asarray(tile_rings[700])[:-1]
    c = ring.mean(axis=0)
    box = lambda x0, y0, x1, y1: np.array([[x0, y0], [x1, y0], [x1, y1], [x0, y1]], dtype=float)
    # a hole exactly over three tiles (given counter-clockwise: Region orients it)
    hole_tiles = [100, 400, 900]
    holes = [np.asarray(tile_rings[i])[:-1] for i in hole_tiles]
    regions = [Region(ring), Region(c + (ring - c) * (1 - 1e-4)), Region(box(-10, -10, 10, 10)), Region(box(20, 20, 21, 22)),
               Region(box(-10, -10, 10, 10), holes), Region(np.array([[0, 0], [1, 1], [2, 2], [3, 3.0]]), validate=False),
               Region(ring[::-1])]
    alive, area = _check(regions, on_device, graph, tile_rings, exact=True)      # edges on edges: the rational oracle
    assert alive[0, 700] == 1 and abs(area[0, 700] - t_area[700]) < 1e-12 and alive[0].sum() == 1
    assert alive[1].sum() == 0 and 0 < area[1, 700] < t_area[700]
    assert alive[2].all() and not alive[3].any() and not alive[5].any()
    # the complete graph's placements overlap: a hole drops its own tile and the tiles that collide with it, no others
    col = graph.arrays.colli_edges
    near_holes = set(hole_tiles) | set(col[1][np.isin(col[0], hole_tiles)].tolist())
    dropped = set(np.flatnonzero(alive[4] == 0).tolist())
    assert set(hole_tiles) <= dropped <= near_holes and len(dropped) > 3
    assert np.array_equal(alive[6], alive[0]) and np.array_equal(area[6], area[0])    # orientation of the input


def test_k1_and_k4096_and_determinism(graph, on_device, tile_rings):
    regions = _stars(graph, [10, 11, 12, 13], 1024, max_vertices=10, low=0.4, high=0.8)
    alive, area = on_device.tiles_in_regions(regions, with_area=True)
    alive2, area2 = on_device.tiles_in_regions(regions, with_area=True)
    assert torch.equal(alive, alive2) and torch.equal(area, area2)                      # same bits run to run
    alive, area = alive.cpu().numpy(), area.cpu().numpy()
    for k in (0, 1, 1023, 2500, 4095):
        a1, r1 = on_device.tiles_in_regions([regions[k]], with_area=True)
        assert np.array_equal(a1.cpu().numpy()[0], alive[k]) and np.array_equal(r1.cpu().numpy()[0], area[k])
    pick = list(range(0, 4096, 97))
    _check([regions[k] for k in pick], on_device, graph, tile_rings)


def _abi_call(tiles, regions, max_edges=None):
    """tgnn_tiles_in_region straight from arrays: tiles = list of rings, regions = list of Region."""
    from tilingnn_amd import _lib
    from tilingnn_amd._lib import check, lib, ptr
    from tilingnn_amd.tiling.region import pack_regions, tile_geometry, signed_area
    areas = np.array([abs(signed_area(np.asarray(t, dtype=float))) for t in tiles])
    geo = [torch.from_numpy(np.ascontiguousarray(a)).to(DEV) for a in tile_geometry(tiles, areas)]
    ring_xy, ring_ptr, kptr, bbox, me = pack_regions(regions)
    reg = [torch.from_numpy(np.ascontiguousarray(a)).to(DEV) for a in (ring_xy, ring_ptr, kptr, bbox)]
    k, n = len(regions), len(tiles)
    alive = torch.full((k, n), -1, dtype=torch.int32, device=DEV)
    area = torch.full((k, n), np.nan, dtype=torch.float64, device=DEV)
    check(lib.tgnn_tiles_in_region(*(ptr(g) for g in geo), n, *(ptr(r) for r in reg), k, me if max_edges is None else max_edges,
                                   ptr(alive), ptr(area), _lib.current_stream(torch.device(DEV))))
    torch.cuda.synchronize()
    return alive.cpu().numpy(), area.cpu().numpy(), areas


@pytest.mark.parametrize("wide", [False, True])
def test_abi_non_convex_tiles(wide):
    from tilingnn_amd.tiling.region import Region
    ell = np.array([[0, 0], [2, 0], [2, 1], [1, 1], [1, 2], [0, 2]], dtype=float)
    u = np.array([[0, 0], [3, 0], [3, 2], [2, 2], [2, 1], [1, 1], [1, 2], [0, 2]], dtype=float)
    tiles = [ell + (3 * i, 3 * j) for i in range(4) for j in range(4)] + [u + (1, 13), (u + (5, 13))[::-1]]
    rng = np.random.default_rng(3)
    regions = [Region(np.array([[-1, -1], [20, -1], [20, 20], [-1, 20]], dtype=float))]
    for _ in range(40):
        cx, cy = rng.uniform(0, 12, 2)
        n = int(rng.integers(3, 9))
        ang = np.sort(rng.uniform(0, 2 * np.pi, n))
        rad = rng.uniform(1, 6, n)
        regions.append(Region(np.stack([cx + rad * np.cos(ang), cy + rad * np.sin(ang)], axis=1), validate=False))
    regions.append(Region(ell + (3, 3)))                                                # one tile exactly
    alive, area, t_area = _abi_call(tiles, regions, max_edges=64 if wide else None)
    want = np.stack([orc.areas_for_region(orc.oriented_rings(r.exterior, r.interiors), tiles) for r in regions])
    assert np.abs(area - want).max() <= 1e-12
    assert np.array_equal(alive.astype(bool), orc.contained(want, t_area[None, :]))
    assert alive[0].all() and alive[-1].sum() == 1 and alive[-1][5] == 1
    alive2, area2, _ = _abi_call(tiles, regions, max_edges=64 if wide else None)
    assert np.array_equal(alive, alive2) and area.tobytes() == area2.tobytes()


def test_abi_rejects_bad_arguments():
    from tilingnn_amd._lib import lib
    assert lib.tgnn_tiles_in_region(None, None, None, None, None, 4, None, None, None, None, 2, 8, None, None, None) == -1
    assert lib.tgnn_tiles_in_region(None, None, None, None, None, 0, None, None, None, None, 0, 8, None, None, None) == 0
    assert lib.tgnn_region_edge_counts(None, 2, 4, None, 0, None, 0, None, None, None) == -1


def test_region_edge_counts(graph, on_device):
    regions = _stars(graph, [21], 300, max_vertices=10, low=0.2, high=0.9)
    alive = on_device.tiles_in_regions(regions)
    counts = on_device.region_edge_counts(alive).cpu().numpy()
    al = alive.cpu().numpy().astype(bool)
    a = graph.arrays
    want_c = (al[:, a.colli_edges[0]] & al[:, a.colli_edges[1]]).sum(axis=1)
    want_a = (al[:, a.adj_edges[0]] & al[:, a.adj_edges[1]]).sum(axis=1)
    assert np.array_equal(counts[:, 0], want_c) and np.array_equal(counts[:, 1], want_a)
    assert (counts == 0).any() and (counts > 0).any()


def _same_layout(a, b):
    for x, y in zip(a, b):
        if isinstance(x, dict):
            assert dict(x) == dict(y)
        else:
            assert np.asarray(x).dtype == np.asarray(y).dtype and np.array_equal(x, y)


def test_crop_bunny_layouts(graph, on_device, tile_rings):
    from tilingnn_amd.tiling import tile_factory as tf
    from tilingnn_amd.util import data_util as du
    from tilingnn_amd.util.shape_processor import load_polygons
    ext, holes = load_polygons(os.path.join(SIL, "bunny.txt"))
    kw = dict(start_angle=0.0, end_angle=60.0, num_of_angle=3, movement_delta_ratio=[0, 0.5], margin_padding_ratios=[0.5, 0.05])
    crops = tf.crop_multiple_layouts_from_contour(ext, holes, graph, device=DEV, **kw)
    regions = tf.crop_variants(ext, holes, graph, 0.0, 60.0, 3, [0, 0.5], [0.5, 0.05])
    want = _oracle(regions, tile_rings)
    sets = [np.flatnonzero(orc.contained(w, graph.arrays.tile_areas)).tolist() for w in want]
    sets = [s for s in sets if s]
    assert len(crops) == len(sets) and 12 <= len(crops) < 24                           # the smallest margin leaves some empty
    for (layout, coverage), tiles in zip(crops, sets):
        assert coverage is None and layout.predict_probs == [0.5] * len(tiles)
        ref = du.create_brick_layout_from_super_set(graph, tiles)
        _same_layout((layout.node_feature, layout.collide_edge_index, layout.collide_edge_features, layout.align_edge_index,
                      layout.align_edge_features, layout.re_index), ref)
    # the DeviceLayout route equals the host route
    big = [r for r, w in zip(regions, want) if orc.contained(w, graph.arrays.tile_areas).any()]
    dls = on_device.layouts_in_regions(big)
    for dl, (layout, _) in zip(dls, crops):
        assert torch.equal(dl.node_feature.cpu(), torch.from_numpy(layout.node_feature).float())
        assert torch.equal(dl.align_edge_index.cpu(), torch.from_numpy(np.asarray(layout.align_edge_index)).long().reshape(2, -1))
        assert torch.equal(dl.collide_edge_index.cpu(), torch.from_numpy(np.asarray(layout.collide_edge_index)).long().reshape(2, -1))
        assert torch.equal(dl.align_edge_features.cpu(),
                           torch.from_numpy(np.asarray(layout.align_edge_features)).float().reshape(dl.align_edge_features.shape))
        assert dl.inverse_index.cpu().tolist() == sorted(layout.re_index.keys())
    # one crop through ML_Solver.solve (synthetic weights)
    from tilingnn_amd import TilinGNN
    from tilingnn_amd.solver.ml_solver.ml_solver import ML_Solver
    from tilingnn_amd.weights import make_state_dict
    net = TilinGNN(adj_edge_features_dim=15, network_depth=20, network_width=32, node_features_dim=3)
    net.load_state_dict(make_state_dict(15, 20, 32, 1, 3, seed=0), strict=True)
    net = net.to(DEV).train()
    idx = int(np.argmax([c[0].node_feature.shape[0] for c in crops]))
    layout = crops[idx][0]
    out, score = ML_Solver(None, torch.device(DEV), graph, net, num_prob_maps=1).solve(layout)
    sel = np.flatnonzero(np.asarray(out.predict) > 0)
    col = np.asarray(layout.collide_edge_index).reshape(2, -1)
    chosen = np.zeros(layout.node_feature.shape[0], dtype=bool)
    chosen[sel] = True
    assert score is None and sel.size > 0 and not (chosen[col[0]] & chosen[col[1]]).any()
    inv = {v: k for k, v in layout.re_index.items()}
    inside = orc.contained([w for w in want if orc.contained(w, graph.arrays.tile_areas).any()][idx], graph.arrays.tile_areas)
    assert all(inside[inv[int(i)]] for i in sel)


def _host_create_data(graph, tile_rings, n_train, n_test, seed, low=0.4, high=0.8, max_vertices=10):
    """The reference's sequential loop with the oracle predicate: (list of tile sets per split, final rng state)."""
    from tilingnn_amd.tiling import tile_factory as tf
    rng = random.Random(seed)
    bound = tf.get_graph_bound(graph)
    a = graph.arrays
    out = []
    for n in (n_train, n_test):
        sets = []
        while len(sets) < n:
            v = np.array(tf.draw_random_polygon(bound, max_vertices, low, high, rng))
            inside = orc.contained(orc.areas_for_region(orc.oriented_rings(v), tile_rings), a.tile_areas)
            m = inside
            if (m[a.colli_edges[0]] & m[a.colli_edges[1]]).any() and (m[a.adj_edges[0]] & m[a.adj_edges[1]]).any():
                sets.append(np.flatnonzero(inside).tolist())
        out.append(sets)
    return out, rng.getstate()


def test_create_data_matches_the_sequential_loop_and_trains(graph, tile_rings, tmp_path):
    from tilingnn_amd import TilinGNN
    from tilingnn_amd.solver.ml_solver.ml_solver import ML_Solver
    from tilingnn_amd.solver.ml_solver.trainer import Trainer
    from tilingnn_amd.util import data_util as du
    from tilingnn_amd.weights import make_state_dict
    net = TilinGNN(adj_edge_features_dim=15, network_depth=4, network_width=32, node_features_dim=3)
    net.load_state_dict(make_state_dict(15, 4, 32, 1, 3, seed=1), strict=True)
    net = net.to(DEV).train()
    trainer = Trainer(None, None, torch.device(DEV), net, str(tmp_path / "data"), model_save_path=str(tmp_path / "model"))
    rng = random.Random(2024)
    trainer.create_data(graph, number_of_data=32, testing_ratio=0.25, rng=rng, batch=16)
    (train_sets, test_sets), state = _host_create_data(graph, tile_rings, 32, 8, 2024)
    assert rng.getstate() == state
    for split, sets in (("train", train_sets), ("test", test_sets)):
        raw = tmp_path / "data" / split / "raw"
        assert sorted(os.listdir(raw)) == sorted(f"data_{i}.pkl" for i in range(len(sets)))
        for i, tiles in enumerate(sets):
            got = (raw / f"data_{i}.pkl").read_bytes()
            du.write_brick_layout_data(f"want_{split}_{i}.pkl", *_write_args(du.create_brick_layout_from_super_set(graph, tiles)),
                                       prefix=str(tmp_path))
            assert got == (tmp_path / f"want_{split}_{i}.pkl").read_bytes(), (split, i)
            re_index, x, col, colf, adj, adjf, *_ = du.load_brick_layout_data(str(raw / f"data_{i}.pkl"))
            assert len(col) > 0 and len(adj) > 0
    opt = torch.optim.Adam(net.parameters(), lr=1e-3)
    history = trainer.train(ML_Solver(None, torch.device(DEV), graph, net, num_prob_maps=1), opt, batch_size=1,
                            training_epoch=2, save_model_per_epoch=1, shuffle_seed=0, log=lambda *_: None)
    assert len(history) == 2 and all(np.isfinite(h).all() for h in history)


def _write_args(out):
    node_feature, col, colf, adj, adjf, re_index = out
    return re_index, node_feature, col, colf, adj, adjf
