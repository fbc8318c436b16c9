"""Input producer and on-disk formats: host side, no GPU.

Expected values come from the REFERENCE's own code (tests/golden/generate_layout_golden.py): its loader, its
producer, its writer.  Everything here is exact: same values, same dtypes, same shapes.
"""
import gzip
import os
import pickle
import pickletools
import shutil
from collections import defaultdict

import numpy as np
import pytest

from tests.golden_util import GOLDEN, load_labyrinth_graph, load_npz
from tilingnn_amd.tiling import tile_graph as tg
from tilingnn_amd.tiling.brick_layout import BrickLayout
from tilingnn_amd.tiling.tile_graph import TileGraph
from tilingnn_amd.util import data_util as du

SMALL = os.path.join(GOLDEN, "complete_graph_small.pkl")
FULL = os.path.join(GOLDEN, "complete_graph_ring9.pkl.gz")      # data/labyrinth/complete_graph_ring9.pkl of the reference, gzipped
KEYS = ("x", "col", "col_attr", "adj", "adj_attr")


def _small(sidecar=False):
    g = TileGraph(2)
    g.load_graph_state(SMALL, sidecar=sidecar)
    return g


def _re_index(tiles):
    r = defaultdict(int)
    for i, t in enumerate(tiles):
        r[t] = i
    return r


def _same(got, want, what):
    got, want = np.asarray(got), np.asarray(want)
    assert got.shape == want.shape and got.dtype == want.dtype, (what, got.shape, want.shape, got.dtype, want.dtype)
    assert np.array_equal(got, want), what


def test_complete_graph_loads_without_shapely():
    g = _small()
    ref = load_npz("ref_layouts.npz")
    assert len(g.tiles) == 150 and g.total_feature_dim == 15 and g.align_start_index == 2
    assert g.max_area == float(ref["max_area"]) and g.max_align_length == float(ref["max_align_length"])
    a = g.arrays
    _same(a.tile_areas, ref["tile_areas"][:150], "areas")          # GEOS operation order: bit-equal to shapely's
    _same(a.tile_ids, ref["tile_ids"][:150], "ids")
    assert max(ref["tile_areas"]) == float(ref["max_area"])         # the number the real shapely stored in the file
    # list / dict views carry what the arrays carry
    assert a.adj_edges.shape == (2, len(g.adj_edges)) and a.colli_edges.shape == (2, len(g.colli_edges))
    u, v = g.adj_edges[7]
    assert np.array_equal(a.adj_features[7], np.asarray(g.edges_features[u][v], dtype=np.float64))
    assert a.adj_type[7] == int(np.argmax(g.edges_features[u][v][2:]))
    assert sorted(g.graph[0]) == sorted({v for (u, v) in g.adj_edges + g.colli_edges if u == 0})
    assert g._get_graph_statistics() == (150, len(g.adj_edges) // 2, len(g.colli_edges) // 2)


def test_edge_type_ids_from_the_one_hot_columns_identify_the_fp32_rows():
    """The device path dedups adjacency feature rows exactly; the one-hot class must induce the same partition once
    the rows are in fp32 (in float64 the align-length column carries ~1e-12 noise)."""
    a = _small().arrays
    rows32 = a.adj_features_normalised().astype(np.float32)
    _, inv = np.unique(rows32, axis=0, return_inverse=True)
    pairs = set(zip(a.adj_type.tolist(), inv.reshape(-1).tolist()))
    assert len(pairs) == len(set(a.adj_type.tolist())) == len(set(inv.reshape(-1).tolist()))


@pytest.mark.parametrize("payload", [
    b"cos\nsystem\n(S'echo pwned'\ntR.",
    pickle.dumps({"tiles": [pickle.Pickler]}, protocol=3),
])
def test_loader_refuses_globals_outside_the_schema(tmp_path, payload):
    p = tmp_path / "evil.pkl"
    p.write_bytes(payload)
    with pytest.raises(pickle.UnpicklingError):
        TileGraph(2).load_graph_state(str(p), sidecar=False)
    with pytest.raises(pickle.UnpicklingError):
        du.load_brick_layout_data(str(p))


def test_graph_construction_is_refused_loudly():
    with pytest.raises(NotImplementedError):
        TileGraph(2, tiles=[object()])


@pytest.mark.parametrize("case", ["small.first80", "small.random60", "small.all", "small.isolated", "small.shuffled40"])
def test_producer_matches_reference(case):
    g, ref = _small(), load_npz("ref_layouts.npz")
    tiles = ref[f"{case}.super_tiles"].tolist()
    out = du.recover_features_from_reindex(_re_index(tiles), g)
    for key, arr in zip(KEYS, out):
        _same(arr, ref[f"{case}.{key}"], (case, key))
    out6 = du.create_brick_layout_from_super_set(g, tiles)
    for key, arr in zip(KEYS, out6[:5]):
        _same(arr, ref[f"{case}.{key}"], (case, key))
    assert dict(out6[5]) == {t: i for i, t in enumerate(tiles)} and out6[5][10 ** 6] == 0     # defaultdict(int)


def test_generate_brick_layout_data_with_edge_lists():
    g, ref = _small(), load_npz("ref_layouts.npz")
    ce = [tuple(e) for e in ref["small.direct.col_edges"].tolist()]
    ae = [tuple(e) for e in ref["small.direct.adj_edges"].tolist()]
    out = du.generate_brick_layout_data(g, list(range(80)), ce, ae)
    for key, arr in zip(KEYS, out[:5]):
        _same(arr, ref[f"small.direct.{key}"], key)
    with pytest.raises(KeyError):
        du.generate_brick_layout_data(g, list(range(80)), [(0, 1)], [(0, 0)])      # (0, 0) is not an edge of the graph


@pytest.fixture(scope="module")
def full_pickle(tmp_path_factory):
    path = str(tmp_path_factory.mktemp("labyrinth") / "complete_graph_ring9.pkl")
    with gzip.open(FULL, "rb") as src, open(path, "wb") as dst:
        shutil.copyfileobj(src, dst)
    return path


@pytest.mark.parametrize("case", ["first200", "random400", "all", "isolated", "shuffled60"])
def test_producer_matches_reference_on_the_full_graph(case, full_pickle):
    g = TileGraph(2)
    g.load_graph_state(full_pickle, sidecar=False)
    ref = load_npz("ref_layouts.npz")
    assert len(g.tiles) == int(ref["n_tiles"]) and len(g.adj_edges) == int(ref["n_adj_edges"])
    _same(g.arrays.tile_areas, ref["tile_areas"], "areas")
    assert g.arrays.tile_areas.max() == g.max_area
    out = du.recover_features_from_reindex(_re_index(ref[f"{case}.super_tiles"].tolist()), g)
    for key, arr in zip(KEYS, out):
        _same(arr, ref[f"{case}.{key}"], (case, key))


def test_sidecar_replaces_the_pickle(tmp_path, monkeypatch):
    p = str(tmp_path / "cg.pkl")
    shutil.copy(SMALL, p)
    first = TileGraph(2)
    first.load_graph_state(p)                                      # parses the pickle, writes the side-car
    assert os.path.exists(p + tg.SIDECAR_SUFFIX)
    monkeypatch.setattr(tg, "load_schema_pickle", lambda path: (_ for _ in ()).throw(AssertionError("pickle touched")))
    second = TileGraph(2)
    second.load_graph_state(p)
    for name in ("tile_ids", "tile_areas", "colli_edges", "adj_edges", "colli_features", "adj_features", "adj_type"):
        _same(getattr(second.arrays, name), getattr(first.arrays, name), name)
    assert second.adj_edges == first.adj_edges and second.colli_edges == first.colli_edges
    assert second.max_area == first.max_area and second.max_align_length == first.max_align_length
    assert {u: dict(r) for u, r in second.edges_features.items()} == \
        {u: {v: [float(x) for x in f] for v, f in r.items()} for u, r in first.edges_features.items()}
    assert {u: sorted(v) for u, v in second.graph.items()} == {u: sorted(v) for u, v in first.graph.items() if v}
    assert np.array_equal(second.tiles[3].tile_poly.exterior, first.tiles[3].tile_poly.exterior)
    tiles = list(range(0, 150, 2))
    for a, b in zip(du.recover_features_from_reindex(_re_index(tiles), second),
                    du.recover_features_from_reindex(_re_index(tiles), first)):
        _same(a, b, "producer from side-car")
    monkeypatch.undo()
    os.utime(p, ns=(1, 1))                                         # the pickle changed: the side-car is stale
    third = TileGraph(2)
    assert not third._load_sidecar(p + tg.SIDECAR_SUFFIX, p)


def _globals_of(path):
    out, strs = set(), []
    for op, arg, _ in pickletools.genops(open(path, "rb").read()):
        if op.name == "GLOBAL":
            out.add(arg)
        elif op.name in ("SHORT_BINUNICODE", "BINUNICODE"):
            strs.append(arg)
        elif op.name == "STACK_GLOBAL":
            out.add(" ".join(strs[-2:]))
    return out


def test_complete_graph_round_trip_names_the_reference_classes(tmp_path):
    g = _small()
    p = str(tmp_path / "again.pkl")
    g.save_current_state(p)
    assert {"tiling.tile Tile", "shapely.geometry.polygon Polygon"} <= _globals_of(p)
    assert _globals_of(p) <= _globals_of(SMALL) | {"numpy.core.multiarray scalar", "numpy._core.multiarray scalar"}
    import sys
    assert "tiling.tile" not in sys.modules                          # the temporary names are gone again
    h = TileGraph(2)
    h.load_graph_state(p, sidecar=False)
    for name in ("tile_ids", "tile_areas", "colli_edges", "adj_edges", "colli_features", "adj_features"):
        _same(getattr(h.arrays, name), getattr(g.arrays, name), name)
    assert h.tiles[5].tile_poly.wkb == g.tiles[5].tile_poly.wkb


def test_brick_layout_files_written_by_the_reference():
    ref = load_npz("ref_layouts.npz")
    got = du.load_brick_layout_data(os.path.join(GOLDEN, "layout_with_features.pkl"))
    assert dict(got[0]) == {i: i for i in range(200)}
    for key, arr in zip(KEYS, got[1:6]):
        _same(arr, ref[f"first200.{key}"], key)
    _same(got[6], np.arange(200) % 2, "predict")
    assert got[7] == [3, 1, 2] and got[8] is None and got[9] == [0.5, 0.25]
    bare = du.load_brick_layout_data(os.path.join(GOLDEN, "layout_reindex_only.pkl"))
    assert dict(bare[0]) == {i: i for i in range(200)} and all(v is None for v in bare[1:])


def test_load_bricklayout_recovers_features_from_the_reindex():
    g = _small()
    ref = load_npz("ref_layouts.npz")
    tiles = ref["small.random60.super_tiles"].tolist()
    d = os.path.join(os.environ.get("TMPDIR", "/tmp"), f"tgnn_layout_{os.getpid()}")
    try:
        du.write_brick_layout_data("bare.pkl", _re_index(tiles), prefix=d)
        layout = du.load_bricklayout(os.path.join(d, "bare.pkl"), g)
        for key, name in zip(KEYS, ("node_feature", "collide_edge_index", "collide_edge_features", "align_edge_index",
                                    "align_edge_features")):
            _same(getattr(layout, name), ref[f"small.random60.{key}"], key)
        assert layout.inverse_index[3] == tiles[3] and layout.predict.shape == (60,)
        layout.predict = np.ones(60)
        layout.predict_order = [1, 2]
        du.write_bricklayout(d, "full.pkl", layout)
        assert _globals_of(os.path.join(d, "full.pkl")) <= _globals_of(os.path.join(GOLDEN, "layout_with_features.pkl")) | \
            {"numpy.core.multiarray _reconstruct", "numpy._core.multiarray _reconstruct"}
        again = du.load_bricklayout(os.path.join(d, "full.pkl"), complete_graph=None)      # features travel in the file
        BrickLayout.assert_equal_layout(layout, again)
        assert again.predict_order == [1, 2] and np.array_equal(again.predict, np.ones(60))
    finally:
        shutil.rmtree(d, ignore_errors=True)


class _Selection:
    def __init__(self, n, labelled):
        self.labelled_nodes = {int(v): 1 for v in labelled}
        self.unlabelled_nodes = {i: 1.0 for i in reversed(range(n)) if i not in self.labelled_nodes}   # unsorted on purpose


@pytest.mark.parametrize("k", [0, 1, 2])
def test_compute_sub_layout_matches_reference(k):
    ref, g = load_npz("ref_greedy.npz"), load_labyrinth_graph()
    n = g["x"].shape[0]
    f64 = lambda a: np.asarray(a, dtype=np.float64)
    layout = BrickLayout(None, f64(g["x"]), g["col"], f64(g["col_attr"]), g["adj"], f64(g["adj_attr"]), {i: i for i in range(n)})
    sel = _Selection(n, ref[f"sub{k}.labelled"])
    sub, inverse = layout.compute_sub_layout(sel)
    assert list(sel.unlabelled_nodes) == sorted(sel.unlabelled_nodes)                        # brick_layout.py:250-252
    _same(sub.node_feature, ref[f"sub{k}.x"], "x")
    _same(sub.align_edge_index, ref[f"sub{k}.adj"], "adj")
    _same(sub.align_edge_features, ref[f"sub{k}.adj_attr"], "adj_attr")
    _same(sub.collide_edge_index, ref[f"sub{k}.col"], "col")
    _same(sub.collide_edge_features, ref[f"sub{k}.col_attr"], "col_attr")
    _same(np.array([inverse[i] for i in range(len(inverse))]), ref[f"sub{k}.inverse"], "inverse")
    assert sub.re_index == {int(v): i for i, v in enumerate(ref[f"sub{k}.inverse"])}


def test_compute_sub_layout_without_surviving_edges():
    x = np.eye(3)
    layout = BrickLayout(None, x, np.array([[0, 1], [1, 0]]), np.ones((2, 4)), np.array([[1, 2], [2, 1]]), np.ones((2, 4)),
                         {i: i for i in range(3)})
    sel = _Selection(3, [1])
    sub, _ = layout.compute_sub_layout(sel)
    for arr in (sub.collide_edge_index, sub.collide_edge_features, sub.align_edge_index, sub.align_edge_features):
        assert arr.shape == (0,)                                   # np.array([]) as in the reference
