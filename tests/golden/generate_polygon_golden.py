"""Golden vectors for the random target shapes of the crop path, produced by the REFERENCE itself.

Run in the build container only (needs the reference tree):   python tests/golden/generate_polygon_golden.py

Imported UNCHANGED: the reference's `tiling/tile_factory.py` (generatePolygon, generate_random_inputs, clip,
get_graph_bound), under the import-time stubs of generate_greedy_golden.import_reference (shapely and friends become
attribute-absorbing dummies).  Only the polygon DRAW is recorded, not the shapely crop: the module's `Polygon` is replaced
by a recorder and `create_brick_layout_from_polygon` by a stand-in that ends the attempt loop at once.  The graph handed in
carries the labyrinth graph's tile rings, so the draw is centred and sized as for the real graph.

Stored (ref_random_polygons.npz), for several seeds of the global `random` stream:
  * gp.<i>.*      generatePolygon(ctr, radius, irregularity, spikeyness, n) -- the vertices and random.getstate() after;
  * gri.<i>.*     generate_random_inputs(graph, max_vertices, low, high), drawn three times in a row -- the vertices of each
                  draw and the state after each.
The graph's bound (get_graph_bound) is stored as `bound`.  A state is the 625 words of the Mersenne Twister (int64) and gauss_next (NaN for None).
"""
import os
import random
import sys
import types

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.dont_write_bytecode = True
sys.path.insert(0, HERE)
sys.path.insert(1, os.path.dirname(os.path.dirname(HERE)))
import generate_greedy_golden as ggg                            # noqa: E402

GP_CASES = [  # seed, ctrX, ctrY, aveRadius, irregularity, spikeyness, numVerts
    (0, 0.0, 0.0, 1.0, 0.3, 0.2, 8), (1, 2.5, -1.0, 3.0, 0.9, 0.7, 3), (2, 0.1, 0.2, 0.5, 1.5, -0.3, 12),
    (3, -4.0, 7.0, 10.0, 0.0, 1.0, 25), (4, 0.0, 0.0, 2.0, 0.5, 0.5, 5)]
GRI_CASES = [  # seed, max_vertices, low, high
    (0, 10, 0.4, 0.8), (1, 10, 0.2, 0.7), (7, 4, 0.4, 0.8), (11, 20, 0.1, 0.9), (12345, 10, 0.4, 0.8)]


def state_arrays(state):
    version, words, gauss_next = state
    assert version == 3
    return np.array(words, dtype=np.int64), np.float64(np.nan if gauss_next is None else gauss_next)


def main():
    ggg.import_reference()
    import tiling.tile_factory as tf
    from tilingnn_amd.tiling.tile_graph import TileGraph
    import gzip
    import shutil
    import tempfile
    with tempfile.TemporaryDirectory() as tmp:
        path = os.path.join(tmp, "g.pkl")
        with gzip.open(os.path.join(HERE, "complete_graph_ring9.pkl.gz"), "rb") as src, open(path, "wb") as dst:
            shutil.copyfileobj(src, dst)
        g = TileGraph(2)
        g.load_graph_state(path, sidecar=False)
        rings = [np.array(t.tile_poly.exterior) for t in g.tiles]
    graph = types.SimpleNamespace(tiles=[types.SimpleNamespace(tile_poly=types.SimpleNamespace(
        exterior=types.SimpleNamespace(coords=r))) for r in rings])

    drawn = []
    tf.Polygon = lambda vertices, *a, **k: drawn.append(np.array(vertices, dtype=np.float64)) or vertices
    tf.create_brick_layout_from_polygon = lambda graph, polygon: (np.zeros((1, 1)), [1], None, [1], None, {})

    out = {}
    for i, (seed, cx, cy, r, irr, spk, n) in enumerate(GP_CASES):
        random.seed(seed)
        v = np.array(tf.generatePolygon(cx, cy, r, irr, spk, n), dtype=np.float64)
        out[f"gp.{i}.args"] = np.array([seed, cx, cy, r, irr, spk, n], dtype=np.float64)
        out[f"gp.{i}.vertices"] = v
        out[f"gp.{i}.state"], out[f"gp.{i}.gauss_next"] = state_arrays(random.getstate())
    for i, (seed, mv, low, high) in enumerate(GRI_CASES):
        random.seed(seed)
        out[f"gri.{i}.args"] = np.array([seed, mv, low, high], dtype=np.float64)
        for d in range(3):
            drawn.clear()
            tf.generate_random_inputs(graph, mv, low=low, high=high)
            assert len(drawn) == 1
            out[f"gri.{i}.{d}.vertices"] = drawn[0]
            out[f"gri.{i}.{d}.state"], out[f"gri.{i}.{d}.gauss_next"] = state_arrays(random.getstate())
    out["bound"] = np.array(tf.get_graph_bound(graph), dtype=np.float64)
    out["n_gp"], out["n_gri"], out["n_draws"] = np.int64(len(GP_CASES)), np.int64(len(GRI_CASES)), np.int64(3)
    np.savez_compressed(os.path.join(HERE, "ref_random_polygons.npz"), **out)
    print(f"wrote ref_random_polygons.npz ({len(out)} arrays)")


if __name__ == "__main__":
    main()
