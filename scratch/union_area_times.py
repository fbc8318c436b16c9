"""Times of the union-area kernels (csrc/union_area.hip) on the labyrinth complete graph, beside the tile-in-region predicate
on the same masks.  Device events around the library call (its two kernels; the read-back of the error word is outside the
events); run under `rocprofv3 --kernel-trace --stats` for the per-kernel split.
Usage: python scratch/union_area_times.py OUT_DIR"""
import gzip
import os
import random
import shutil
import sys
import tempfile

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from tests.golden_util import GOLDEN  # noqa: E402
from tilingnn_amd import _lib  # noqa: E402
from tilingnn_amd._lib import check, lib, ptr  # noqa: E402
from tilingnn_amd.tiling import tile_factory as tf  # noqa: E402
from tilingnn_amd.tiling.region import UNION_TOL, Region  # noqa: E402
from tilingnn_amd.tiling.tile_graph import TileGraph  # noqa: E402
from tilingnn_amd.util.data_util import graph_on_device  # noqa: E402
from tilingnn_amd.util.shape_processor import load_polygons  # noqa: E402

out_dir = sys.argv[1]
os.makedirs(out_dir, exist_ok=True)
tmp = tempfile.mkdtemp()
path = os.path.join(tmp, "g.pkl")
with gzip.open(os.path.join(GOLDEN, "complete_graph_ring9.pkl.gz"), "rb") as src, open(path, "wb") as dst:
    shutil.copyfileobj(src, dst)
g = TileGraph(2)
g.load_graph_state(path, sidecar=False)
dev = torch.device("cuda:0")
od = graph_on_device(g, dev)
n = od.n_tiles
bound = tf.get_graph_bound(g)
rng = random.Random(0)
stars = [Region(tf.draw_random_polygon(bound, 10, 0.4, 0.8, rng), validate=False) for _ in range(4096)]
ext, holes = load_polygons(os.path.join(GOLDEN, "silhouettes", "bunny.txt"))
bunny = tf.crop_variants(ext, holes, g, 0.0, 60.0, 7, [0, 0.25, 0.5], [0.3, 0.5, 0.7])
col = g.arrays.colli_edges
pairs = col[:, col[0] < col[1]].T
pair_masks = np.zeros((pairs.shape[0], n), dtype=np.int32)
pair_masks[np.arange(pairs.shape[0]), pairs[:, 0]] = 1
pair_masks[np.arange(pairs.shape[0]), pairs[:, 1]] = 1
geo = od._union_geometry()
lines = []


def timed(name, alive, reps=20):
    k = int(alive.shape[0])
    area = torch.empty(k, dtype=torch.float64, device=dev)
    err = torch.zeros(1, dtype=torch.int32, device=dev)
    ws_bytes = int(lib.tgnn_union_area_workspace_bytes(k, n))
    ws = torch.empty(ws_bytes // 8, dtype=torch.float64, device=dev)
    call = lambda: check(lib.tgnn_union_area(ptr(geo[0]), ptr(geo[1]), n, ptr(geo[2]), ptr(geo[3]), ptr(alive), k, UNION_TOL,
                                             ptr(area), ptr(err), ptr(ws), ws_bytes, _lib.current_stream(dev)))
    for _ in range(3):
        call()
    torch.cuda.synchronize()
    t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    t0.record()
    for _ in range(reps):
        call()
    t1.record()
    torch.cuda.synchronize()
    assert int(err.item()) == 0
    share = float((alive != 0).float().mean())
    lines.append(f"tgnn_union_area {name}: {t0.elapsed_time(t1) / reps:.3f} ms per call (device events, {reps} calls back to back; "
                 f"{share:.1%} of the {k} x {n} tiles alive; areas {float(area.min()):.3f} .. {float(area.max()):.3f})")


alive_stars = od.tiles_in_regions(stars)
alive_bunny = od.tiles_in_regions(bunny)
timed("4 096 random-star masks x 1 254 tiles", alive_stars)
timed(f"{len(bunny)} bunny crop variants x 1 254 tiles", alive_bunny)
timed(f"{pairs.shape[0]} colliding-pair masks x 1 254 tiles", torch.from_numpy(pair_masks).to(dev))
timed("4 096 full masks x 1 254 tiles (every tile alive)", torch.ones(4096, n, dtype=torch.int32, device=dev))
shutil.rmtree(tmp)
open(os.path.join(out_dir, "union_area_times.txt"), "w").write("\n".join(lines) + "\n")
print("\n".join(lines))
