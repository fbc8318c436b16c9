"""Times of the tile-in-region predicate (csrc/region.hip) and of Trainer.create_data on the labyrinth complete graph.
Run under `rocprofv3 --kernel-trace --stats` for kernel times; the wall times printed here are host clocks around work that
ends in a device synchronise.  Usage: python scratch/region_times.py OUT_DIR [n_data]"""
import gzip
import os
import random
import shutil
import sys
import tempfile
import time

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from tests.golden_util import GOLDEN  # noqa: E402
from tilingnn_amd.solver.ml_solver.trainer import Trainer  # noqa: E402
from tilingnn_amd.tiling import tile_factory as tf  # noqa: E402
from tilingnn_amd.tiling.region import Region  # noqa: E402
from tilingnn_amd.tiling.tile_graph import TileGraph  # noqa: E402
from tilingnn_amd.util.data_util import graph_on_device  # noqa: E402
from tilingnn_amd.util.shape_processor import load_polygons  # noqa: E402

out_dir = sys.argv[1]
n_data = int(sys.argv[2]) if len(sys.argv) > 2 else 20000
os.makedirs(out_dir, exist_ok=True)
tmp = tempfile.mkdtemp()
path = os.path.join(tmp, "g.pkl")
with gzip.open(os.path.join(GOLDEN, "complete_graph_ring9.pkl.gz"), "rb") as src, open(path, "wb") as dst:
    shutil.copyfileobj(src, dst)
g = TileGraph(2)
g.load_graph_state(path, sidecar=False)
dev = torch.device("cuda:0")
od = graph_on_device(g, dev)
bound = tf.get_graph_bound(g)
rng = random.Random(0)
stars = [Region(tf.draw_random_polygon(bound, 10, 0.4, 0.8, rng), validate=False) for _ in range(4096)]
ext, holes = load_polygons(os.path.join(GOLDEN, "silhouettes", "bunny.txt"))
bunny = tf.crop_variants(ext, holes, g, 0.0, 60.0, 7, [0, 0.25, 0.5], [0.3, 0.5, 0.7])
lines = []


def timed(name, fn, reps=5):
    fn()
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(reps):
        fn()
    torch.cuda.synchronize()
    ms = (time.perf_counter() - t0) / reps * 1e3
    lines.append(f"{name}: {ms:.3f} ms per call (host clock, packing + upload + launch + sync)")


timed("tiles_in_regions 4096 random stars x 1254 tiles", lambda: od.tiles_in_regions(stars))
timed(f"tiles_in_regions {len(bunny)} bunny crop variants x 1254 tiles", lambda: od.tiles_in_regions(bunny))
timed("region_edge_counts 4096 x (10472 + 8502 edges)", lambda: od.region_edge_counts(od.tiles_in_regions(stars)))
work = tempfile.mkdtemp()
trainer = Trainer(None, None, dev, None, os.path.join(work, "data"), model_save_path=os.path.join(work, "model"))
t0 = time.perf_counter()
trainer.create_data(g, number_of_data=n_data, testing_ratio=0.2, rng=random.Random(1))
wall = time.perf_counter() - t0
ct = trainer.create_data_times
lines.append(f"create_data {n_data} + {int(n_data * 0.2)} layouts: {wall:.2f} s wall; draws + predicate + counts {ct['gpu']:.2f} s, "
             f"producer + files {ct['write']:.2f} s")
shutil.rmtree(work)
shutil.rmtree(tmp)
open(os.path.join(out_dir, "region_times.txt"), "w").write("\n".join(lines) + "\n")
print("\n".join(lines))
