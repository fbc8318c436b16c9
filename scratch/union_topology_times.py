"""Times of the union-topology call (csrc/union_topology.hip) beside the union-area call (csrc/union_area.hip) on the same masks
of the labyrinth complete graph, and the host cost of the contact relation.  Host clock around a synchronise, one call per
measurement, the two calls interleaved (A B A B ...), median and spread of the repeats.  The read-back of the error word is
outside the clock.  Also runs the README's silhouette -> crops -> solve_many -> detect_holes_many flow once, on the bunny.
Usage: python scratch/union_topology_times.py OUT_DIR"""
import gzip
import os
import shutil
import sys
import tempfile
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from tests import topology_oracle as to  # noqa: E402
from tests.golden_util import GOLDEN  # noqa: E402
from tilingnn_amd import TilinGNN, _lib  # noqa: E402
from tilingnn_amd._lib import check, lib, ptr  # noqa: E402
from tilingnn_amd.solver.ml_solver.ml_solver import ML_Solver  # noqa: E402
from tilingnn_amd.tiling import tile_factory as tf  # noqa: E402
from tilingnn_amd.tiling.brick_layout import detect_holes_many  # noqa: E402
from tilingnn_amd.tiling.region import UNION_TOL, contact_geometry, sweep_direction, union_geometry  # noqa: E402
from tilingnn_amd.tiling.tile_graph import TileGraph  # noqa: E402
from tilingnn_amd.util.data_util import graph_on_device  # noqa: E402
from tilingnn_amd.util.shape_processor import load_polygons  # noqa: E402
from tilingnn_amd.weights import make_state_dict  # noqa: E402

out_dir = sys.argv[1]
os.makedirs(out_dir, exist_ok=True)
tmp = tempfile.mkdtemp()
path = os.path.join(tmp, "g.pkl")
with gzip.open(os.path.join(GOLDEN, "complete_graph_ring9.pkl.gz"), "rb") as src, open(path, "wb") as dst:
    shutil.copyfileobj(src, dst)
g = TileGraph(2)
g.load_graph_state(path, sidecar=False)
shutil.rmtree(tmp)
dev = torch.device("cuda:0")
od = graph_on_device(g, dev)
n = od.n_tiles
col = g.arrays.colli_edges
lines = []

# ---- host cost of the contact relation and the sweep direction
host = []
for _ in range(5):
    t0 = time.perf_counter()
    ring_xy, ring_ptr, _, _ = union_geometry([t.tile_poly.exterior for t in g.tiles], col, n)
    t1 = time.perf_counter()
    theta = sweep_direction(ring_xy, ring_ptr)
    touch_ptr, touch_idx = contact_geometry(ring_xy, ring_ptr)
    host.append((time.perf_counter() - t1, t1 - t0))
lines.append(f"host, ring 9: contact_geometry + sweep_direction {1e3 * np.median([h[0] for h in host]):.0f} ms (median of 5; "
             f"{touch_idx.size} entries, longest row {int(np.diff(touch_ptr).max())}, theta {theta}); union_geometry before it "
             f"{1e3 * np.median([h[1] for h in host]):.0f} ms")

geo = od._union_geometry()
top = od._topology_geometry()


def calls(alive):
    k = int(alive.shape[0])
    area = torch.empty(k, dtype=torch.float64, device=dev)
    out = torch.empty(k, 3, dtype=torch.int32, device=dev)
    err = torch.zeros(1, dtype=torch.int32, device=dev)
    a_bytes = int(lib.tgnn_union_area_workspace_bytes(k, n))
    a_ws = torch.empty(a_bytes // 8, dtype=torch.float64, device=dev)
    t_bytes = int(lib.tgnn_union_topology_workspace_bytes(k, n))
    t_ws = torch.empty(t_bytes // 4, dtype=torch.int32, device=dev)
    stream = _lib.current_stream(dev)
    area_call = lambda: check(lib.tgnn_union_area(ptr(geo[0]), ptr(geo[1]), n, ptr(geo[2]), ptr(geo[3]), ptr(alive), k, UNION_TOL,
                                                  ptr(area), ptr(err), ptr(a_ws), a_bytes, stream))
    topo_call = lambda: check(lib.tgnn_union_topology(ptr(geo[0]), ptr(geo[1]), n, ptr(geo[2]), ptr(geo[3]), ptr(top[0]),
                                                      ptr(top[1]), ptr(alive), k, UNION_TOL, top[2], top[3], ptr(out), ptr(err),
                                                      ptr(t_ws), t_bytes, stream))
    return area_call, topo_call, out, err


def timed(name, alive, reps=15):
    area_call, topo_call, out, err = calls(alive)
    for _ in range(3):
        area_call()
        topo_call()
    torch.cuda.synchronize()
    took = {"tgnn_union_area": [], "tgnn_union_topology": []}
    for _ in range(reps):
        for label, call in (("tgnn_union_area", area_call), ("tgnn_union_topology", topo_call)):
            t0 = time.perf_counter()
            call()
            torch.cuda.synchronize()
            took[label].append(1e3 * (time.perf_counter() - t0))
    assert int(err.item()) == 0
    o = out.cpu().numpy()
    share = float((alive != 0).float().mean())
    lines.append(f"{name}: {share:.1%} of the {alive.shape[0]} x {n} tiles alive; holes {o[:, 1].min()} .. {o[:, 1].max()}, "
                 f"components {o[:, 0].min()} .. {o[:, 0].max()}, status != 0 in {int((o[:, 2] != 0).sum())}")
    for label, t in took.items():
        lines.append(f"    {label}: median {np.median(t):.3f} ms, min {min(t):.3f}, max {max(t):.3f} (host clock around a "
                     f"synchronise, {reps} calls, interleaved)")


# ---- 4 096 thinned independent sets: 64 maximal independent sets, each thinned 64 ways
rng = np.random.default_rng(0)
base = [to.independent_set(n, col, seed) for seed in range(64)]
masks = np.stack([b & (rng.random(n) > 0.3) for b in base for _ in range(64)]).astype(np.int32)
timed("4 096 thinned independent sets of ring 9", torch.from_numpy(masks).to(dev))

# ---- the README flow on the bunny: crops -> solve_many -> detect_holes_many
ext, holes = load_polygons(os.path.join(GOLDEN, "silhouettes", "bunny.txt"))
crops = tf.crop_multiple_layouts_from_contour(ext, holes, g, device=dev, coverage=True, start_angle=0.0, end_angle=60.0,
                                              num_of_angle=6, movement_delta_ratio=[0, 0.5], margin_padding_ratios=[0.5])
net = TilinGNN(adj_edge_features_dim=15, network_depth=20, network_width=32, node_features_dim=3)
net.load_state_dict(make_state_dict(15, 20, 32, 1, 3, seed=0), strict=True)
net = net.to(dev).train()
solutions = ML_Solver(None, dev, g, net, num_prob_maps=1).solve_many([c[0] for c in crops])
t0 = time.perf_counter()
found = detect_holes_many([s for s, _ in solutions])
took = 1e3 * (time.perf_counter() - t0)
lines.append(f"README flow, bunny: {len(crops)} crops solved by one solve_many; detect_holes_many -> (components, holes) {found} "
             f"in {took:.2f} ms (host clock, masks built on the host, one call, one read-back)")
alive = np.zeros((len(solutions), n), dtype=np.int32)
for k, (s, _) in enumerate(solutions):
    alive[k, s.selected_tiles()] = 1
timed(f"the {len(solutions)} solved bunny crops", torch.from_numpy(alive).to(dev))
open(os.path.join(out_dir, "union_topology_times.txt"), "w").write("\n".join(lines) + "\n")
print("\n".join(lines))
