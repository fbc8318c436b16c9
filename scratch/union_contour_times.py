"""Times of the union-contour call (csrc/union_contour.hip) beside the union-topology call (csrc/union_topology.hip) on the same
masks of the labyrinth complete graph: the two mask sets of scratch/union_topology_times.py.  Host clock around a synchronise,
one call per measurement, the two calls interleaved (A B A B ...), median and spread of the repeats.  The read-back of the error
word is outside the clock.
Usage: python scratch/union_contour_times.py OUT_DIR [--profile]   (--profile: five contour calls on the first set and nothing
else, for a kernel trace)"""
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
from tilingnn_amd.tiling.region import UNION_TOL  # noqa: E402
from tilingnn_amd.tiling.tile_graph import TileGraph  # noqa: E402
from tilingnn_amd.util.data_util import graph_on_device  # noqa: E402
from tilingnn_amd.util.shape_processor import load_polygons  # noqa: E402
from tilingnn_amd.weights import make_state_dict  # noqa: E402

out_dir = sys.argv[1]
profile = "--profile" in sys.argv[2:]
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
geo = od._union_geometry()
top = od._topology_geometry()
verts = (geo[1][1:] - geo[1][:-1]).to(torch.float64)


def calls(alive):
    k = int(alive.shape[0])
    out = torch.empty(k, 3, dtype=torch.int32, device=dev)
    err = torch.zeros(1, dtype=torch.int32, device=dev)
    t_bytes = int(lib.tgnn_union_topology_workspace_bytes(k, n))
    t_ws = torch.empty(t_bytes // 4, dtype=torch.int32, device=dev)
    bound = 2 * int(((alive != 0).to(torch.float64) @ verts).sum().item())
    cap_rings = bound // 3 + 1
    mask_out = torch.empty(k, 4, dtype=torch.int32, device=dev)
    ring_out, ring_area = torch.empty(cap_rings, 4, dtype=torch.int32, device=dev), torch.empty(cap_rings, dtype=torch.float64, device=dev)
    pts_xy, pts_src = torch.empty(bound, 2, dtype=torch.float64, device=dev), torch.empty(bound, dtype=torch.int32, device=dev)
    total = torch.zeros(2, dtype=torch.int64, device=dev)
    c_bytes = int(lib.tgnn_union_contour_workspace_bytes(k, n, bound))
    c_ws = torch.empty(c_bytes // 8 + 1, dtype=torch.int64, device=dev)
    stream = _lib.current_stream(dev)
    topo_call = lambda: check(lib.tgnn_union_topology(ptr(geo[0]), ptr(geo[1]), n, ptr(geo[2]), ptr(geo[3]), ptr(top[0]),
                                                      ptr(top[1]), ptr(alive), k, UNION_TOL, top[2], top[3], ptr(out), ptr(err),
                                                      ptr(t_ws), t_bytes, stream))
    contour_call = lambda: check(lib.tgnn_union_contour(ptr(geo[0]), ptr(geo[1]), n, ptr(geo[2]), ptr(geo[3]), ptr(top[0]),
                                                        ptr(top[1]), ptr(alive), k, UNION_TOL, cap_rings, bound, ptr(mask_out),
                                                        ptr(ring_out), ptr(ring_area), ptr(pts_xy), ptr(pts_src), ptr(total),
                                                        ptr(err), ptr(c_ws), c_bytes, stream))
    return topo_call, contour_call, out, mask_out, total, err, c_bytes


def timed(name, alive, reps=15):
    topo_call, contour_call, out, mask_out, total, err, c_bytes = calls(alive)
    for _ in range(3):
        topo_call()
        contour_call()
    torch.cuda.synchronize()
    took = {"tgnn_union_topology": [], "tgnn_union_contour": []}
    for _ in range(reps):
        for label, call in (("tgnn_union_topology", topo_call), ("tgnn_union_contour", contour_call)):
            t0 = time.perf_counter()
            call()
            torch.cuda.synchronize()
            took[label].append(1e3 * (time.perf_counter() - t0))
    assert int(err.item()) == 0
    o, m, t = out.cpu().numpy(), mask_out.cpu().numpy(), total.cpu().numpy()
    assert (m[:, 0] == o[:, 0] + o[:, 1]).all()
    share = float((alive != 0).float().mean())
    lines.append(f"{name}: {share:.1%} of the {alive.shape[0]} x {n} tiles alive; holes {o[:, 1].min()} .. {o[:, 1].max()}, "
                 f"components {o[:, 0].min()} .. {o[:, 0].max()}; {int(t[0])} rings, {int(t[1])} points, at most "
                 f"{int(m[:, 2].max())} points in a mask; contour workspace {c_bytes / 2 ** 20:.1f} MiB")
    for label, ms in took.items():
        lines.append(f"    {label}: median {np.median(ms):.3f} ms, min {min(ms):.3f}, max {max(ms):.3f} (host clock around a "
                     f"synchronise, {reps} calls, interleaved)")


# ---- 4 096 thinned independent sets: 64 maximal independent sets, each thinned 64 ways
rng = np.random.default_rng(0)
base = [to.independent_set(n, col, seed) for seed in range(64)]
masks = torch.from_numpy(np.stack([b & (rng.random(n) > 0.3) for b in base for _ in range(64)]).astype(np.int32)).to(dev)
if profile:
    contour_call = calls(masks)[1]
    for _ in range(5):
        contour_call()
    torch.cuda.synchronize()
    sys.exit(0)
timed("4 096 thinned independent sets of ring 9", masks)

# ---- the 24 solved bunny crops of the README flow
ext, holes = load_polygons(os.path.join(GOLDEN, "silhouettes", "bunny.txt"))
crops = tf.crop_multiple_layouts_from_contour(ext, holes, g, device=dev, coverage=True, start_angle=0.0, end_angle=60.0,
                                              num_of_angle=6, movement_delta_ratio=[0, 0.5], margin_padding_ratios=[0.5])
net = TilinGNN(adj_edge_features_dim=15, network_depth=20, network_width=32, node_features_dim=3)
net.load_state_dict(make_state_dict(15, 20, 32, 1, 3, seed=0), strict=True)
net = net.to(dev).train()
solutions = ML_Solver(None, dev, g, net, num_prob_maps=1).solve_many([c[0] for c in crops])
alive = np.zeros((len(solutions), n), dtype=np.int32)
for k, (s, _) in enumerate(solutions):
    alive[k, s.selected_tiles()] = 1
timed(f"the {len(solutions)} solved bunny crops", torch.from_numpy(alive).to(dev))
from tilingnn_amd.tiling.brick_layout import union_polygons_many  # noqa: E402
t0 = time.perf_counter()
polys = union_polygons_many([s for s, _ in solutions])
took = 1e3 * (time.perf_counter() - t0)
lines.append(f"README flow, bunny: union_polygons_many of the {len(solutions)} solutions -> {sum(len(p) for p in polys)} regions, "
             f"{sum(len(r.interiors) for p in polys for r in p)} holes, {sum(r.exterior.shape[0] for p in polys for r in p)} "
             f"exterior points in {took:.2f} ms (host clock, masks built on the host, one call, one read-back)")
open(os.path.join(out_dir, "union_contour_times.txt"), "w").write("\n".join(lines) + "\n")
print("\n".join(lines))
