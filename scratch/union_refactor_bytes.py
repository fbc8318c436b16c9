"""Every output tensor of the four union calls (CompleteGraphOnDevice.union_areas, union_topology, hole_deltas, union_contours) on
the 4 096 thinned independent sets of ring 9 that scratch/union_topology_times.py times, written to one .npz -- to compare two
builds of the library byte for byte (the kernels sum in a fixed order, so equality is the expectation, not a tolerance):
    TGNN_LIB_PATH=<library A> python scratch/union_refactor_bytes.py a.npz
    TGNN_LIB_PATH=<library B> python scratch/union_refactor_bytes.py b.npz
    python scratch/union_refactor_bytes.py --compare a.npz b.npz"""
import gzip
import hashlib
import os
import shutil
import sys
import tempfile

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

if sys.argv[1] == "--compare":
    a, b = np.load(sys.argv[2]), np.load(sys.argv[3])
    assert sorted(a.files) == sorted(b.files), (a.files, b.files)
    same = []
    for name in a.files:
        x, y = a[name], b[name]
        same.append(x.dtype == y.dtype and x.shape == y.shape and x.tobytes() == y.tobytes())
        print(f"{name}: {x.dtype} {x.shape} sha256 {hashlib.sha256(x.tobytes()).hexdigest()[:16]} / "
              f"{hashlib.sha256(y.tobytes()).hexdigest()[:16]} {'identical' if same[-1] else 'DIFFERENT'}")
    print(f"union calls on the 4 096 masks, {sys.argv[2]} against {sys.argv[3]}: {sum(same)} of {len(same)} arrays byte-identical")
    sys.exit(0 if all(same) else 1)

import torch  # noqa: E402

from tests import topology_oracle as to  # noqa: E402
from tests.golden_util import GOLDEN  # noqa: E402
from tilingnn_amd import _lib  # noqa: E402
from tilingnn_amd.tiling.tile_graph import TileGraph  # noqa: E402
from tilingnn_amd.util.data_util import graph_on_device  # noqa: E402

tmp = tempfile.mkdtemp()
path = os.path.join(tmp, "g.pkl")
with gzip.open(os.path.join(GOLDEN, "complete_graph_ring9.pkl.gz"), "rb") as src, open(path, "wb") as dst:
    shutil.copyfileobj(src, dst)
g = TileGraph(2)
g.load_graph_state(path, sidecar=False)
shutil.rmtree(tmp)
od = graph_on_device(g, torch.device("cuda:0"))
n = od.n_tiles
col = g.arrays.colli_edges
rng = np.random.default_rng(0)
base = [to.independent_set(n, col, seed) for seed in range(64)]
masks = np.stack([b & (rng.random(n) > 0.3) for b in base for _ in range(64)]).astype(np.int32)
alive = torch.from_numpy(masks).to(od.device)
delta, state = od.hole_deltas(alive)
rings = od.union_contours(alive)
out = {"area": od.union_areas(alive), "topology": od.union_topology(alive), "hole_delta": delta, "hole_state": state,
       "contour_mask": rings.mask, "contour_ring": rings.ring, "contour_ring_area": rings.ring_area, "contour_pts_xy": rings.pts_xy,
       "contour_pts_src": rings.pts_src}
np.savez(sys.argv[1], **{name: t.cpu().numpy() for name, t in out.items()})
print(f"{_lib.LIB_PATH}: {len(out)} arrays of {masks.shape[0]} masks x {n} tiles -> {sys.argv[1]}")
