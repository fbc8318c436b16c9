"""Times of the hole-delta call (csrc/union_hole_delta.hip) on ring 9 beside the only other way to the same answer --
tgnn_union_topology over all the (mask + t) rows, one row per candidate -- and of the guarded greedy solve beside the unguarded
one.  Host clock around a synchronise, one call per measurement, the two calls interleaved (A B A B ...), median and spread of
the repeats; the read-back of the error word is outside the clock.
Usage: python scratch/union_hole_delta_times.py OUT_DIR [--profile]   (--profile: five hole-delta calls on the 4 096 masks and
nothing else, for a rocprofv3 --kernel-trace --stats run of its own)"""
import gzip
import os
import shutil
import sys
import tempfile
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from tests import hole_guard_restatement as hg  # noqa: E402
from tests import topology_oracle as to  # noqa: E402
from tests.golden_util import GOLDEN  # noqa: E402
from tilingnn_amd import TilinGNN, _lib  # noqa: E402
from tilingnn_amd._lib import check, lib, ptr  # noqa: E402
from tilingnn_amd.solver.ml_solver.ml_solver import ML_Solver  # noqa: E402
from tilingnn_amd.tiling.brick_layout import BrickLayout  # noqa: E402
from tilingnn_amd.tiling.region import UNION_TOL  # noqa: E402
from tilingnn_amd.tiling.tile_graph import TileGraph  # noqa: E402
from tilingnn_amd.util import algorithms as alg  # noqa: E402
from tilingnn_amd.util import data_util as du  # noqa: E402
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
od = du.graph_on_device(g, dev)
n = od.n_tiles
col = g.arrays.colli_edges
geo = od._union_geometry()
top = od._topology_geometry()
stream = _lib.current_stream(dev)
lines = []


def delta_call(alive):
    k = int(alive.shape[0])
    delta = torch.empty(k, n, 2, dtype=torch.int32, device=dev)
    state = torch.empty(k, n, dtype=torch.int32, device=dev)
    err = torch.zeros(1, dtype=torch.int32, device=dev)
    ws_bytes = int(lib.tgnn_union_hole_delta_workspace_bytes(k, n))
    ws = torch.empty(ws_bytes // 4, dtype=torch.int32, device=dev)
    call = lambda: check(lib.tgnn_union_hole_delta(ptr(geo[0]), ptr(geo[1]), n, ptr(geo[2]), ptr(geo[3]), ptr(top[0]), ptr(top[1]),
                                                   ptr(alive), k, UNION_TOL, top[2], top[3], ptr(delta), ptr(state), ptr(err),
                                                   ptr(ws), ws_bytes, stream))
    return call, delta, state, err


def topology_call(alive):
    k = int(alive.shape[0])
    out = torch.empty(k, 3, dtype=torch.int32, device=dev)
    err = torch.zeros(1, dtype=torch.int32, device=dev)
    ws_bytes = int(lib.tgnn_union_topology_workspace_bytes(k, n))
    ws = torch.empty(ws_bytes // 4, dtype=torch.int32, device=dev)
    call = lambda: check(lib.tgnn_union_topology(ptr(geo[0]), ptr(geo[1]), n, ptr(geo[2]), ptr(geo[3]), ptr(top[0]), ptr(top[1]),
                                                 ptr(alive), k, UNION_TOL, top[2], top[3], ptr(out), ptr(err), ptr(ws), ws_bytes,
                                                 stream))
    return call, out, err


def timed(name, alive, reps=15):
    d_call, delta, state, d_err = delta_call(alive)
    d_call()
    torch.cuda.synchronize()
    ks, ts = torch.nonzero(state == 0, as_tuple=True)
    rows = torch.cat([alive, alive[ks]])                      # the masks themselves, then one row per candidate
    rows[alive.shape[0] + torch.arange(ks.shape[0], device=dev), ts] = 1
    t_call, out, t_err = topology_call(rows)
    for _ in range(2):
        d_call()
        t_call()
    torch.cuda.synchronize()
    took = {"tgnn_union_hole_delta": [], "tgnn_union_topology over the (mask + t) rows": []}
    for _ in range(reps):
        for label, call in zip(took, (d_call, t_call)):
            t0 = time.perf_counter()
            call()
            torch.cuda.synchronize()
            took[label].append(1e3 * (time.perf_counter() - t0))
    assert int(d_err.item()) == 0 and int(t_err.item()) == 0
    k = alive.shape[0]
    want = out[k:, :2] - out[ks, :2]
    assert bool((delta[ks, ts] == want).all()) and bool((out[:, 2] == 0).all())
    dh = delta[ks, ts][:, 1].cpu().numpy()
    lines.append(f"{name}: {float((alive != 0).float().mean()):.1%} of the {k} x {n} tiles alive, {ks.shape[0]} candidates "
                 f"({ks.shape[0] / k:.1f} a mask), d holes {dict(zip(*[v.tolist() for v in np.unique(dh, return_counts=True)]))}; "
                 f"the two ways agree on every candidate")
    for label, t in took.items():
        lines.append(f"    {label}: median {np.median(t):.3f} ms, min {min(t):.3f}, max {max(t):.3f} (host clock around a "
                     f"synchronise, {reps} calls, interleaved)")
    lines.append(f"    (the second way also needs its {rows.shape[0]} x {n} rows built: {rows.numel() * 4 / 2 ** 20:.0f} MiB, not in its time)")


rng = np.random.default_rng(0)
base = [to.independent_set(n, col, seed) for seed in range(64)]
masks = torch.from_numpy(np.stack([b & (rng.random(n) > 0.3) for b in base for _ in range(64)]).astype(np.int32)).to(dev)

if profile:
    call, *_ = delta_call(masks)
    for _ in range(5):
        call()
    torch.cuda.synchronize()
    sys.exit(0)

timed("4 096 thinned independent sets of ring 9", masks)
idx = np.flatnonzero(to.independent_set(n, col, 0))
half = np.zeros((1, n), dtype=np.int32)
half[0, np.random.default_rng(200).permutation(idx)[:len(idx) // 2]] = 1
timed("one half solution of ring 9 (seed 0)", torch.from_numpy(half).to(dev))

# ---- the guarded solve beside the unguarded one: the stub recipe of tests/test_hole_guard_solve.py, seed 0
layout = BrickLayout(g, *du.create_brick_layout_from_super_set(g, list(range(n))))


class Stub:
    device = dev

    def __init__(self):
        self.round = 0

    def predict(self, sub):
        self.round += 1
        return hg.round_probs(0, self.round, n, sub.inverse_index.cpu().numpy())


def solve_times(name, make_solver, solve, reps=5):
    for guarded in (False, True):
        took, accept = [], []
        for _ in range(reps + 1):
            solver = make_solver()
            np.random.seed(0)
            spent = [0.0]
            real = alg.HoleGuard.accept

            def clocked(self, node):
                t0 = time.perf_counter()
                real(self, node)
                spent[0] += time.perf_counter() - t0
            alg.HoleGuard.accept = clocked
            try:
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                sel, order = solve(solver, guarded)
                torch.cuda.synchronize()
                took.append(1e3 * (time.perf_counter() - t0))
            finally:
                alg.HoleGuard.accept = real
            accept.append(1e3 * spent[0])
        took, accept = took[1:], accept[1:]
        solved = BrickLayout(g, *du.create_brick_layout_from_super_set(g, list(range(n))))
        solved.predict = sel
        line = (f"{name}, {'guarded' if guarded else 'unguarded'}: {int(np.sum(sel))} tiles, (components, holes) {solved.count_holes(dev)}; "
                f"median {np.median(took):.1f} ms, min {min(took):.1f}, max {max(took):.1f} ({reps} solves, host clock)")
        if guarded:
            guard = alg.solve_by_probablistic_greedy.last_guard
            line += (f"; of that HoleGuard.accept {np.median(accept):.1f} ms in {guard.launches} calls "
                     f"({1e3 * np.median(accept) / guard.launches:.0f} us a call: index write, launch, one read-back, host gather), "
                     f"{guard.vetoes} vetoes")
        lines.append(line)


def stub_solve(solver, guarded):
    sel, _, order = alg.solve_by_probablistic_greedy(solver, layout, score_fn=lambda s, l: None, check_holes=guarded)
    return sel, order


solve_times("ring 9 solve, stub recipe seed 0", Stub, stub_solve)

net = TilinGNN(adj_edge_features_dim=15, network_depth=20, network_width=32, node_features_dim=3)
net.load_state_dict(make_state_dict(15, 20, 32, 1, 3, seed=0), strict=True)
net = net.to(dev).train()


def net_solve(solver, guarded):
    out, _ = solver.solve(layout, check_holes=guarded)
    return out.predict, out.predict_order


solve_times("ring 9 solve, TilinGNN with the seed-0 weights (no trained checkpoint is in the repository)",
            lambda: ML_Solver(None, dev, g, net, num_prob_maps=1, score_fn=lambda s, l: None), net_solve, reps=3)
open(os.path.join(out_dir, "union_hole_delta_times.txt"), "w").write("\n".join(lines) + "\n")
print("\n".join(lines))
