"""Times of the hole-free greedy solve with the guarded sweep on the host (HoleGuard: one map call per accepted tile) and on the
device (DeviceHoleSweep, csrc/hole_sweep.hip: one call per round), on ring 9 with the whole graph as the layout -- the stub
recipe of tests/test_hole_guard_solve.py, seed 0, and TilinGNN with the seed-0 weights -- and of ML_Solver.solve_many_hole_free
over 8 ring-9 cuts beside the same 8 solved one after another by the host-guarded path.  One process, the two ways interleaved
(A B A B ...), host clock around a synchronise, median and spread of the repeats.
Usage: python scratch/hole_sweep_times.py OUT_DIR [--profile]   (--profile: three device-sweep stub solves and nothing else,
for a rocprofv3 --kernel-trace --stats run of its own)"""
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
from tests.golden_util import GOLDEN  # noqa: E402
from tilingnn_amd import TilinGNN  # noqa: E402
from tilingnn_amd.solver.ml_solver.ml_solver import ML_Solver  # noqa: E402
from tilingnn_amd.tiling.brick_layout import BrickLayout, detect_holes_many  # noqa: E402
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
n = len(g.tiles)
cut = lambda tiles: BrickLayout(g, *du.create_brick_layout_from_super_set(g, [int(t) for t in tiles]))
layout = cut(range(n))
lines = []


class Stub:
    """The recipe's probabilities for one layout (predict) or K (predict_many: every sub-layout names its layout)."""
    device = dev

    def __init__(self, seeds=(0,), layouts=(layout,)):
        self.seeds = list(seeds)
        self.tiles = [np.array([l.inverse_index[i] for i in range(len(l.node_feature))]) for l in layouts]
        self.rounds = [0] * len(self.tiles)

    def _probs(self, k, sub):
        self.rounds[k] += 1
        return hg.round_probs(self.seeds[k], self.rounds[k], n, self.tiles[k][sub.inverse_index.cpu().numpy()])

    def predict(self, sub):
        return self._probs(0, sub)

    def predict_many(self, subs):
        return [self._probs(sub.origin_index, sub) for sub in subs]


def stub_solve(device_sweep):
    sel, _, order = alg.solve_by_probablistic_greedy(Stub(), layout, score_fn=lambda s, l: None, check_holes=True, device_sweep=device_sweep)
    return sel, order


if profile:
    for _ in range(3):
        np.random.seed(0)
        stub_solve(True)
    torch.cuda.synchronize()
    sys.exit(0)


def interleaved(name, solve, reps):
    """solve(device_sweep) -> (selection, order), host sweep and device sweep turn by turn; one warm-up of each."""
    took, results = {False: [], True: []}, {}
    for rep in range(reps + 1):
        for on in (False, True):
            np.random.seed(0)
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            results[on] = solve(on)
            torch.cuda.synchronize()
            if rep:
                took[on].append(1e3 * (time.perf_counter() - t0))
            guard = alg.solve_by_probablistic_greedy.last_guard
            results[on] += ((guard.launches, guard.vetoes) if not on else (int(guard.launches[0]), int(guard.vetoes[0])),)
    same = np.array_equal(results[False][0], results[True][0]) and results[False][1] == results[True][1]
    lines.append(f"{name}: {int(results[True][0].sum())} tiles, {results[True][2][1]} vetoes; the two ways agree: {same}")
    for on in (False, True):
        t = took[on]
        lines.append(f"    device_sweep={on}: median {np.median(t):.1f} ms, min {min(t):.1f}, max {max(t):.1f} ({reps} solves, host clock around "
                     f"a synchronise, interleaved); {results[on][2][0]} guard launches")


interleaved("ring 9 solve, check_holes=True, stub recipe seed 0", stub_solve, 5)

net = TilinGNN(adj_edge_features_dim=15, network_depth=20, network_width=32, node_features_dim=3)
net.load_state_dict(make_state_dict(15, 20, 32, 1, 3, seed=0), strict=True)
net = net.to(dev).train()
solver = ML_Solver(None, dev, g, net, num_prob_maps=1, score_fn=lambda s, l: None)


def net_solve(device_sweep):
    out, _ = solver.solve(layout, check_holes=True, device_sweep=device_sweep)
    return out.predict, out.predict_order


interleaved("ring 9 solve, check_holes=True, TilinGNN with the seed-0 weights (no trained checkpoint is in the repository)", net_solve, 5)

# ---- K = 8 cuts of ring 9: one loop for all against one host-guarded solve after the other
cuts = [cut(np.flatnonzero(np.random.default_rng(100 + k).random(n) < 0.5)) for k in range(8)]
seeds = list(range(8))


class Stubbed(ML_Solver):
    def __init__(self, stub):
        self.device, self._greedy_solver, self._score_fn, self.stub = dev, None, (lambda s, l: None), stub
        self.device_greedy_min_nodes, self.device_greedy_seed = None, 0

    def predict(self, sub):
        return self.stub.predict(sub)

    def predict_many(self, subs):
        return self.stub.predict_many(subs)


def many(make_solver):
    return [(o.predict, o.predict_order) for o, _ in make_solver().solve_many_hole_free(cuts, seed=seeds)]


def one_by_one(make_solo):
    out = []
    for k, (c, seed) in enumerate(zip(cuts, seeds)):
        np.random.seed(seed)
        sel, _, order = alg.solve_by_probablistic_greedy(make_solo(k), c, score_fn=lambda s, l: None, check_holes=True)
        out.append((sel, order))
    return out


def many_times(name, make_solver, make_solo, reps):
    took, results = {"one": [], "many": []}, {}
    for rep in range(reps + 1):
        for which, run in (("one", lambda: one_by_one(make_solo)), ("many", lambda: many(make_solver))):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            results[which] = run()
            torch.cuda.synchronize()
            if rep:
                took[which].append(1e3 * (time.perf_counter() - t0))
    same = all(np.array_equal(a[0], b[0]) and a[1] == b[1] for a, b in zip(results["one"], results["many"]))
    solved = []
    for c, (sel, _) in zip(cuts, results["many"]):
        c = cut([c.inverse_index[i] for i in range(len(c.node_feature))])
        c.predict = sel
        solved.append(c)
    holes = [h for _, h in detect_holes_many(solved, dev)]
    lines.append(f"{name}: 8 cuts of ring 9 ({[len(c.node_feature) for c in cuts]} nodes), rounds {alg.solve_many_hole_free.last_rounds}, "
                 f"{alg.solve_many_hole_free.last_sweep_calls} sweep calls, holes {holes}; the two ways agree: {same}")
    lines.append(f"    8 host-guarded solves one after another: median {np.median(took['one']):.1f} ms, min {min(took['one']):.1f}, max "
                 f"{max(took['one']):.1f}; solve_many_hole_free: median {np.median(took['many']):.1f} ms, min {min(took['many']):.1f}, "
                 f"max {max(took['many']):.1f} ({reps} runs each, host clock around a synchronise, interleaved)")


many_times("stub recipe, seeds 0..7", lambda: Stubbed(Stub(seeds, cuts)), lambda k: Stub([seeds[k]], [cuts[k]]), 3)
many_times("TilinGNN with the seed-0 weights", lambda: solver, lambda k: solver, 3)
open(os.path.join(out_dir, "hole_sweep_times.txt"), "w").write("\n".join(lines) + "\n")
print("\n".join(lines))
