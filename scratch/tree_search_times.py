"""Times of the tree search with its branch sweeps on the device (solve_by_treesearch / ML_Solver.solve_tree, csrc/tree_sweep.hip)
on ring 9 with the whole graph as the layout: roots=8, beam=8, top_k=1, check_holes=True, run until the queue is empty -- eight
randomised hole-free tilings from ONE loop -- beside eight hole-free greedy solves with the device sweep one after another
(solve(layout, check_holes=True, device_sweep=True), csrc/hole_sweep.hip).  The two sides do NOT run the same algorithm (another
acceptance rule, another number of forwards): the ratio compares two ways to get eight hole-free tilings of one region, nothing
else.  Stub recipes (tests/hole_guard_restatement.py, tests/tree_search_restatement.py) and TilinGNN with the seed-0 weights.
One process, the two ways interleaved (A B A B ...), host clock around a synchronise, median and spread of the repeats.
Usage: python scratch/tree_search_times.py OUT_DIR [--profile]   (--profile: three stub searches and nothing else, for a
rocprofv3 --kernel-trace --stats run of its own)"""
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
from tests import tree_search_restatement as ts  # noqa: E402
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
layout = BrickLayout(g, *du.create_brick_layout_from_super_set(g, list(range(n))))
SEARCH = dict(roots=8, beam=8, top_k=1, check_holes=True, max_predictions=100000)
score = lambda s, l: float(np.sum(s))
lines = []


class Stub:
    """The recipes' probabilities: per greedy round (predict) and per prediction of a search (predict_top_maps)."""
    device = dev

    def __init__(self, seed=0):
        self.seed, self.rounds = seed, 0

    def predict(self, sub):
        self.rounds += 1
        return hg.round_probs(self.seed, self.rounds, n, sub.inverse_index.cpu().numpy())

    def predict_top_maps(self, subs, top_k):
        return [ts.recipe_maps(self.seed, n, 1, top_k)(sub.predict_index, sub.inverse_index.cpu().numpy()) for sub in subs]


def stub_tree():
    results, cnt = alg.solve_by_treesearch(Stub(), layout, seed=0, score_fn=score, **SEARCH)
    dsw = alg.solve_by_treesearch.last_sweep
    return [r[0] for r in results], dict(predictions=cnt, steps=alg.solve_by_treesearch.last_steps, calls=dsw.calls, vetoes=dsw.vetoes)


def stub_greedy():
    sels, rounds = [], 0
    for seed in range(8):
        np.random.seed(seed)
        stub = Stub(seed)
        sel, _, _ = alg.solve_by_probablistic_greedy(stub, layout, score_fn=score, check_holes=True, device_sweep=True)
        sels.append(sel)
        rounds += stub.rounds
    return sels, dict(predictions=rounds, calls=rounds)


if profile:
    for _ in range(3):
        stub_tree()
    torch.cuda.synchronize()
    sys.exit(0)

fe, fxd = int(np.asarray(layout.align_edge_features).shape[1]), int(np.asarray(layout.node_feature).shape[1])
net = TilinGNN(adj_edge_features_dim=fe, network_depth=20, network_width=32, node_features_dim=fxd)
net.load_state_dict(make_state_dict(fe, 20, 32, 1, fxd, seed=0), strict=True)
solver = ML_Solver(None, dev, g, net.to(dev).train(), num_prob_maps=1, score_fn=score)


def net_tree():
    out = solver.solve_tree(layout, seed=0, **SEARCH)
    dsw = alg.solve_by_treesearch.last_sweep
    return [o.predict for o, _ in out], dict(predictions=solver.last_predict_cnt, steps=alg.solve_by_treesearch.last_steps, calls=dsw.calls,
                                             vetoes=dsw.vetoes)


def net_greedy():
    sels, rounds = [], 0
    for seed in range(8):
        np.random.seed(seed)
        out, _ = solver.solve(layout, check_holes=True, device_sweep=True)
        sels.append(out.predict)
        rounds += int(alg.solve_by_probablistic_greedy.last_guard.launches[0])
    return sels, dict(predictions=rounds, calls=rounds)


def holes_of(sels):
    import copy
    outs = []
    for sel in sels:
        l = copy.deepcopy(layout)
        l.predict = np.asarray(sel, dtype=float)
        outs.append(l)
    return [h for _, h in detect_holes_many(outs, dev)]


def interleaved(name, tree, greedy, reps=5):
    tree(), greedy()                                             # one warm-up of each
    times = {"tree": [], "greedy": []}
    for _ in range(reps):
        for key, fn in (("tree", tree), ("greedy", greedy)):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            sels, info = fn()
            torch.cuda.synchronize()
            times[key].append((time.perf_counter() - t0) * 1e3)
            if key == "tree":
                t_sels, t_info = sels, info
            else:
                g_sels, g_info = sels, info
    med = {k: float(np.median(v)) for k, v in times.items()}
    lines.append(f"{name}, ring 9 ({n} nodes), {reps} runs each, host clock around a synchronise, interleaved:")
    lines.append(f"    tree search (roots=8, beam=8, top_k=1, check_holes, to an empty queue): median {med['tree']:.1f} ms, min "
                 f"{min(times['tree']):.1f}, max {max(times['tree']):.1f}; {len(t_sels)} distinct tilings of "
                 f"{[int(s.sum()) for s in t_sels]} tiles, holes {holes_of(t_sels)}; {t_info}")
    lines.append(f"    8 x solve(check_holes=True, device_sweep=True) one after another: median {med['greedy']:.1f} ms, min "
                 f"{min(times['greedy']):.1f}, max {max(times['greedy']):.1f}; tilings of {[int(s.sum()) for s in g_sels]} tiles, holes "
                 f"{holes_of(g_sels)}; {g_info}")
    lines.append(f"    ratio greedy / tree: {med['greedy'] / med['tree']:.2f} (two ways to eight hole-free tilings; not the same algorithm)")


interleaved("stub recipes", stub_tree, stub_greedy)
interleaved("TilinGNN with the seed-0 weights (no trained checkpoint is in the repository)", net_tree, net_greedy)
text = "\n".join(lines)
print(text)
with open(os.path.join(out_dir, "tree_search_times.txt"), "w") as f:
    f.write(text + "\n")
