"""K greedy solves: a Python loop of solve_by_device_greedy (the baseline) against solve_many_by_device_greedy, same layouts, same
seed, one process, warmed up, A/B interleaved.  Workloads: the bunny crops of tests/test_solve_many.py, the crops of the README's
silhouette example (num_of_angle=6), 32 synthetic layouts of 1 000 nodes.  Weights: make_state_dict(..., seed=0).

    python scratch/solve_many_times.py --out profiles/solve_many_times.txt            (times, rounds, synchronisations)
    python scratch/solve_many_times.py --trace bunny                                  (one batched solve, for rocprofv3 --kernel-trace --stats)
"""
import argparse
import gzip
import os
import shutil
import statistics
import sys
import tempfile
import time

import numpy as np
import torch

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)
GOLDEN = os.path.join(REPO, "tests", "golden")
DEV = torch.device("cuda:0")


def crops(num_of_angle, paddings):
    from tilingnn_amd.tiling import tile_factory as tf
    from tilingnn_amd.tiling.tile_graph import TileGraph
    from tilingnn_amd.util.shape_processor import load_polygons
    tmp = tempfile.mkdtemp()
    path = os.path.join(tmp, "complete_graph_ring9.pkl")
    with gzip.open(os.path.join(GOLDEN, "complete_graph_ring9.pkl.gz"), "rb") as src, open(path, "wb") as dst:
        shutil.copyfileobj(src, dst)
    graph = TileGraph(2)
    graph.load_graph_state(path, sidecar=False)
    ext, holes = load_polygons(os.path.join(GOLDEN, "silhouettes", "bunny.txt"))
    got = tf.crop_multiple_layouts_from_contour(ext, holes, graph, device=str(DEV), coverage=True, start_angle=0.0, end_angle=60.0,
                                                num_of_angle=num_of_angle, movement_delta_ratio=[0, 0.5], margin_padding_ratios=paddings)
    return graph, [c[0] for c in got]


def synthetic(k, n):
    from tilingnn_amd.synth import make_super_graph
    from tilingnn_amd.util.algorithms import DeviceLayout
    out = []
    for i in range(k):
        x, a, attr, c, _ = make_super_graph(n, 8 * n, 10 * n, tile_count=2, n_edge_types=13, seed=100 + i).to_torch(DEV)
        out.append(DeviceLayout(x, a, attr, c))
    return None, out


WORKLOADS = {"bunny": lambda: crops(3, [0.5, 0.05]), "readme": lambda: crops(6, [0.5]), "synth32": lambda: synthetic(32, 1000)}


def solver(graph):
    from tilingnn_amd import TilinGNN
    from tilingnn_amd.solver.ml_solver.ml_solver import ML_Solver
    from tilingnn_amd.weights import make_state_dict
    net = TilinGNN(adj_edge_features_dim=15, network_depth=20, network_width=32, node_features_dim=3)
    net.load_state_dict(make_state_dict(15, 20, 32, 1, 3, seed=0), strict=True)
    return ML_Solver(None, DEV, graph, net.to(DEV).train(), num_prob_maps=1)


def timed(fn):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    out = fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) * 1e3, out


def measure(name, reps, say):
    from tilingnn_amd.util import algorithms as alg
    graph, layouts = WORKLOADS[name]()
    ms = solver(graph)
    sizes = [int(l.node_feature.shape[0]) for l in layouts]

    def loop():
        out, rounds = [], []
        for l in layouts:
            out.append(alg.solve_by_device_greedy(ms, l, seed=0))
            rounds.append(alg.solve_by_device_greedy.last_rounds)
        return out, rounds
    many = lambda: alg.solve_many_by_device_greedy(ms, layouts, seed=0)
    for _ in range(2):                                           # warm-up: allocator, graph-prep paths, stream measurement
        (want, rounds), got = loop(), many()
    assert all(np.array_equal(a[0], b[0]) and a[1] == b[1] and a[2] == b[2] for a, b in zip(want, got))
    assert rounds == alg.solve_many_by_device_greedy.last_rounds
    # share of the batched loop inside forward_many + the health poll (host clock; the poll synchronises)
    inner, fwd_ms = alg._forward_many_checked, [0.0, 0]

    def clocked(*a):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        out = inner(*a)
        fwd_ms[0] += (time.perf_counter() - t0) * 1e3
        fwd_ms[1] += 1
        return out
    alg._forward_many_checked = clocked
    total, _ = timed(many)
    alg._forward_many_checked = inner
    base, cand = [], []
    for _ in range(reps):                                        # A/B interleaved
        base.append(timed(loop)[0])
        cand.append(timed(many)[0])
    mb, mc = statistics.median(base), statistics.median(cand)
    spread = (max(base) - min(base)) / mb
    say(f"{name}: {len(layouts)} layouts, {min(sizes)}..{max(sizes)} nodes ({sum(sizes)} in all), rounds {min(rounds)}..{max(rounds)} "
        f"(sum {sum(rounds)}, longest {max(rounds)})")
    say(f"  baseline  loop of solve_by_device_greedy : median {mb:9.2f} ms  min {min(base):9.2f}  max {max(base):9.2f}  (relative spread {spread:.3f})")
    say(f"  candidate solve_many_by_device_greedy    : median {mc:9.2f} ms  min {min(cand):9.2f}  max {max(cand):9.2f}")
    say(f"  ratio {mb / mc:.2f}x; gain {(mb - mc) / mb:.3f} of the baseline against 3 x spread = {3 * spread:.3f}: "
        f"{'DONE' if (mb - mc) / mb > 3 * spread else 'NOT beyond the noise margin'}")
    say(f"  read-backs that synchronise: baseline {sum(rounds) + len(layouts)} compactions + one health poll per scored round; candidate "
        f"{max(rounds) + 1} compactions + {fwd_ms[1]} health polls (1 + 1 per round against K + K)")
    say(f"  inside forward_many + poll: {fwd_ms[0]:.2f} ms of {total:.2f} ms ({fwd_ms[0] / total:.2f} of the batched solve, {fwd_ms[1]} calls)")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--workloads", default="bunny,readme,synth32")
    ap.add_argument("--trace", default=None, help="run ONE batched solve of this workload after a warm-up and exit")
    args = ap.parse_args()
    if args.trace:
        from tilingnn_amd.util import algorithms as alg
        graph, layouts = WORKLOADS[args.trace]()
        ms = solver(graph)
        for _ in range(3):
            alg.solve_many_by_device_greedy(ms, layouts, seed=0)
        torch.cuda.synchronize()
        print(f"traced {args.trace}: 3 batched solves of {len(layouts)} layouts, rounds {alg.solve_many_by_device_greedy.last_rounds}")
        return
    lines = []

    def say(s):
        print(s, flush=True)
        lines.append(s)
    say(f"solve_many_times: {torch.cuda.get_device_name(0)}, GPU_MAX_HW_QUEUES={os.environ.get('GPU_MAX_HW_QUEUES', 'unset')}, "
        f"{args.reps} interleaved repetitions, host clock around a device synchronise")
    for name in args.workloads.split(","):
        measure(name, args.reps, say)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
