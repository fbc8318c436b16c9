"""forward_many / solve_many with the small layouts' graphs prepared by ONE library call per round (union_prep=True /
ML_Solver.union_prep = True, on top of the union forward) against the union forward alone (every layout's graph prepared by its
own call and its own host synchronisation on a lane): same layouts, same seed, one process, warmed up, A/B interleaved.
Workloads: those of scratch/solve_many_times.py (12 bunny crops, the 24 crops of the README's example, 32 synthetic layouts of
1 000 nodes).  forward_many is timed with a COLD graph cache (cleared in front of every call): the first round of a solve.

    python scratch/union_prep_times.py --out profiles/union_prep_times.txt        (times)
    python scratch/union_prep_times.py --trace bunny [--union-prep]                (three batched solves, for rocprofv3 --kernel-trace --stats)
    python scratch/forward_union_times.py --summarise a_kernel_trace.csv           (launches by kernel name)
"""
import argparse
import os
import statistics
import sys

import numpy as np
import torch

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)
sys.path.insert(0, os.path.join(REPO, "scratch"))
from forward_union_times import ab  # noqa: E402
from solve_many_times import DEV, WORKLOADS, solver  # noqa: E402


def report(say, what, base, cand):
    mb, mc = statistics.median(base), statistics.median(cand)
    spread = (max(base) - min(base)) / mb
    gain = (mb - mc) / mb
    say(f"  {what}")
    say(f"    union forward alone: median {mb:9.3f} ms  ({min(base):.3f} - {max(base):.3f})  relative spread {spread:.3f}")
    say(f"    ... with union_prep: median {mc:9.3f} ms  ({min(cand):.3f} - {max(cand):.3f})")
    say(f"    ratio {mb / mc:.2f}x; gain {gain:.3f} of the baseline against 3 x spread = {3 * spread:.3f}: "
        f"{'a gain beyond the noise margin' if gain > 3 * spread else 'NOT beyond the noise margin'}")


def measure(name, reps, say):
    from tilingnn_amd import _lib
    from tilingnn_amd.graph_networks import _graph_cache
    from tilingnn_amd.util import algorithms as alg
    from tilingnn_amd.util.algorithms import PackedLayouts
    graph, layouts = WORKLOADS[name]()
    ms = solver(graph)
    ms.union_forward = True
    net = ms.network
    pk = PackedLayouts(layouts, DEV)
    views = [pk.layout(k) for k in range(pk.k)]
    args = [(v.node_feature, v.align_edge_index, v.align_edge_features, v.collide_edge_index) for v in views]
    sizes = [int(a[0].shape[0]) for a in args]

    def cold(**kw):
        def run():
            _graph_cache.clear()
            return net.forward_many(args, union=True, **kw)
        return run
    fwd, fwd_p = cold(), cold(union_prep=True)
    many = lambda: alg.solve_many_by_device_greedy(ms, layouts, seed=0)

    def many_p():
        ms.union_prep = True
        try:
            return many()
        finally:
            ms.union_prep = False
    for _ in range(2):                                           # warm-up: allocator, stream measurement, the library's buffers
        a, b = fwd(), fwd_p()
        want, got = many(), many_p()
    torch.cuda.synchronize()
    assert all(torch.equal(x, y) for x, y in zip(a, b))
    assert all(np.array_equal(x[0], y[0]) and x[1] == y[1] and x[2] == y[2] for x, y in zip(want, got))
    rounds = alg.solve_many_by_device_greedy.last_rounds
    c0 = _lib.graph_prep_small_many_counts()
    fwd_p()
    c1 = _lib.graph_prep_small_many_counts()
    many_p()
    c2 = _lib.graph_prep_small_many_counts()
    say(f"{name}: {len(layouts)} layouts, {min(sizes)}..{max(sizes)} nodes ({sum(sizes)} in all), rounds {min(rounds)}..{max(rounds)}; "
        f"first round: {c1[1] - c0[1]} layouts prepared in {c1[0] - c0[0]} launch(es); one solve_many: {c2[1] - c1[1]} layouts in "
        f"{c2[0] - c1[0]} launches")
    report(say, "forward_many on the first-round layouts, cold graph cache", *ab(fwd, fwd_p, reps))
    report(say, "solve_many (the whole greedy loop)", *ab(many, many_p, reps))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--workloads", default="bunny,readme,synth32")
    ap.add_argument("--trace", default=None, help="run three batched solves of this workload after a warm-up and exit")
    ap.add_argument("--union-prep", action="store_true", help="--trace: with ML_Solver.union_prep = True beside union_forward")
    args = ap.parse_args()
    if args.trace:
        from tilingnn_amd.util import algorithms as alg
        graph, layouts = WORKLOADS[args.trace]()
        ms = solver(graph)
        ms.union_forward = True
        ms.union_prep = args.union_prep
        for _ in range(3):
            alg.solve_many_by_device_greedy(ms, layouts, seed=0)
        torch.cuda.synchronize()
        r = alg.solve_many_by_device_greedy.last_rounds
        print(f"traced {args.trace} (union_forward=True, union_prep={args.union_prep}): 3 batched solves of {len(layouts)} layouts, "
              f"rounds {r} (longest {max(r)})")
        return
    lines = []

    def say(s):
        print(s, flush=True)
        lines.append(s)
    say(f"union_prep_times: {torch.cuda.get_device_name(0)}, GPU_MAX_HW_QUEUES={os.environ.get('GPU_MAX_HW_QUEUES', 'unset')}, "
        f"{args.reps} interleaved repetitions, host clock around a device synchronise; baseline = union forward with every layout's "
        "graph prepared by its own call on a lane, candidate = the graphs of a round from one call on the current stream")
    for name in args.workloads.split(","):
        measure(name, args.reps, say)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
