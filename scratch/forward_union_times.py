"""forward_many / solve_many with the small layouts inside ONE persistent kernel launch (union=True / ML_Solver.union_forward = True) against
the default path (every layout its own kernel on one of three lanes), same layouts, same seed, one process, warmed up, A/B
interleaved.  Workloads: those of scratch/solve_many_times.py (12 bunny crops, the 24 crops of the README's example, 32 synthetic
layouts of 1 000 nodes).

    python scratch/forward_union_times.py --out profiles/forward_union_times.txt      (times)
    python scratch/forward_union_times.py --trace bunny [--union]                     (three batched solves, for rocprofv3 --kernel-trace --stats)
    python scratch/forward_union_times.py --summarise a_kernel_trace.csv b_kernel_trace.csv   (launches by kernel name)
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
from solve_many_times import DEV, WORKLOADS, solver, timed  # noqa: E402


def ab(base_fn, cand_fn, reps):
    base, cand = [], []
    for _ in range(reps):                                        # A/B interleaved
        base.append(timed(base_fn)[0])
        cand.append(timed(cand_fn)[0])
    return base, cand


def report(say, what, base, cand):
    mb, mc = statistics.median(base), statistics.median(cand)
    spread = (max(base) - min(base)) / mb
    gain = (mb - mc) / mb
    say(f"  {what}")
    say(f"    default            : median {mb:9.3f} ms  ({min(base):.3f} - {max(base):.3f})  relative spread {spread:.3f}")
    say(f"    union              : median {mc:9.3f} ms  ({min(cand):.3f} - {max(cand):.3f})")
    say(f"    ratio {mb / mc:.2f}x; gain {gain:.3f} of the default against 3 x spread = {3 * spread:.3f}: "
        f"{'a gain beyond the noise margin' if gain > 3 * spread else 'NOT beyond the noise margin'}")


def measure(name, reps, say):
    from tilingnn_amd import _lib
    from tilingnn_amd.util import algorithms as alg
    from tilingnn_amd.util.algorithms import PackedLayouts
    graph, layouts = WORKLOADS[name]()
    ms = solver(graph)
    net = ms.network
    pk = PackedLayouts(layouts, DEV)
    views = [pk.layout(k) for k in range(pk.k)]
    args = [(v.node_feature, v.align_edge_index, v.align_edge_features, v.collide_edge_index) for v in views]
    sizes = [int(a[0].shape[0]) for a in args]
    fwd = lambda: net.forward_many(args)
    fwd_u = lambda: net.forward_many(args, union=True)
    many = lambda: alg.solve_many_by_device_greedy(ms, layouts, seed=0)
    def with_union(fn):
        def run():
            ms.union_forward = True
            try:
                return fn()
            finally:
                ms.union_forward = False
        return run
    many_u = with_union(many)
    before = _lib.forward_union_counts()
    for _ in range(2):                                           # warm-up: allocator, graph cache, stream measurement
        a, b = fwd(), fwd_u()
        want, got = many(), many_u()
    torch.cuda.synchronize()
    assert all(torch.equal(x, y) for x, y in zip(a, b))
    assert all(np.array_equal(x[0], y[0]) and x[1] == y[1] and x[2] == y[2] for x, y in zip(want, got))
    rounds = alg.solve_many_by_device_greedy.last_rounds
    c0 = _lib.forward_union_counts()
    fwd_u()
    c1 = _lib.forward_union_counts()
    say(f"{name}: {len(layouts)} layouts, {min(sizes)}..{max(sizes)} nodes ({sum(sizes)} in all), rounds {min(rounds)}..{max(rounds)}; "
        f"first round: {c1[1] - c0[1]} layouts in {c1[0] - c0[0]} union launch(es); union launches so far {c1[0] - before[0]}")
    report(say, "forward_many on the first-round layouts", *ab(fwd, fwd_u, reps))
    report(say, "solve_many (the whole greedy loop)", *ab(many, many_u, reps))


def summarise(paths, say):
    """rocprofv3 --kernel-trace csv files -> calls, total and average time by kernel name"""
    import csv
    for path in paths:
        by = {}
        for r in csv.DictReader(open(path)):
            c = by.setdefault(r["Kernel_Name"], [0, 0.0])
            c[0] += 1
            c[1] += (int(r["End_Timestamp"]) - int(r["Start_Timestamp"])) / 1e3
        total = sum(v[1] for v in by.values())
        say(f"{os.path.basename(os.path.dirname(path)) or path}: {sum(v[0] for v in by.values())} launches, {total:.1f} us of kernel time")
        say("  calls     total us     avg us   share  kernel")
        for name, (calls, us) in sorted(by.items(), key=lambda kv: -kv[1][1]):
            say(f"  {calls:5d}  {us:11.1f}  {us / calls:9.2f}  {us / total:6.3f}  {name[:110]}")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--workloads", default="bunny,readme,synth32")
    ap.add_argument("--trace", default=None, help="run three batched solves of this workload after a warm-up and exit")
    ap.add_argument("--union", action="store_true", help="--trace: with ML_Solver.union_forward = True")
    ap.add_argument("--summarise", nargs="+", default=None, help="kernel-trace csv files of --trace runs: the table by kernel name")
    args = ap.parse_args()
    if args.summarise:
        summarise(args.summarise, print)
        return
    if args.trace:
        from tilingnn_amd.util import algorithms as alg
        graph, layouts = WORKLOADS[args.trace]()
        ms = solver(graph)
        ms.union_forward = args.union
        for _ in range(3):
            alg.solve_many_by_device_greedy(ms, layouts, seed=0)
        torch.cuda.synchronize()
        r = alg.solve_many_by_device_greedy.last_rounds
        print(f"traced {args.trace} (union_forward={args.union}): 3 batched solves of {len(layouts)} layouts, rounds {r} (longest {max(r)})")
        return
    lines = []

    def say(s):
        print(s, flush=True)
        lines.append(s)
    say(f"forward_union_times: {torch.cuda.get_device_name(0)}, GPU_MAX_HW_QUEUES={os.environ.get('GPU_MAX_HW_QUEUES', 'unset')}, "
        f"{args.reps} interleaved repetitions, host clock around a device synchronise; default = every layout its own persistent "
        "kernel on one of three lanes, union = one persistent launch per group on the current stream")
    for name in args.workloads.split(","):
        measure(name, args.reps, say)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
