"""Training-step timings at network_width 32 and 64 (GPU box): forward keeping activations + loss + backward + Adam, and the
forward alone, on the labyrinth layout (1 254 nodes) and at config 3's shape (100 000 nodes, 1 M / 1.25 M edges, Fx = 5,
T = 13, depth 20).  One JSON line per (width, size).
  python scratch/train_width64.py                 all four
  python scratch/train_width64.py --steps 64 100000 3  three steps, nothing else (for rocprofv3 --kernel-trace --stats: the
                                                      first step also prepares the graph, both directions)
  python scratch/train_width64.py --summary STATS.csv STEPS   per-step kernel table of a rocprofv3 kernel_stats.csv"""
import argparse
import json
import os
import sys
import time

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from tests.golden_util import graph_tensors, load_labyrinth_graph  # noqa: E402
from tilingnn_amd import TilinGNN  # noqa: E402
from tilingnn_amd.solver.ml_solver.losses import Losses  # noqa: E402
from tilingnn_amd.synth import make_super_graph  # noqa: E402
from tilingnn_amd.weights import make_state_dict  # noqa: E402


def setup(width, n):
    if n == 1254:
        x, adj, attr, col, _ = graph_tensors(load_labyrinth_graph(), torch.float32, "cuda:0")
        fx = 3
    else:
        x, adj, attr, col, _ = make_super_graph(n, 10 * n, int(12.5 * n), tile_count=4, n_edge_types=13, seed=2).to_torch("cuda:0")
        fx = int(x.shape[1])
    fe = int(attr.shape[1])
    net = TilinGNN(adj_edge_features_dim=fe, network_depth=20, network_width=width, node_features_dim=fx)
    net.load_state_dict(make_state_dict(fe, 20, width, 1, fx, seed=0))
    net = net.cuda().train()
    net.cache_graph = True
    net.autograd = True
    opt = torch.optim.Adam(net.parameters(), lr=1e-4)

    def step():
        probs, _ = net(x, adj, attr, col)
        opt.zero_grad()
        loss, _, _ = Losses.calculate_unsupervised_loss(probs, x, col, adj, attr)
        loss.backward()
        opt.step()
        return loss

    def fwd():
        probs, _ = net(x, adj, attr, col)
        del probs
    return step, fwd


def timed(fn, reps):
    torch.cuda.synchronize()
    t = time.perf_counter()
    for _ in range(reps):
        fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t) / reps * 1e3


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", nargs=3, type=int, metavar=("WIDTH", "NODES", "STEPS"))
    ap.add_argument("--summary", nargs=2, metavar=("STATS_CSV", "STEPS"))
    args = ap.parse_args()
    if args.steps:
        step, _ = setup(*args.steps[:2])
        for _ in range(args.steps[2]):
            step()
        torch.cuda.synchronize()
        return
    if args.summary:
        import csv
        rows = list(csv.DictReader(open(args.summary[0])))
        k = int(args.summary[1])
        tot = sum(float(r["TotalDurationNs"]) for r in rows)
        print(f"{'kernel'[:90]:90s} {'calls/step':>10s} {'avg_us':>9s} {'us/step':>10s} {'pct':>6s}")
        for r in rows:
            print(f"{r['Name'][:90]:90s} {int(r['Calls']) / k:10.2f} {float(r['AverageNs']) / 1e3:9.1f} "
                  f"{float(r['TotalDurationNs']) / 1e3 / k:10.1f} {float(r['Percentage']):6.2f}")
        print(f"kernel time per step (sum over kernels / {k}): {tot / 1e6 / k:.2f} ms")
        return
    for n in (1254, 100_000):
        for width in (32, 64):
            step, fwd = setup(width, n)
            reps = 20 if n == 1254 else 5
            for _ in range(2):
                step()
            ms = timed(step, reps)
            for _ in range(2):
                fwd()
            fwd_ms = timed(fwd, reps)
            loss = float(step().detach())
            print(json.dumps({"width": width, "nodes": n, "train_step_ms": round(ms, 3), "forward_keeping_ms": round(fwd_ms, 3),
                              "forward_share": round(fwd_ms / ms, 3), "loss": loss,
                              "peak_mem_GB": round(torch.cuda.max_memory_allocated() / 2 ** 30, 2)}), flush=True)
            del step, fwd
            torch.cuda.empty_cache()
            torch.cuda.reset_peak_memory_stats()


if __name__ == "__main__":
    main()
