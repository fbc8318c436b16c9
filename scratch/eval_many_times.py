"""Evaluating a split: `cal_avg_loss` (one layout at a time: forward, three launches of loss, two blocking copies) against
`cal_avg_loss_many` (groups of 8 and 32: forward_many, one health poll and one tgnn_unsupervised_loss_many per group, one
read-back per split), union forward off and on; 256 layouts written by Trainer.create_data on the ring-9 graph, one process,
graphs cached, warmed up, alternatives interleaved, host clock around a device synchronise.  Then the loss alone: 32 solo
`Losses.unsupervised_losses` calls (queued, no read-back) against one `unsupervised_losses_many` at K = 32.

    python scratch/eval_many_times.py --out profiles/eval_many_times.txt
"""
import argparse
import gzip
import os
import random
import shutil
import statistics
import sys
import tempfile
import time

import torch

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)
DEV = "cuda:0"


def sync_ms(fn):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) * 1e3


def interleaved(fns, reps):
    out = [[] for _ in fns]
    for _ in range(reps):
        for k, fn in enumerate(fns):
            out[k].append(sync_ms(fn))
    return out


def fmt(ts):
    m = statistics.median(ts)
    return f"median {m:10.3f} ms  ({min(ts):.3f} - {max(ts):.3f}, spread {(max(ts) - min(ts)) / m:.3f})"


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--layouts", type=int, default=256)
    args = ap.parse_args()
    from tilingnn_amd.graph_networks.networks.TilinGNN import TilinGNN
    from tilingnn_amd.solver.ml_solver.losses import Losses
    from tilingnn_amd.solver.ml_solver.trainer import LayoutDataset, Trainer, cal_avg_loss, cal_avg_loss_many
    from tilingnn_amd.tiling.tile_graph import TileGraph
    from tilingnn_amd.weights import make_state_dict
    lines = []

    def say(s):
        print(s, flush=True)
        lines.append(s)

    work = tempfile.mkdtemp(prefix="eval_times_")
    path = os.path.join(work, "ring9.pkl")
    with gzip.open(os.path.join(REPO, "tests", "golden", "complete_graph_ring9.pkl.gz"), "rb") as src, open(path, "wb") as dst:
        shutil.copyfileobj(src, dst)
    graph = TileGraph(2)
    graph.load_graph_state(path, sidecar=False)
    net = TilinGNN(adj_edge_features_dim=15, network_depth=20, network_width=32, node_features_dim=3)
    net.load_state_dict(make_state_dict(15, 20, 32, 1, 3, seed=0))
    net = net.to(DEV).train()
    trainer = Trainer(None, None, DEV, net, os.path.join(work, "data"))
    t0 = time.perf_counter()
    trainer.create_data(graph, number_of_data=args.layouts, testing_ratio=0.0, rng=random.Random(0))
    split = LayoutDataset(trainer.training_path, DEV)
    packed = split.packed
    sizes = [packed.nodes(k) for k in range(packed.k)]
    say(f"eval_many_times: {torch.cuda.get_device_name(0)}, GPU_MAX_HW_QUEUES={os.environ.get('GPU_MAX_HW_QUEUES', 'unset')}, "
        f"{args.reps} interleaved repetitions, host clock around a device synchronise; width 32, depth 20, train mode")
    say(f"split: {len(split)} layouts of create_data on the ring-9 graph ({time.perf_counter() - t0:.1f} s to write and load), "
        f"{min(sizes)}..{max(sizes)} nodes (median {int(statistics.median(sizes))}, {sum(sizes)} in all), {packed.ea} adjacency and "
        f"{packed.ec} collision edges in all")

    # ---- the split
    box = {}
    variants = [("cal_avg_loss (one layout at a time)", lambda: cal_avg_loss(net, split))]
    for group in (8, 32):
        for union in (False, True):
            variants.append((f"cal_avg_loss_many, group {group:2d}, union {'on ' if union else 'off'}",
                             (lambda g, u: lambda: cal_avg_loss_many(net, split, group=g, union=u))(group, union)))
    results = []
    for name, fn in variants:                                       # warm-up: every graph prepared and cached, every shape once
        results.append(fn())
    same = all(r == results[0] for r in results)
    say(f"mean loss of the split {results[0]!r}; the five variants return the same float: {same}")
    ts = interleaved([fn for _, fn in variants], args.reps)
    say(f"one evaluation of the split ({len(split)} layouts):")
    base = statistics.median(ts[0])
    for (name, _), t in zip(variants, ts):
        m = statistics.median(t)
        say(f"  {name:48s} {fmt(t)}  = {m / len(split) * 1e3:8.1f} us per layout, {base / m:5.2f}x")

    # ---- the loss alone, K = 32
    ids = list(range(32))
    with torch.no_grad():
        probs = net.forward_many([(l.node_feature, l.align_edge_index, l.align_edge_features, l.collide_edge_index)
                                  for l in split.layouts[:32]])
    torch.cuda.synchronize()

    def solo():
        box["solo"] = [Losses.unsupervised_losses(p, l.node_feature, l.collide_edge_index, l.align_edge_index, l.align_edge_features)
                       for p, l in zip(probs, split.layouts[:32])]

    def many():
        box["many"] = Losses.unsupervised_losses_many(probs, packed, first=0, count=32)

    def solo_read():
        for p, l in zip(probs, split.layouts[:32]):
            Losses.calculate_unsupervised_loss(p, l.node_feature, l.collide_edge_index, l.align_edge_index, l.align_edge_features)

    def many_read():
        buf, lo, te, er = Losses.many_outputs(32, 1, DEV)
        Losses.unsupervised_losses_many(probs, packed, first=0, count=32, out=(lo, te, er))
        Losses.results_many(*Losses.read_back_many(buf, 32, 1))
    fns = [solo, many, solo_read, many_read]
    for fn in fns:
        fn()
    equal = all(torch.equal(box["many"][0][k], box["solo"][k][0]) and torch.equal(box["many"][1][k], box["solo"][k][1]) for k in ids)
    tl = interleaved([(lambda f: lambda: [f() for _ in range(10)])(fn) for fn in fns], max(args.reps, 10))
    say(f"the loss of 32 layouts, 10 calls per repetition (batched rows equal to the solo calls': {equal}):")
    for name, t in zip(["32 x Losses.unsupervised_losses, queued only", "1 x unsupervised_losses_many (K = 32), queued only",
                        "32 x calculate_unsupervised_loss (2 blocking copies each)",
                        "1 x unsupervised_losses_many + read_back_many + results_many"], tl):
        say(f"  {name:62s} {fmt(t)}  = {statistics.median(t) / 10 * 1e3:8.1f} us per 32 layouts")
    say(f"  ratio queued only {statistics.median(tl[0]) / statistics.median(tl[1]):.2f}x, with the read-back "
        f"{statistics.median(tl[2]) / statistics.median(tl[3]):.2f}x")
    shutil.rmtree(work, ignore_errors=True)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
