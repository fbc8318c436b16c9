"""Mini-batch training (Trainer.train_batches, ops.batch_union) against Trainer.train: 256 training layouts (+ 8 test layouts) written
by Trainer.create_data on the ring-9 graph, one process, warmed up, alternatives interleaved, host clock around a device
synchronise.

  steps of an epoch   the 256 layouts once through train_step (graphs cached: what Trainer.train runs) against the same layouts
                      through train_batch_step in chunks of B = 1, 8, 32 (a fixed permutation)
  whole epochs        Trainer.train / Trainer.train_batches(B) through their public entry, 4 epochs each, the first dropped:
                      steps + both evaluations + the checkpoint of an improved test loss
  one B = 32 step     where its time goes: union, graph preparation, the transposed CSRs of TrainGraph, the rest
  union build         tgnn_batch_union for B = 32 against torch.cat + offset adds for the same members

    python scratch/batch_training_times.py --out profiles/batch_training_times.txt
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

import numpy as np
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


def cat_union(layouts, ids):
    """The union without the kernel: 4 torch.cat over B operands + the offset adds."""
    from tilingnn_amd.util.algorithms import DeviceLayout
    first, adjs, cols = 0, [], []
    for i in ids:
        l = layouts[i]
        adjs.append(l.align_edge_index + first)
        cols.append(l.collide_edge_index + first)
        first += int(l.node_feature.shape[0])
    return DeviceLayout(torch.cat([layouts[i].node_feature for i in ids]), torch.cat(adjs, 1),
                        torch.cat([layouts[i].align_edge_features for i in ids]), torch.cat(cols, 1))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--layouts", type=int, default=256)
    args = ap.parse_args()
    from tilingnn_amd import ops, train
    from tilingnn_amd.graph_networks.networks.TilinGNN import TilinGNN
    from tilingnn_amd.solver.ml_solver.trainer import LayoutDataset, Trainer, batch_chunks
    from tilingnn_amd.tiling.tile_graph import TileGraph
    from tilingnn_amd.weights import make_state_dict
    lines = []

    def say(s):
        print(s, flush=True)
        lines.append(s)

    work = tempfile.mkdtemp(prefix="batch_times_")
    path = os.path.join(work, "ring9.pkl")
    with gzip.open(os.path.join(REPO, "tests", "golden", "complete_graph_ring9.pkl.gz"), "rb") as src, open(path, "wb") as dst:
        shutil.copyfileobj(src, dst)
    graph = TileGraph(2)
    graph.load_graph_state(path, sidecar=False)

    def fresh():
        net = TilinGNN(adj_edge_features_dim=15, network_depth=20, network_width=32, node_features_dim=3)
        net.load_state_dict(make_state_dict(15, 20, 32, 1, 3, seed=0))
        net = net.to(DEV).train()
        return net, torch.optim.Adam(net.parameters(), lr=1e-3)

    net, opt = fresh()
    data = os.path.join(work, "data")
    trainer = Trainer(None, None, DEV, net, data)
    t0 = time.perf_counter()
    trainer.create_data(graph, number_of_data=args.layouts, testing_ratio=8 / args.layouts, rng=random.Random(0))
    train_set = LayoutDataset(trainer.training_path, DEV)
    packed = train_set.packed
    sizes = [packed.nodes(k) for k in range(packed.k)]
    say(f"batch_training_times: {torch.cuda.get_device_name(0)}, GPU_MAX_HW_QUEUES={os.environ.get('GPU_MAX_HW_QUEUES', 'unset')}, "
        f"{args.reps} interleaved repetitions, host clock around a device synchronise; width 32, depth 20, Adam")
    say(f"data: {len(train_set)} training layouts of create_data on the ring-9 graph ({time.perf_counter() - t0:.1f} s to write and load), "
        f"{min(sizes)}..{max(sizes)} nodes (median {int(statistics.median(sizes))}, {sum(sizes)} in all), {packed.ea} adjacency and "
        f"{packed.ec} collision edges in all")

    # ---- the steps of one epoch
    order = np.random.default_rng(1).permutation(len(train_set))

    def singles():
        for i in order:
            trainer.train_step(train_set[int(i)], opt)

    def batches(b):
        def run():
            for ids in batch_chunks(order, b):
                trainer.train_batch_step(packed, ids, opt)
        return run
    fns = [singles, batches(1), batches(8), batches(32)]
    names = ["Trainer.train's steps (train_step per layout, graphs cached)", "train_batch_step, B =  1", "train_batch_step, B =  8",
             "train_batch_step, B = 32"]
    net.autograd = True
    for fn in fns:                                                  # warm-up: every shape once, the graph cache filled
        fn()
    ts = interleaved(fns, args.reps)
    say(f"steps of one epoch over the {len(train_set)} layouts:")
    for name, t, b in zip(names, ts, (1, 1, 8, 32)):
        steps = len(batch_chunks(order, b))
        say(f"  {name:62s} {fmt(t)}  = {statistics.median(t) / steps:8.3f} ms per step, {steps} steps")
    say(f"  ratio to Trainer.train's steps: B = 1 {statistics.median(ts[0]) / statistics.median(ts[1]):.2f}x, "
        f"B = 8 {statistics.median(ts[0]) / statistics.median(ts[2]):.2f}x, B = 32 {statistics.median(ts[0]) / statistics.median(ts[3]):.2f}x")

    # ---- one B = 32 step, by phase
    ids32 = batch_chunks(order, 32)[0]
    box = {}

    def p_union():
        box["lay"] = ops.batch_union(packed, ids32)

    def p_prep():
        l = box["lay"]
        box["g"] = ops.prepare_graph(int(l.node_feature.shape[0]), l.align_edge_index, l.align_edge_features, l.collide_edge_index)

    def p_tg():
        l = box["lay"]
        box["tg"] = train.TrainGraph(box["g"], l.align_edge_index, l.collide_edge_index)

    def p_step():
        trainer.train_batch_step(packed, ids32, opt)
    phases = [p_union, p_prep, p_tg, p_step]
    for fn in phases:
        fn()
    tp = interleaved(phases, max(args.reps, 10))
    l = box["lay"]
    say(f"one step on a union of 32 ({int(l.node_feature.shape[0])} nodes, {int(l.align_edge_index.shape[1])} adjacency, "
        f"{int(l.collide_edge_index.shape[1])} collision edges, {box['g'].n_types} edge types):")
    for name, t in zip(["batch_union", "prepare_graph (cache bypassed)", "TrainGraph (transposed CSRs, degrees)",
                        "the whole train_batch_step (all of the above + forward, loss, backward, Adam)"], tp):
        say(f"  {name:82s} {fmt(t)}")
    net.autograd = False

    # ---- the union: the kernel against torch.cat
    a, b = ops.batch_union(packed, ids32), cat_union(train_set.layouts, ids32)
    same = all(torch.equal(u, v) for u, v in ((a.node_feature, b.node_feature), (a.align_edge_index, b.align_edge_index),
                                              (a.align_edge_features, b.align_edge_features), (a.collide_edge_index, b.collide_edge_index)))
    say(f"union of 32 members, 20 calls per repetition (outputs equal to the torch.cat union: {same}):")
    loop = lambda fn: (lambda: [fn() for _ in range(20)])
    tu = interleaved([loop(lambda: ops.batch_union(packed, ids32)), loop(lambda: cat_union(train_set.layouts, ids32))], max(args.reps, 10))
    bytes_moved = 2 * (a.node_feature.numel() * 4 + a.align_edge_features.numel() * 4 + a.align_edge_index.numel() * 8 + a.collide_edge_index.numel() * 8)
    for name, t in zip(["ops.batch_union (one copy of the table, one launch)", "torch.cat x 4 + 2 B offset adds"], tu):
        say(f"  {name:62s} {fmt(t)}  = {statistics.median(t) / 20 * 1e3:8.1f} us per union")
    say(f"  ratio {statistics.median(tu[1]) / statistics.median(tu[0]):.2f}x; the union reads + writes {bytes_moved / 1e6:.2f} MB")

    # ---- whole epochs through the public entries
    say("whole epochs (steps + the evaluation of both splits + checkpoint), 4 epochs each, the first dropped:")

    def epochs(run):
        stamps = []

        def log(msg):
            if msg.startswith("Training Start") or "testing loss" in msg:
                torch.cuda.synchronize()
                stamps.append(time.perf_counter())
        run(log)
        return [(b_ - a_) * 1e3 for a_, b_ in zip(stamps[1:-1], stamps[2:])]
    for name, b in (("Trainer.train", 0), ("Trainer.train_batches, B =  1", 1), ("Trainer.train_batches, B =  8", 8),
                    ("Trainer.train_batches, B = 32", 32)):
        net_b, opt_b = fresh()
        tr = Trainer(None, None, DEV, net_b, data, model_save_path=os.path.join(work, f"model_{b}"))
        if b == 0:
            t = epochs(lambda log: tr.train(None, opt_b, training_epoch=4, save_model_per_epoch=1000, shuffle_seed=1, log=log))
        else:
            t = epochs(lambda log: tr.train_batches(None, opt_b, batch_size=b, training_epoch=4, save_model_per_epoch=1000,
                                                    shuffle_seed=1, log=log))
        say(f"  {name:62s} {fmt(t)}")
    shutil.rmtree(work, ignore_errors=True)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
