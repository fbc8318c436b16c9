"""Width-64 fp32 NNConv on edge groups (csrc/nnconv64_eg.hip, tgnn_set_nnconv64_eg) against the generic kernel it replaces:
(a) the op alone, (b) the inference forward, (c) the training step (forward, loss, backward) at width 64, depth 20 -- on the
benchmark's layout (100 000 nodes, 1 M adjacency / 1.25 M collision edges, 13 edge types) and on the labyrinth layout.  Same
process, same device, the two settings interleaved, host clock around a device synchronise, medians with the spread.

The driver starts one child process per (layout, measurement), each under its own time limit, checks every exit status and
stops at the first failure.

    python scratch/nnconv64_eg_times.py --out profiles/nnconv64_eg_times.txt
"""
import argparse
import os
import statistics
import subprocess
import sys
import time

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)
DEV = "cuda:0"
W, DEPTH = 64, 20
STEPS = [("bench", "op", 240), ("bench", "forward", 300), ("bench", "step", 420),
         ("labyrinth", "op", 180), ("labyrinth", "forward", 180), ("labyrinth", "step", 240)]


def sync_ms(fn):
    import torch
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
    return f"median {m:9.3f} ms  ({min(ts):.3f} - {max(ts):.3f}, spread {(max(ts) - min(ts)) / m:.3f})"


def layout(name):
    import torch
    if name == "bench":
        from tilingnn_amd.synth import make_super_graph
        sg = make_super_graph(100_000, 1_000_000, 1_250_000, tile_count=2, n_edge_types=13, seed=1)
        x, adj, attr, col, _ = sg.to_torch(DEV)
        return x, adj, attr, col
    from tests.golden_util import graph_tensors, load_labyrinth_graph
    return graph_tensors(load_labyrinth_graph(), torch.float32, DEV)[:4]


def child(name, what, reps):
    import torch
    from tilingnn_amd import ops, train
    from tilingnn_amd.graph_networks.networks.TilinGNN import TilinGNN
    from tilingnn_amd.solver.ml_solver.losses import Losses
    from tilingnn_amd.weights import make_state_dict
    x, adj, attr, col = layout(name)
    n, fe = int(x.shape[0]), int(attr.shape[1])
    head = f"{name} ({n} nodes, {int(adj.shape[1])} / {int(col.shape[1])} edges), {what}"
    net = TilinGNN(adj_edge_features_dim=fe, network_depth=DEPTH, network_width=W, node_features_dim=int(x.shape[1]))
    net.load_state_dict(make_state_dict(fe, DEPTH, W, 1, int(x.shape[1]), seed=0))
    net = net.to(DEV).train()

    def with_switch(on, fn):
        def run():
            prev = ops.set_nnconv64_eg(on)
            try:
                fn()
            finally:
                ops.set_nnconv64_eg(prev)
        return run

    if what == "op":
        g = ops.prepare_graph(n, adj, attr, col, groups=True)
        gen = torch.Generator().manual_seed(1)
        h = torch.randn(n, W, generator=gen).to(DEV)
        wtab = torch.rand(g.n_types, W, W, generator=gen).to(DEV)
        root, bias = (torch.randn(W, W, generator=gen) * 0.3).to(DEV), torch.randn(W, generator=gen).to(DEV)
        part = ops.new_partials(W, DEV)
        reps_in = 10                                         # launches per timed window (the op includes its bound and image launches)
        fns = [lambda: [ops.nnconv_mean(h, g, wtab, root, bias, ops.ACT_LEAKY_RELU, part) for _ in range(reps_in)],
               lambda: [ops.nnconv_mean(h, g, wtab, root, bias, ops.ACT_LEAKY_RELU, part, kernel="eg") for _ in range(reps_in)]]
        a, b = fns[0]()[0][0], fns[1]()[0][0]
        print(f"{head}: T {g.n_types}, max in-degree {g.max_in_degree}; outputs differ by "
              f"{float((a - b).abs().max() / a.abs().max()):.2e} of the max-norm; times per call, {reps_in} calls per window")
        ts = interleaved(fns, reps)
        print(f"  generic kernel        {fmt([t / reps_in for t in ts[0]])}")
        print(f"  nnconv64_eg (+ bound, image) {fmt([t / reps_in for t in ts[1]])}")
        return
    if what == "forward":
        def fwd():
            with torch.no_grad():
                return net(x=x, adj_e_index=adj, adj_e_features=attr, col_e_idx=col)[0]
        fns = [with_switch(0, fwd), with_switch(1, fwd)]
        label = "inference forward (train-mode BatchNorm, graph cached)"
    else:
        net.autograd = True

        def step():
            net.zero_grad(set_to_none=True)
            probs, _ = net(x, adj, attr, col)
            loss, _, _ = Losses.calculate_unsupervised_loss(probs, x, col, adj, attr)
            loss.backward()
        fns = [with_switch(0, step), with_switch(1, step)]
        label = "training step (forward, loss, backward)"
    for fn in fns:                                           # warm up both settings (graph preparation, groups, code objects)
        fn()
        fn()
    ts = interleaved(fns, reps)
    print(f"{head}: {label}, width {W}, depth {DEPTH}")
    print(f"  switch off (generic kernel) {fmt(ts[0])}")
    print(f"  switch on  (nnconv64_eg)    {fmt(ts[1])}")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--child", nargs=2, default=None, metavar=("LAYOUT", "WHAT"))
    args = ap.parse_args()
    if args.child:
        child(args.child[0], args.child[1], args.reps)
        return 0
    lines = [f"nnconv64_eg_times: {args.reps} interleaved repetitions per setting, host clock around a device synchronise, "
             f"GPU_MAX_HW_QUEUES={os.environ.get('GPU_MAX_HW_QUEUES', 'unset')}"]
    print(lines[0], flush=True)
    rc = 0
    for name, what, limit in STEPS:
        run = subprocess.run(["timeout", "-k", "10", str(limit), sys.executable, os.path.abspath(__file__), "--reps", str(args.reps),
                              "--child", name, what], capture_output=True, text=True, cwd=REPO)
        print(run.stdout, end="", flush=True)
        lines += run.stdout.splitlines()
        if run.returncode != 0:
            msg = f"STOPPED: {name} {what} ended with status {run.returncode}"
            print(msg + "\n" + run.stderr[-3000:], flush=True)
            lines.append(msg)
            rc = 1
            break
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write("\n".join(lines) + "\n")
    return rc


if __name__ == "__main__":
    sys.exit(main())
