"""Width-64 fp32 GIN MLP on the matrix cores (csrc/gin64_mlp.hip, tgnn_set_gin64_mfma) against the generic kernel it replaces:
(a) the op alone (ops.gin, kernel=None against kernel="mfma"), (b) the inference forward, (c) the training step (forward, loss,
backward; no optimizer) at width 64, depth 20 -- on the benchmark's layout (100 000 nodes, 1 M adjacency / 1.25 M collision
edges, 13 edge types) and on the labyrinth layout.  (b) and (c) run with tgnn_set_nnconv64_eg ON in both legs, so that the GIN
is what differs.  Same process, same device, the two settings interleaved, host clock around a device synchronise, medians with
the spread; per measurement the gate of DESIGN.md section 28: the new median below the generic one by more than the larger of
the two spreads (max - min).

The driver starts one child process per (layout, measurement), each under its own time limit, checks every exit status and
stops at the first failure.

    python scratch/gin64_mfma_times.py --out profiles/gin64_mfma_times.txt
    rocprofv3 --kernel-trace --stats --output-format csv -d DIR -o t -- python scratch/gin64_mfma_times.py --child bench profile
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


def child(name, what, reps, profile=False):
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
            prev_eg, prev = ops.set_nnconv64_eg(1), ops.set_gin64_mfma(on)
            try:
                fn()
            finally:
                ops.set_gin64_mfma(prev)
                ops.set_nnconv64_eg(prev_eg)
        return run

    def gate(ts_old, ts_new):
        m_old, m_new = statistics.median(ts_old), statistics.median(ts_new)
        worst = max(max(ts_old) - min(ts_old), max(ts_new) - min(ts_new))
        return (f"  gate: generic - new = {m_old - m_new:.3f} ms, larger spread {worst:.3f} ms: "
                f"{'PASS' if m_old - m_new > worst else 'FAIL'} ({m_old / m_new:.2f} x)")

    if what == "op":
        g = ops.prepare_graph(n, adj, attr, col)
        gen = torch.Generator().manual_seed(1)
        h = torch.randn(n, W, generator=gen).to(DEV)
        gin = net.brch_2_coll_conv_layers[1].ginConv
        ps = [gin.eps] + [p.detach() for p in gin._mlp_params()]
        part = ops.new_partials(W, DEV)
        reps_in = 10                                         # calls per timed window (the new op is two launches: gather, MLP)
        fns = [lambda: [ops.gin(h, g, *ps, act=ops.ACT_LEAKY_RELU, partials=part) for _ in range(reps_in)],
               lambda: [ops.gin(h, g, *ps, act=ops.ACT_LEAKY_RELU, partials=part, kernel="mfma") for _ in range(reps_in)]]
        if profile:                                          # for rocprofv3 --kernel-trace --stats: 40 calls of each, nothing else
            for fn in fns:
                for _ in range(4):
                    fn()
            torch.cuda.synchronize()
            return
        a, b = fns[0]()[0][0], fns[1]()[0][0]
        print(f"{head}: outputs differ by {float((a - b).abs().max() / a.abs().max()):.2e} of the max-norm; times per call, "
              f"{reps_in} calls per window")
        ts = interleaved(fns, reps)
        ts = [[t / reps_in for t in tt] for tt in ts]
        print(f"  generic kernel           {fmt(ts[0])}")
        print(f"  gather + gin64_mlp_kernel {fmt(ts[1])}")
        print(gate(ts[0], ts[1]))
        return
    if what == "forward":
        def fwd():
            with torch.no_grad():
                return net(x=x, adj_e_index=adj, adj_e_features=attr, col_e_idx=col)[0]
        fns = [with_switch(0, fwd), with_switch(1, fwd)]
        label = "inference forward (train-mode BatchNorm, graph cached, nnconv64_eg on)"
    else:
        net.autograd = True

        def step():
            net.zero_grad(set_to_none=True)
            probs, _ = net(x, adj, attr, col)
            loss, _, _ = Losses.calculate_unsupervised_loss(probs, x, col, adj, attr)
            loss.backward()
        fns = [with_switch(0, step), with_switch(1, step)]
        label = "training step (forward, loss, backward; nnconv64_eg on)"
    for fn in fns:                                           # warm up both settings (graph preparation, groups, code objects)
        fn()
        fn()
    ts = interleaved(fns, reps)
    print(f"{head}: {label}, width {W}, depth {DEPTH}")
    print(f"  switch off (generic kernel)  {fmt(ts[0])}")
    print(f"  switch on  (gin64_mlp_kernel) {fmt(ts[1])}")
    print(gate(ts[0], ts[1]))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--child", nargs=2, default=None, metavar=("LAYOUT", "WHAT"))
    ap.add_argument("--only", default=None, help="run only the measurements of this kind (op, forward, step)")
    args = ap.parse_args()
    if args.child:
        child(args.child[0], "op" if args.child[1] == "profile" else args.child[1], args.reps, profile=args.child[1] == "profile")
        return 0
    lines = [f"gin64_mfma_times: {args.reps} interleaved repetitions per setting, host clock around a device synchronise, "
             f"GPU_MAX_HW_QUEUES={os.environ.get('GPU_MAX_HW_QUEUES', 'unset')}"]
    print(lines[0], flush=True)
    rc = 0
    for name, what, limit in STEPS:
        if args.only and what != args.only:
            continue
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
