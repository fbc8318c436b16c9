"""The fused adjoint of GINConv's MLP at width 64 (csrc/mlp_bwd.hip: mlp_bwd_tall64_kernel, tgnn_set_mlp_bwd_tall64) against the chain
of generic kernels it replaces (tgnn_sigmoid_mlp_bwd): (a) the op alone (64 -> 32 -> 64 -> 64 over the layout's rows), (b) the
training step without the optimizer (forward, loss, backward) at width 64, depth 20, with set_nnconv64_eg(1) and set_gin64_mfma(1)
on in both settings -- on the labyrinth layout (1 254 nodes) and on the benchmark's layout (100 000 nodes, 1 M adjacency / 1.25 M
collision edges, 13 edge types).  Per measurement both settings run in the same process, interleaved, host clock around a device
synchronise, medians with the spread, and the gate of DESIGN.md section 28: the new median below the old one by more than the
larger of the two spreads (max - min).

The driver starts one child process per (layout, measurement), each under its own time limit, checks every exit status and
stops at the first failure.

    python scratch/mlp_bwd_tall64_times.py --out profiles/mlp_bwd_tall64_times.txt
    rocprofv3 --kernel-trace --stats --output-format csv -d DIR -o t -- python scratch/mlp_bwd_tall64_times.py --child bench profile0
    (profile0 / profile1: THREE training steps with the switch off / on, nothing else)
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
STEPS = [("labyrinth", "op", 180), ("labyrinth", "step", 240), ("bench", "op", 240), ("bench", "step", 420)]


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
    return f"median {m:9.4f} ms  ({min(ts):.4f} - {max(ts):.4f}, spread {(max(ts) - min(ts)) / m:.3f})"


def gate(ts_old, ts_new):
    m_old, m_new = statistics.median(ts_old), statistics.median(ts_new)
    worst = max(max(ts_old) - min(ts_old), max(ts_new) - min(ts_new))
    return (f"  gate: chain - tall64 = {m_old - m_new:.4f} ms, larger spread {worst:.4f} ms: "
            f"{'PASS' if m_old - m_new > worst else 'FAIL'} ({m_old / m_new:.2f} x)")


def layout(name):
    import torch
    if name == "bench":
        from tilingnn_amd.synth import make_super_graph
        sg = make_super_graph(100_000, 1_000_000, 1_250_000, tile_count=2, n_edge_types=13, seed=1)
        x, adj, attr, col, _ = sg.to_torch(DEV)
        return x, adj, attr, col
    from tests.golden_util import graph_tensors, load_labyrinth_graph
    return graph_tensors(load_labyrinth_graph(), torch.float32, DEV)[:4]


def op_inputs(n, d0, d3, seed):
    import torch
    g = torch.Generator().manual_seed(seed)
    r = lambda *s: torch.randn(*s, generator=g)
    x = r(n, d0)
    w = [r(32, d0) * (2.0 / d0 ** 0.5), 0.5 * r(32), r(64, 32) * (2.0 / 32 ** 0.5), 0.5 * r(64), r(d3, 64) * 0.25, 0.5 * r(d3)]
    t3 = torch.sigmoid(torch.sigmoid(torch.sigmoid(x @ w[0].t() + w[1]) @ w[2].t() + w[3]) @ w[4].t() + w[5])
    return [v.to(DEV) for v in (x, t3, r(n, d3))], [v.to(DEV) for v in w]


def child(name, what, reps):
    import torch
    from tilingnn_amd import train
    from tilingnn_amd.graph_networks.networks.TilinGNN import TilinGNN
    from tilingnn_amd.solver.ml_solver.losses import Losses
    from tilingnn_amd.weights import make_state_dict
    x, adj, attr, col = layout(name)
    n, fe = int(x.shape[0]), int(attr.shape[1])
    head = f"{name} ({n} nodes, {int(adj.shape[1])} / {int(col.shape[1])} edges)"
    names = [f"mlp.{k}" for k in range(3)]

    if what == "op":
        reps_in = 10                                         # calls per timed window
        cases = [(f"tall64 op, {n} rows of 64 -> 32 -> 64 -> 64", op_inputs(n, 64, 64, 1), True)]
        for label, ((xx, t3, d_out), w), need_dx in cases:
            fns = [lambda k=k: [train.sigmoid_mlp_backward(w, xx, t3, d_out, {}, names, need_dx, kernel=k) for _ in range(reps_in)]
                   for k in ("chain", "tall64")]
            for fn in fns:
                fn()
            ts = [[t / reps_in for t in tt] for tt in interleaved(fns, reps)]
            print(f"{head}: {label}; times per call, {reps_in} calls per window")
            print(f"  chain  (tgnn_sigmoid_mlp_bwd)        {fmt(ts[0])}")
            print(f"  tall64 (tgnn_sigmoid_mlp_bwd_tall64) {fmt(ts[1])}")
            print(gate(ts[0], ts[1]))
        return

    from tilingnn_amd import ops
    ops.set_nnconv64_eg(1)                                   # the two forward switches: on in both settings
    ops.set_gin64_mfma(1)
    net = TilinGNN(adj_edge_features_dim=fe, network_depth=DEPTH, network_width=W, node_features_dim=int(x.shape[1]))
    net.load_state_dict(make_state_dict(fe, DEPTH, W, 1, int(x.shape[1]), seed=0))
    net = net.to(DEV).train()
    net.autograd = True

    def step():
        net.zero_grad(set_to_none=True)
        probs, _ = net(x, adj, attr, col)
        loss, _, _ = Losses.calculate_unsupervised_loss(probs, x, col, adj, attr)
        loss.backward()

    def with_switch(on):
        def run():
            prev = train.set_mlp_bwd_tall64(on)
            try:
                step()
            finally:
                train.set_mlp_bwd_tall64(prev)
        return run

    if what in ("profile0", "profile1"):                     # for rocprofv3 --kernel-trace --stats: three steps of one setting
        run = with_switch(int(what[-1]))
        for _ in range(3):
            run()
        torch.cuda.synchronize()
        return
    fns = [with_switch(0), with_switch(1)]
    for fn in fns:                                           # warm up both settings (graph preparation, code objects)
        fn()
        fn()
    ts = interleaved(fns, reps)
    print(f"{head}: training step (forward, loss, backward; no optimizer), width {W}, depth {DEPTH}, nnconv64_eg and gin64_mfma on")
    print(f"  switch off (the chain)              {fmt(ts[0])}")
    print(f"  switch on  (mlp_bwd_tall64_kernel)  {fmt(ts[1])}")
    print(gate(ts[0], ts[1]))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--child", nargs=2, default=None, metavar=("LAYOUT", "WHAT"))
    ap.add_argument("--only", default=None, help="run only the measurements of this kind (op, step)")
    args = ap.parse_args()
    if args.child:
        child(args.child[0], args.child[1], args.reps)
        return 0
    lines = [f"mlp_bwd_tall64_times: {args.reps} interleaved repetitions per setting, host clock around a device synchronise, "
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
