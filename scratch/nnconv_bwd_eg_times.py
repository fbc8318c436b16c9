"""The NNConv adjoint on edge groups (csrc/nnconv_bwd_eg.hip, tgnn_set_nnconv_bwd_eg) against the chain it replaces (type sums S' over
the transposed CSR, two layout swaps, one dense product, one weight-gradient product, a third swap): (a) the op alone
(train.nnconv_backward, kernel="chain" against kernel="eg": dh, d root, d bias and the edge MLP's adjoint, which both routes share),
(b) the training step without the optimizer (forward, loss, backward) at depth 20 with the four older switches on in both settings
(set_nnconv64_eg, set_gin64_mfma, set_mlp_bwd_fused, set_mlp_bwd_tall64) -- at widths 32 and 64, on the labyrinth layout (1 254
nodes) and on the benchmark's layout (100 000 nodes, 1 M adjacency / 1.25 M collision edges, 13 edge types).  Per measurement both
settings run in the same process, interleaved, host clock around a device synchronise, medians with the spread, and the gate of
DESIGN.md section 28: the new median below the old one by more than the larger of the two spreads (max - min).

The driver starts one child process per (layout, width, measurement), each under its own time limit, checks every exit status and
stops at the first failure.

    python scratch/nnconv_bwd_eg_times.py --out profiles/nnconv_bwd_eg_times.txt
    rocprofv3 --kernel-trace --stats --output-format csv -d DIR -o t -- python scratch/nnconv_bwd_eg_times.py --child bench 64 profile0
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
DEPTH = 20
STEPS = [(name, w, what, limit) for name, lim in (("labyrinth", (120, 180)), ("bench", (240, 360))) for w in (32, 64)
         for what, limit in zip(("op", "step"), lim)]


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
    return (f"  gate: chain - eg = {m_old - m_new:.4f} ms, larger spread {worst:.4f} ms: "
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


def child(name, W, what, reps):
    import torch
    from tilingnn_amd import ops, train
    from tilingnn_amd.graph_networks.networks.TilinGNN import TilinGNN
    from tilingnn_amd.solver.ml_solver.losses import Losses
    from tilingnn_amd.weights import make_state_dict
    x, adj, attr, col = layout(name)
    n, fe = int(x.shape[0]), int(attr.shape[1])
    head = f"{name} ({n} nodes, {int(adj.shape[1])} / {int(col.shape[1])} edges), width {W}"
    ops.set_nnconv64_eg(1)                                   # the four older switches: on in both settings
    ops.set_gin64_mfma(1)
    train.set_mlp_bwd_fused(1)
    train.set_mlp_bwd_tall64(1)
    net = TilinGNN(adj_edge_features_dim=fe, network_depth=DEPTH, network_width=W, node_features_dim=int(x.shape[1]))
    net.load_state_dict(make_state_dict(fe, DEPTH, W, 1, int(x.shape[1]), seed=0))
    net = net.to(DEV).train()
    net.autograd = True

    if what == "op":
        reps_in = 10                                         # calls per timed window
        probs, sv = train.forward_train(net, x, adj, attr, col)
        tg, i = sv.tg, DEPTH - 1
        conv = net.brch_1_graph_conv_layers[i].nnConv
        g = torch.Generator().manual_seed(1)
        dz = (torch.randn(n, W, generator=g) * 1e-4).to(DEV)
        gsc = dz * tg.inv_deg[:, None]
        args = (conv, "p", tg, sv.wtab[i], sv.skip[i], dz, gsc, sv.ea)
        fns = [lambda k=k: [train.nnconv_backward(*args, {}, kernel=k) for _ in range(reps_in)] for k in ("chain", "eg")]
        for fn in fns:
            fn()
        ts = [[t / reps_in for t in tt] for tt in interleaved(fns, reps)]
        gt = tg.groups_t
        print(f"{head}: NNConv adjoint op, {tg.g.n_types} edge types, {gt.n_list} forward groups, in-/out-degree up to "
              f"{gt.max_in_degree} / {gt.max_out_degree}; times per call, {reps_in} calls per window")
        print(f"  chain (type sums, dense, wgrad)   {fmt(ts[0])}")
        print(f"  eg    (tgnn_nnconv_bwd_eg)        {fmt(ts[1])}")
        print(gate(ts[0], ts[1]))
        return

    def step():
        net.zero_grad(set_to_none=True)
        probs, _ = net(x, adj, attr, col)
        loss, _, _ = Losses.calculate_unsupervised_loss(probs, x, col, adj, attr)
        loss.backward()

    def with_switch(on):
        def run():
            prev = train.set_nnconv_bwd_eg(on)
            try:
                step()
            finally:
                train.set_nnconv_bwd_eg(prev)
        return run

    if what in ("profile0", "profile1"):                     # for rocprofv3 --kernel-trace --stats: three steps of one setting
        run = with_switch(int(what[-1]))
        for _ in range(3):
            run()
        torch.cuda.synchronize()
        return
    fns = [with_switch(0), with_switch(1)]
    for fn in fns:                                           # warm up both settings (graph preparation, groups, code objects)
        fn()
        fn()
    ts = interleaved(fns, reps)
    print(f"{head}: training step (forward, loss, backward; no optimizer), depth {DEPTH}, the four older switches on")
    print(f"  switch off (the chain)            {fmt(ts[0])}")
    print(f"  switch on  (tgnn_nnconv_bwd_eg)   {fmt(ts[1])}")
    print(gate(ts[0], ts[1]))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--child", nargs=3, default=None, metavar=("LAYOUT", "WIDTH", "WHAT"))
    ap.add_argument("--only", default=None, help="run only the measurements of this kind (op, step)")
    args = ap.parse_args()
    if args.child:
        child(args.child[0], int(args.child[1]), args.child[2], args.reps)
        return 0
    lines = [f"nnconv_bwd_eg_times: {args.reps} interleaved repetitions per setting, host clock around a device synchronise, "
             f"GPU_MAX_HW_QUEUES={os.environ.get('GPU_MAX_HW_QUEUES', 'unset')}"]
    print(lines[0], flush=True)
    rc = 0
    for name, w, what, limit in STEPS:
        if args.only and what != args.only:
            continue
        run = subprocess.run(["timeout", "-k", "10", str(limit), sys.executable, os.path.abspath(__file__), "--reps", str(args.reps),
                              "--child", name, str(w), what], capture_output=True, text=True, cwd=REPO)
        print(run.stdout, end="", flush=True)
        lines += run.stdout.splitlines()
        if run.returncode != 0:
            msg = f"STOPPED: {name} width {w} {what} ended with status {run.returncode}"
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
