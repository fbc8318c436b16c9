"""The optimizer step of the training loop: torch.optim.Adam as the reference's network_train.py:27 builds it (default arguments: the
multi-tensor path), torch.optim.Adam(fused=True) where this torch accepts it, and tilingnn_amd.optim.Adam (csrc/adam.hip: ONE launch
over the backward's flat gradient buffer) -- (a) the optimizer step alone on the gradients of one real backward, (b) the whole
training step (zero_grad, forward, loss, backward, optimizer step) at depth 20 -- at widths 32 and 64, on the labyrinth layout
(1 254 nodes) and on the benchmark's layout (100 000 nodes, 1 M adjacency / 1.25 M collision edges, 13 edge types).  Per measurement
the optimizers run in the same process, interleaved, 7 repetitions, host clock around a device synchronise; medians with the spread
(max - min) of each row's own repetitions, and the verdict the records ask for: the fused step is not slower than torch's default
beyond the larger of the two spreads.

The driver starts one child process per (layout, width), each under its own time limit, checks every exit status and stops at the
first failure.

    python scratch/adam_times.py --out profiles/adam_fused_times.txt
    rocprofv3 --kernel-trace --stats --output-format csv -d DIR -o t -- python scratch/adam_times.py --child labyrinth 32 profile
    (profile: THREE training steps with tilingnn_amd.optim.Adam, nothing else)
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
REPS = 7
CASES = [(name, w, limit) for name, limit in (("labyrinth", 150), ("bench", 400)) for w in (32, 64)]


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
    return f"median {m:9.4f} ms  ({min(ts):.4f} - {max(ts):.4f}, spread {max(ts) - min(ts):.4f} ms)"


def verdict(ts_default, ts_ours):
    m_old, m_new = statistics.median(ts_default), statistics.median(ts_ours)
    worst = max(max(ts_default) - min(ts_default), max(ts_ours) - min(ts_ours))
    return (f"  torch default - fused one-launch = {m_old - m_new:+.4f} ms ({m_old / m_new:.2f} x), larger spread {worst:.4f} ms: "
            f"{'not slower' if m_new <= m_old + worst else 'SLOWER'}{', faster beyond the spread' if m_old - m_new > worst else ''}")


def layout(name):
    import torch
    if name == "bench":
        from tilingnn_amd.synth import make_super_graph
        sg = make_super_graph(100_000, 1_000_000, 1_250_000, tile_count=2, n_edge_types=13, seed=1)
        x, adj, attr, col, _ = sg.to_torch(DEV)
        return x, adj, attr, col
    from tests.golden_util import graph_tensors, load_labyrinth_graph
    return graph_tensors(load_labyrinth_graph(), torch.float32, DEV)[:4]


def child(name, W, what):
    import torch
    from tilingnn_amd import optim
    from tilingnn_amd.graph_networks.networks.TilinGNN import TilinGNN
    from tilingnn_amd.solver.ml_solver.losses import Losses
    from tilingnn_amd.weights import make_state_dict
    x, adj, attr, col = layout(name)
    n, fe = int(x.shape[0]), int(attr.shape[1])
    net = TilinGNN(adj_edge_features_dim=fe, network_depth=DEPTH, network_width=W, node_features_dim=int(x.shape[1]))
    net.load_state_dict(make_state_dict(fe, DEPTH, W, 1, int(x.shape[1]), seed=0))
    net = net.to(DEV).train()
    net.autograd = True
    params = list(net.parameters())
    floats = sum(p.numel() for p in params)
    lr = 1e-6                                                # (many steps on one layout: the weights should stay where they are)

    def backward():
        probs, _ = net(x, adj, attr, col)
        loss, _, _ = Losses.calculate_unsupervised_loss(probs, x, col, adj, attr)
        loss.backward()

    if what == "profile":
        opt = optim.Adam(params, lr=lr)
        for _ in range(3):
            opt.zero_grad()
            backward()
            opt.step()
        torch.cuda.synchronize()
        assert opt.launches == 3 and opt.table_uploads == 1
        return

    rows = [("torch.optim.Adam (default)", torch.optim.Adam(params, lr=lr))]
    try:
        rows.append(("torch.optim.Adam(fused=True)", torch.optim.Adam(params, lr=lr, fused=True)))
    except (RuntimeError, ValueError, TypeError) as e:       # this torch does not take fused=True here
        print(f"  (torch.optim.Adam(fused=True) refused: {e})")
    ours = optim.Adam(params, lr=lr)
    rows.append(("tilingnn_amd.optim.Adam", ours))
    print(f"{name} ({n} nodes, {int(adj.shape[1])} / {int(col.shape[1])} edges), width {W}: {len(params)} parameter tensors, "
          f"{floats} floats ({7 * 4 * floats / 1e6:.1f} MB to move per step: read p, g, m, v, write p, m, v)")

    # (a) the optimizer step alone, on the gradients one real backward left
    backward()
    torch.cuda.synchronize()
    calls = 10                                               # steps per timed window
    fns = [lambda o=o: [o.step() for _ in range(calls)] for _, o in rows]
    for fn in fns:
        fn()
    ts = [[t / calls for t in tt] for tt in interleaved(fns, REPS)]
    print(f" optimizer step alone (per step, {calls} steps per window, host clock around a device synchronise):")
    for (label, _), tt in zip(rows, ts):
        print(f"  {label:32s} {fmt(tt)}")
    print(verdict(ts[0], ts[-1]))

    # (b) the whole training step
    def step_with(o):
        def run():
            o.zero_grad()
            backward()
            o.step()
        return run
    fns = [step_with(o) for _, o in rows]
    for fn in fns:
        fn()
        fn()
    ts = interleaved(fns, REPS)
    print(" whole training step (zero_grad, forward, loss, backward, optimizer step):")
    for (label, _), tt in zip(rows, ts):
        print(f"  {label:32s} {fmt(tt)}")
    print(verdict(ts[0], ts[-1]))
    print(f"  (tilingnn_amd.optim.Adam: {ours.launches} launches, {ours.table_uploads} table upload(s))")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--child", nargs=3, metavar=("LAYOUT", "WIDTH", "WHAT"))
    ap.add_argument("--out")
    a = ap.parse_args()
    if a.child:
        child(a.child[0], int(a.child[1]), a.child[2])
        return
    lines = []
    for name, w, limit in CASES:
        r = subprocess.run([sys.executable, os.path.abspath(__file__), "--child", name, str(w), "times"], capture_output=True,
                           text=True, timeout=limit)
        sys.stdout.write(r.stdout)
        sys.stdout.flush()
        if r.returncode != 0:
            sys.stderr.write(r.stderr[-3000:])
            raise SystemExit(f"{name} width {w}: exit status {r.returncode}; stopping")
        lines.append(r.stdout)
    if a.out:
        with open(a.out, "w") as f:
            f.write("scratch/adam_times.py: torch.optim.Adam (default), torch.optim.Adam(fused=True) and tilingnn_amd.optim.Adam, "
                    f"interleaved in one process per case, {REPS} repetitions each\n\n")
            f.write("\n".join(lines))


if __name__ == "__main__":
    main()
