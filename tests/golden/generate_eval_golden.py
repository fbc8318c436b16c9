#!/usr/bin/env python3
"""Generate tests/golden/ref_forward_eval.npz from the REFERENCE ITSELF, in .eval().

Runs only where the reference checkout is mounted (see generate_golden.py, whose recipe this follows: the reference's
graph_networks/* imported UNCHANGED, `inputs.config` stubbed, the two PyG convolutions stood in by generate_golden.py's classes --
nothing is copied).  The reference never calls .eval() itself (ml_solver.py:129-131); its modules are torch.nn modules, so
`network.eval()` is defined by torch: every nn.BatchNorm1d normalises with its running buffers.

Per case of tests/eval_cases.py: GOLDEN_CASES (the labyrinth graph at width 32 and 64, a 17-row and a one-row synthetic layout):
the case's state dict -- conditioned running buffers included -- is loaded into the reference network, which runs in float64:

  <case>/probs          [N, 1]   float64
  <case>/rows, /cols             the sampled rows (up to 64) and columns (8) of the skip slots
  <case>/middle         [D + 1, rows, cols]  float64: middle[k] (TilinGNN.py:58,71) read off the final MLP's input
  <case>/middle_colsum  [D + 1, C]           float64: column sums over ALL rows (every entry of every slot enters the pin)
  <case>/bn_mean, /bn_var        the running buffers, concatenated in state-dict order, float32 (what the test's recipe must
                                 reproduce bit for bit before the comparison means anything)

All columns of 64 rows in float64 would be 1.1 MB; the file stays under 400 KB by sampling columns, the column sums keep
every entry in the comparison."""
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
REPO = os.path.dirname(os.path.dirname(HERE))
sys.dont_write_bytecode = True
sys.path.insert(0, REPO)
sys.path.insert(0, HERE)

from generate_golden import import_reference  # noqa: E402
from tests import eval_cases  # noqa: E402


def sample(n, c):
    rows = np.unique(np.linspace(0, n - 1, min(n, 64)).astype(np.int64))
    cols = np.arange(0, c, c // 8, dtype=np.int64)
    return rows, cols


def run_reference(case):
    TilinGNN = import_reference(case.tile_count)
    net = TilinGNN(adj_edge_features_dim=case.fe, network_depth=case.depth, network_width=case.width, output_dim=case.out_dim,
                   node_features_dim=case.fx)
    sd = case.state_dict()
    net.load_state_dict(sd, strict=True)
    net = net.double().eval()
    seen = {}
    hook = net.final_mlp.register_forward_pre_hook(lambda mod, inp: seen.__setitem__("cat", inp[0].detach().clone()))
    x, adj, attr, col = case.inputs()
    with torch.no_grad():
        probs, _ = net(x=x, adj_e_index=adj, adj_e_features=attr, col_e_idx=col, col_e_features=None)
    hook.remove()
    after = net.state_dict()
    for k, v in sd.items():                                      # .eval() writes no buffer
        assert torch.equal(after[k], v.double() if v.is_floating_point() else v), k
    middle = seen["cat"].view(case.n, case.depth + 1, case.width).permute(1, 0, 2).numpy()
    rows, cols = sample(case.n, case.width)
    bn = lambda leaf: np.concatenate([v.numpy().ravel() for k, v in sd.items() if k.endswith(leaf)]).astype(np.float32)
    return {"probs": probs.numpy(), "rows": rows, "cols": cols, "middle": middle[:, rows][:, :, cols],
            "middle_colsum": middle.sum(axis=1), "bn_mean": bn("running_mean"), "bn_var": bn("running_var")}


def main():
    torch.manual_seed(0)
    torch.set_num_threads(1)                                     # deterministic summation order
    out = {}
    for name in eval_cases.GOLDEN_CASES:
        for k, v in run_reference(eval_cases.CASES[name]).items():
            out[f"{name}/{k}"] = v
    path = os.path.join(HERE, "ref_forward_eval.npz")
    np.savez_compressed(path, **out)
    size = os.path.getsize(path)
    print(f"ref_forward_eval.npz: {size / 1024:.1f} KiB, {len(out)} members")
    assert size < 400 * 1024


if __name__ == "__main__":
    main()
