"""Every output array of the greedy and loss entries that csrc/greedy_rule.h and csrc/loss_sums.h serve, written to one .npz -- to
compare two builds of the library byte for byte (the expressions and the fixed trees are the same, so equality is the
expectation, not a tolerance):
    TGNN_LIB_PATH=<library A> python scratch/greedy_rule_refactor_bytes.py a.npz
    TGNN_LIB_PATH=<library B> python scratch/greedy_rule_refactor_bytes.py b.npz
    python scratch/greedy_rule_refactor_bytes.py --compare a.npz b.npz
Calls: tgnn_greedy_round / _round_many at sub-layout sizes 65, 1025, 5000; tgnn_greedy_finish / _finish_many at 5, 1025, 4096;
tgnn_unsupervised_loss / _loss_many and tgnn_solution_score_sums / _sums_many at 1025 items (two blocks); one
solve_many_by_device_greedy of the bunny crops (selections, orders, round counts, scores).  Inputs: the case builders of
tests/test_greedy_ops.py and tests/test_loss_many.py, seeded."""
import ctypes as C
import hashlib
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

if sys.argv[1] == "--compare":
    a, b = np.load(sys.argv[2]), np.load(sys.argv[3])
    assert sorted(a.files) == sorted(b.files), (a.files, b.files)
    same = []
    for name in a.files:
        x, y = a[name], b[name]
        same.append(x.dtype == y.dtype and x.shape == y.shape and x.tobytes() == y.tobytes())
        print(f"{name}: {x.dtype} {x.shape} sha256 {hashlib.sha256(x.tobytes()).hexdigest()[:16]} / "
              f"{hashlib.sha256(y.tobytes()).hexdigest()[:16]} {'identical' if same[-1] else 'DIFFERENT'}")
    print(f"greedy and loss entries, {sys.argv[2]} against {sys.argv[3]}: {sum(same)} of {len(same)} arrays byte-identical")
    sys.exit(0 if all(same) else 1)

import torch  # noqa: E402

from scratch import solve_many_times as smt  # noqa: E402
from tests import test_greedy_ops as ops  # noqa: E402
from tests import test_loss_many as tlm  # noqa: E402
from tilingnn_amd import _lib  # noqa: E402
from tilingnn_amd._lib import check, lib, ptr  # noqa: E402
from tilingnn_amd.solver.ml_solver.losses import Losses  # noqa: E402
from tilingnn_amd.util import algorithms as alg  # noqa: E402

DEV = torch.device("cuda:0")
out = {}


def keep(prefix, **tensors):
    for name, t in tensors.items():
        out[f"{prefix}.{name}"] = t.cpu().numpy() if torch.is_tensor(t) else np.asarray(t)


# ---- one round, single and many
for n in (65, 1025, 5000):
    c = ops.build_round_case(f"n{n}", n, True, 3, ops.SEEDS[1], 3, "loops_dups", 17, 9000 + n)
    prob_d, saved_d, alive_d, sel_d, inv_d, col_d = (ops._t(a) for a in (c.prob, c.saved, c.alive, c.selected, c.inverse, c.col))
    tail = ops._t(np.array([c.n_sel0, 0], dtype=np.int64))
    wsb = int(lib.tgnn_greedy_round_workspace_bytes(c.n))
    ws = torch.empty(wsb, dtype=torch.uint8, device=DEV)
    check(lib.tgnn_greedy_round(C.c_void_p(prob_d.data_ptr() + 4 * c.column), c.ld, ptr(inv_d), c.n, ptr(col_d), int(c.col.shape[1]), c.rnd,
                                c.seed, ptr(saved_d), ptr(alive_d), ptr(sel_d), ptr(tail[:1]), ptr(tail[1:].view(torch.int32)[:1]), ptr(ws),
                                wsb, _lib.current_stream(DEV)))
    torch.cuda.synchronize()
    keep(f"round{n}", saved=saved_d, alive=alive_d, selected=sel_d, n_selected_err=tail)
rng = np.random.default_rng(5)
many = ops.ManyCase("bytes", [ops._many_layout(rng, n, 4 * n, 3, 2, 11 + k, null_prob=k == 1, n_sel0=k) for k, n in enumerate((65, 1025, 5000))],
                    3, 2, 1, first_round=3)
st = ops.ManyDevice(many)
st.round()
keep("round_many", saved=st.saved, alive=st.alive, selected=st.selected, n_selected=st.n_sel, err=st.err)

# ---- the finish, single and many
for n in (5, 1025, 4096):
    c = ops.build_finish_case(f"n{n}", n, 4, True, 0.3, "both", ops.SEEDS[2], 1000, 9100 + n)
    rc, saved_d, alive_d, sel_d, tail, o = ops._run_finish(c)
    assert rc == 0
    keep(f"finish{n}", saved=saved_d, alive=alive_d, selected=sel_d, n_selected_err=tail, out=o)
rng = np.random.default_rng(6)
many = ops.ManyCase("bytes", [ops._many_layout(rng, n, 4 * n, 2, 1, 21 + k) for k, n in enumerate((5, 1025, 4096))], 2, 1, 0, first_round=2)
st = ops.ManyDevice(many)
st.finish()
keep("finish_many", saved=st.saved, alive=st.alive, selected=st.selected, n_selected=st.n_sel, err=st.err, out=st.out)

# ---- the loss and the score sums at 1025 items: nodes, collision edges, adjacency edges the largest set in turn
rng = np.random.default_rng(7)
arrays = [tlm._synthetic(rng, *s) for s in ((1025, 600, 300), (300, 1025, 200), (300, 500, 1025))]
layouts = [tlm._dev(a) for a in arrays]
pk = alg.PackedLayouts(layouts, DEV)
probs = [torch.from_numpy(tlm._probs(rng, a[0].shape[0], 2)).to(DEV) for a in arrays]
losses, terms, err = Losses.unsupervised_losses_many(probs, pk)
keep("loss_many", losses=losses, terms=terms, err=err)
for k, (lay, p) in enumerate(zip(layouts, probs)):
    l, t = tlm._solo(lay, p)
    keep(f"loss{k}", losses=l, terms=t)
K = len(layouts)
predict = ops._t((rng.uniform(size=pk.n) < 0.3).astype(np.float32))
perim = ops._t(rng.uniform(1.0, 9.0, size=pk.n).astype(np.float32))
sums = torch.zeros(K, 3, dtype=torch.float64, device=DEV)
wsb = int(lib.tgnn_solution_score_sums_many_workspace_bytes(K))
ws = torch.empty(wsb, dtype=torch.uint8, device=DEV)
check(lib.tgnn_solution_score_sums_many(K, None, ptr(pk.node_ptr), ptr(pk.adj_ptr), pk.n, pk.ea, ptr(predict),
                                        C.c_void_p(pk.x.data_ptr() + 4 * (pk.fx - 1)), pk.fx, ptr(perim), ptr(pk.adj),
                                        C.c_void_p(pk.attr.data_ptr() + 4), pk.fe, ptr(sums), ptr(ws), wsb, _lib.current_stream(DEV)))
keep("score_many", sums=sums)
wsb1 = int(lib.tgnn_unsupervised_loss_workspace_bytes(1))
ws1 = torch.empty(wsb1, dtype=torch.uint8, device=DEV)
for k, l in enumerate(layouts):
    sl = slice(pk.node_ptr_h[k], pk.node_ptr_h[k + 1])
    n, ea = int(l.node_feature.shape[0]), int(l.align_edge_index.shape[1])
    x, attr, adj = l.node_feature.contiguous(), l.align_edge_features.contiguous(), l.align_edge_index.contiguous()
    pk_, perk = predict[sl].clone(), perim[sl].clone()
    one = torch.zeros(3, dtype=torch.float64, device=DEV)
    check(lib.tgnn_solution_score_sums(ptr(pk_), C.c_void_p(x.data_ptr() + 4 * (x.shape[1] - 1)), x.shape[1], ptr(perk), n, ptr(adj), ea,
                                       C.c_void_p(attr.data_ptr() + 4), attr.shape[1], ptr(one), ptr(ws1), wsb1, _lib.current_stream(DEV)))
    keep(f"score{k}", sums=one)

# ---- one batched solve of the bunny crops
graph, crops = smt.WORKLOADS["bunny"]()
ms = smt.solver(graph)
got = alg.solve_many_by_device_greedy(ms, crops, seed=0)
keep("solve_many", rounds=np.array(alg.solve_many_by_device_greedy.last_rounds, dtype=np.int64),
     scores=np.array([float(g[1]) for g in got], dtype=np.float64), selections=np.concatenate([np.asarray(g[0], np.float64) for g in got]),
     orders=np.concatenate([np.asarray(g[2], np.int64) for g in got]))
torch.cuda.synchronize()
np.savez(sys.argv[1], **out)
print(f"{_lib.LIB_PATH}: {len(out)} arrays -> {sys.argv[1]}")
