"""fp64 restatement of "the unsupervised loss of K layouts" for tests/test_loss_many*.py, in numpy alone: independent of
`PackedLayouts`, of the kernels and of the oracle package (tests/test_loss_many_host.py pins it against
`oracle.unsupervised_losses` on the reference's golden cases).

A layout is (x [N, Fx], adj [2, Ea], attr [Ea, Fe], col [2, Ec]) as numpy; its probabilities [N, M].  Per map m
(the reference's solver/ml_solver/losses.py:48-116):
    t_area  = log(max(mean_v x[v, -1] p[v], eps))
    t_feas  = mean over collision edges of log(1 - clamp(p[i] p[j], eps, 1 - eps))         (0 without such edges)
    t_align = mean over adjacency edges of log10(max(p[i] p[j] attr[e, 1], eps))            (0 without such edges)
    loss    = (1 - Wa t_area) (1 - Wc t_feas) (1 - Wl t_align)
"""
import math

import numpy as np

EPS = 1e-7
WEIGHTS = (1.0 / math.log(1.0 + 1e-1), 0.02, 1.0)            # (collision, align length, average area): inputs/config.py:49-51


def loss_blocks(n, ec, ea):
    """Blocks of 256 threads the loss kernels give one layout: clamp(ceil(max(n, ec, ea) / 1024), 1, 512)."""
    work = max(int(n), int(ec), int(ea))
    return int(min(max(-(-work // 1024), 1), 512))


def groups(n, group):
    """range(n) in contiguous groups of `group`, the short last one kept."""
    return [list(range(i, min(i + group, n))) for i in range(0, n, group)]


def loss_terms(layout, probs, weights=WEIGHTS):
    """(losses [M], terms [M, 3]) of one layout in float64."""
    x, adj, attr, col = (np.asarray(a) for a in layout)
    p_all = np.asarray(probs, dtype=np.float64)
    wc, wl, wa = weights
    adj, col = adj.reshape(2, -1), col.reshape(2, -1)
    losses, terms = [], []
    for m in range(p_all.shape[1]):
        p = p_all[:, m]
        t_area = math.log(max(float(np.mean(x[:, -1].astype(np.float64) * p)), EPS))
        t_feas = t_align = 0.0
        if col.shape[1]:
            t_feas = float(np.mean(np.log(1.0 - np.clip(p[col[0]] * p[col[1]], EPS, 1.0 - EPS))))
        if adj.shape[1]:
            t_align = float(np.mean(np.log(np.maximum(p[adj[0]] * p[adj[1]] * attr[:, 1].astype(np.float64), EPS)) / math.log(10.0)))
        terms.append((t_area, t_feas, t_align))
        losses.append((1.0 - wa * t_area) * (1.0 - wc * t_feas) * (1.0 - wl * t_align))
    return np.array(losses), np.array(terms).reshape(-1, 3)


def losses_many(layouts, probs, active=None, weights=WEIGHTS):
    """Per layout (losses, terms), or None where the batched call writes nothing: probs None, inactive, or no nodes."""
    out = []
    for k, (lay, p) in enumerate(zip(layouts, probs)):
        if p is None or (active is not None and not active[k]) or np.asarray(lay[0]).shape[0] == 0:
            out.append(None)
        else:
            out.append(loss_terms(lay, p, weights))
    return out


def sub_layout(layout, alive):
    """compute_sub_layout (brick_layout.py:248-286) on arrays: the nodes with alive != 0 in ascending order, the edges with both
    ends alive in edge order, ends renumbered."""
    x, adj, attr, col = layout
    alive = np.asarray(alive) != 0
    new = np.cumsum(alive) - 1
    keep_a = alive[adj[0]] & alive[adj[1]] if adj.shape[1] else np.zeros(0, bool)
    keep_c = alive[col[0]] & alive[col[1]] if col.shape[1] else np.zeros(0, bool)
    return x[alive], new[adj[:, keep_a]], attr[keep_a], new[col[:, keep_c]]
