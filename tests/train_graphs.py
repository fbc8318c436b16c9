"""Directed graphs for the adjoint tests (tests/test_training_sizes.py, tests/test_training_sizes_host.py).

Every larger graph of the suite (`make_super_graph`, the labyrinth layout) stores both directions of every pair: its transposed
CSR equals its forward CSR up to edge order and in-degree equals out-degree, so an adjoint that gathered along the wrong CSR or
divided by the wrong degree would pass on it.  `directed_graph` stores ONE direction of every pair and has rows whose two degrees
differ by hundreds."""
import numpy as np
import torch

N_MID = 4099             # the width-64 kernel tests' size: not a multiple of any kernel's rows per block
N_BIG = 66003            # > 65 536, no multiple of 4, 8, 16, 32 or 128: past every block / partial-row cap of csrc/backward.hip
EA_BIG, EC_BIG = 260000, 600002      # EC_BIG is past the 2048 x 256 edges of one sweep of the loss backward

ADJ_SINK, ADJ_SOURCE = 17, 23        # adjacency hubs: in-edges into row 17 (all of one type), out-edges from row 23
COL_SINK, COL_SOURCE = 5, 11         # collision hubs
NO_OUT = (100, 107)                  # rows 100 .. 106 have no out-edges (adjacency)
NO_IN_TAIL = 7                       # rows n - 7 .. n - 1 have no in-edges (adjacency)
ADJ_HUB, COL_HUB, SELF_LOOPS = 700, 400, 100


def hub_sizes(n):
    """(adjacency hub, collision hub) edge counts: 700 and 400, fewer on graphs too small for that many distinct neighbours."""
    return min(ADJ_HUB, n // 3), min(COL_HUB, n // 3)


def directed_graph(n, ea, ec, T, fe, seed):
    """-> x [n, 3] float32, adj [2, ea] int64, attr [ea, fe] float32, col [2, ec] int64 (CPU tensors; row 0 = source, row 1 =
    destination, as torch_geometric has it).

    adj: random directed edges, (v, u) never stored when (u, v) is and no pair twice; a sink hub (hub_sizes(n)[0] in-edges into
    row 17, all of one type) and a source hub (as many out-edges from row 23: the hub row of the TRANSPOSED CSR); rows n - 7 ..
    n - 1 get no in-edges, rows 100 .. 106 have no out-edges.  attr: exactly T distinct rows, each drawn once from U(0, 1), one
    type per edge, every type used.
    col: random directed edges, 100 self loops (GIN drops them), a sink hub into row 5 and a source hub from row 11."""
    if n < 200 or T < 1 or fe < 2:
        raise ValueError("directed_graph: n >= 200, T >= 1, fe >= 2")
    rng = np.random.default_rng(seed)
    hub_a, hub_c = hub_sizes(n)
    if ea < 2 * hub_a + T or ec < 2 * hub_c + SELF_LOOPS:
        raise ValueError("directed_graph: too few edges for the hubs")
    may_send = np.setdiff1d(np.arange(n), np.arange(*NO_OUT))
    may_recv = np.arange(n - NO_IN_TAIL)

    def distinct(pool, count, *without):
        return rng.choice(np.setdiff1d(pool, np.array(without)), size=count, replace=False)

    sink_src = distinct(may_send, hub_a, ADJ_SINK, ADJ_SOURCE)
    source_dst = distinct(may_recv, hub_a, ADJ_SINK, ADJ_SOURCE)
    src = np.concatenate([sink_src, np.full(hub_a, ADJ_SOURCE)])
    dst = np.concatenate([np.full(hub_a, ADJ_SINK), source_dst])
    while True:                                               # random pairs until `ea` unordered pairs are distinct
        more = 2 * (ea - src.shape[0]) + 64
        src = np.concatenate([src, may_send[rng.integers(0, may_send.shape[0], more)]])
        dst = np.concatenate([dst, may_recv[rng.integers(0, may_recv.shape[0], more)]])
        key = np.minimum(src, dst).astype(np.int64) * n + np.maximum(src, dst)
        _, first = np.unique(key, return_index=True)
        first = np.sort(first)                                # keeps the hubs: they come first
        first = first[src[first] != dst[first]]
        src, dst = src[first], dst[first]
        if src.shape[0] >= ea:
            src, dst = src[:ea], dst[:ea]
            break
    etype = rng.integers(0, T, ea)
    etype[:hub_a] = int(rng.integers(0, T))                   # the sink hub: hundreds of edges of one type on one row
    etype[2 * hub_a:2 * hub_a + T] = np.arange(T)             # every type is used
    order = rng.permutation(ea)
    src, dst, etype = src[order], dst[order], etype[order]
    rows = rng.random((T, fe)).astype(np.float32)
    if np.unique(rows, axis=0).shape[0] != T:
        raise ValueError("directed_graph: two attribute rows coincide; take another seed")
    attr = rows[etype]

    n_rand = ec - 2 * hub_c - SELF_LOOPS
    loops = rng.integers(0, n, SELF_LOOPS)
    c_src = np.concatenate([rng.integers(0, n, n_rand), loops, distinct(np.arange(n), hub_c, COL_SINK), np.full(hub_c, COL_SOURCE)])
    c_dst = np.concatenate([rng.integers(0, n, n_rand), loops, np.full(hub_c, COL_SINK), distinct(np.arange(n), hub_c, COL_SOURCE)])
    order = rng.permutation(ec)
    c_src, c_dst = c_src[order], c_dst[order]

    x = np.zeros((n, 3), dtype=np.float32)                    # two tile types one-hot, then the area ratio the loss reads
    x[np.arange(n), rng.integers(0, 2, n)] = 1.0
    x[:, 2] = 0.2 + 0.8 * rng.random(n)
    return (torch.from_numpy(x), torch.from_numpy(np.stack([src, dst]).astype(np.int64)), torch.from_numpy(attr),
            torch.from_numpy(np.stack([c_src, c_dst]).astype(np.int64)))


def edge_types(attr):
    """-> (type of every edge [Ea] int64, number of distinct attribute rows)."""
    uniq, inv = torch.unique(attr, dim=0, return_inverse=True)
    return inv, int(uniq.shape[0])


def degrees(edge_index, n):
    """-> (in-degree, out-degree) int64 [n]."""
    return torch.bincount(edge_index[1], minlength=n), torch.bincount(edge_index[0], minlength=n)
