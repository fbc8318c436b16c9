"""Shared layouts of the bf16-storage path's shape tests (tests/test_bf16_shapes.py, tests/test_bf16_cases_host.py).

A plain module: one seeded generator of small random layouts and the table of cases, chosen by what they exercise in
csrc/bf16_path.hip -- the 8-way row split below 8 rows, ragged 16-row tiles, the 8-block remap, every remainder of the 4-way
gather loop, rows without in-edges, no collision edges at all, in-degrees in the hundreds, the block cap."""
import torch

W = 64
FX, FE = 5, 15                   # tile_count 4 (node features), the adjacency attribute width of the test networks
ADJ_PER_NODE, N_TYPES = 4, 13
DEGREE_LADDER = 20               # rows 8 .. 27 get collision in-degree 0 .. 19 (layouts of 28 rows or more, with collision edges)

# (n, col_per_node, hub).  The last case was planned as (29 000, 8, 1500): the CPU model of tests/test_bf16_cases_host.py puts the
# REFERENCE's own storage error of that realisation at 5.4e-3 for the CollConv seam, above 0.6 x TOL_BF16 = 4.7e-3 (the maximum
# over 1.9 M elements of a BatchNorm output is a draw; 7 edges per node draws 3.7e-3) -- the nearest case the model accepts
# keeps the row count (past the block cap) and the hub's in-degree.
CASES = [(2, 1, 0), (7, 2, 0), (9, 2, 0), (17, 3, 0), (130, 8, 0), (1030, 8, 300), (3000, 1, 0), (3000, 0, 0), (29_000, 7, 1500)]
HUB_ROW, ISOLATED_ROW = 3, 5


def case_id(case):
    return "n%d-c%d-hub%d" % case


def random_graph(n, adj_per_node, col_per_node, n_types, seed, hub=0, isolated=True):
    """x [n, 5] fp32, adj [2, n * adj_per_node + hub] int64, attr [Ea, 15] fp32 drawn from `n_types` distinct rows,
    col [2, Ec] int64 -- CPU tensors.  hub > 0: that many more adjacency AND collision edges end in node 3; isolated: node 5
    has no in-edge in either graph (n > 6).  Self loops and duplicate edges occur as they fall (NNConv keeps self loops,
    GINConv drops them).  From 28 rows on, rows 8 .. 27 have exactly 0 .. 19 collision in-edges (no self loops among them):
    every remainder of a gather loop unrolled by four, at 0 .. 4 full rounds."""
    g = torch.Generator().manual_seed(seed)

    def edges(per_node):
        e = n * per_node
        src = torch.randint(0, n, (e,), generator=g)
        dst = torch.randint(0, n, (e,), generator=g)
        if hub and e:
            src = torch.cat([src, torch.randint(0, n, (hub,), generator=g)])
            dst = torch.cat([dst, torch.full((hub,), HUB_ROW, dtype=torch.int64)])
        return src, dst

    a_src, a_dst = edges(adj_per_node)
    c_src, c_dst = edges(col_per_node)
    if n >= 8 + DEGREE_LADDER and c_dst.numel():
        keep = (c_dst < 8) | (c_dst >= 8 + DEGREE_LADDER)
        c_src, c_dst = c_src[keep], c_dst[keep]
        for d in range(DEGREE_LADDER):
            row = 8 + d
            s = torch.randint(0, n - 1, (d,), generator=g)
            s = s + (s >= row).long()                                   # (any row but `row` itself)
            c_src = torch.cat([c_src, s])
            c_dst = torch.cat([c_dst, torch.full((d,), row, dtype=torch.int64)])
        perm = torch.randperm(c_dst.numel(), generator=g)               # (the ladder's edges anywhere in the edge list)
        c_src, c_dst = c_src[perm], c_dst[perm]
    if isolated and n > ISOLATED_ROW + 1:
        a_dst[a_dst == ISOLATED_ROW] = ISOLATED_ROW + 1
        c_dst[c_dst == ISOLATED_ROW] = ISOLATED_ROW + 1
    table = torch.rand(max(n_types, 1), FE, generator=g)
    typ = torch.randint(0, max(n_types, 1), (a_src.numel(),), generator=g)
    k = min(n_types, typ.numel())
    typ[:k] = torch.arange(k)                                            # every type occurs (as many as there are edges)
    x = torch.randn(n, FX, generator=g)
    return x, torch.stack([a_src, a_dst]), table[typ].contiguous(), torch.stack([c_src, c_dst])


def case_graph(case, seed=None, n_types=N_TYPES, adj_per_node=ADJ_PER_NODE):
    n, col_per_node, hub = case
    return random_graph(n, adj_per_node, col_per_node, n_types, seed if seed is not None else 1000 + n + col_per_node, hub=hub)


def col_in_degree(n, col):
    """In-degree of the collision graph as GINConv sees it (self loops removed)."""
    keep = col[0] != col[1]
    return torch.bincount(col[1][keep], minlength=n)
