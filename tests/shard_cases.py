"""Partitions the sharded forward (tilingnn_amd.dist, tgnn_forward_sharded) meets in a real solve and no other test cuts: uneven,
one-way and empty ones.  Plain module: numpy, torch on the CPU, the oracle -- no GPU import.  tests/test_shard_cases_host.py asserts
the preconditions of every kind and the gate on the CPU; tests/test_shard_shapes.py runs the case table on the device.

Kinds (world 4 and 96 rows per rank unless stated; every node has 4 adjacency and 5 collision in-edges from its own range unless
the kind says otherwise; edge order shuffled; 13 one-hot edge types as in tilingnn_amd/synth.py):

  islands         ranks 1 and 3 exchange with nobody (halo 0, send 0, every recv_counts entry 0); ranks 0 and 2 exchange across rank 1
  one_way         every cross edge of both sets runs from rank r + 1 into rank r: the last rank has halo 0 and send > 0, rank 0 has
                  send 0 and halo > 0
  hub             one row of rank 2 is a source into rows of every rank (sent to all peers: its send_row_ptr count is world - 1); one
                  row of rank 0 has 200 remote sources (rank 0's halo is more than twice its owned rows)
  branch_missing  rank 1 has no adjacency in-edge at all (ea_loc == 0, n_types == 0, max_in_degree == 0 there) but is a source for
                  others; rank 3 has no collision in-edge
  deg2049         704 rows per rank; one row of rank 1 has 2 049 adjacency in-edges from distinct sources (one above the edge-group
                  kernel's limit), every other row at most 16
  tiny            `hub` (its 200-source row moved to row 1) compacted through dist.compact_shard with an alive mask that leaves ranges
                  of 2, 15, 17 and 96 rows; rank 0 keeps a halo of more than 4 x its 2 owned rows
  width64         `one_way` at world 2, network width 64

Schemes: fused (FusedShardForward(fused=True), one stream), split (the same with two_streams), split_nopack (split with
pack_in_nnconv = False), allreduce (fused=False), per_op (ShardProgram over HipBackend through LocalSimComm).

The gate.  Reference: the fp64 oracle (oracle.tilingnn_oracle.tilingnn_forward, update_running=True, capture) on the GLOBAL graph --
for `tiny` the sub-layout of oracle.greedy_oracle.compute_sub_layout.  Per skip-buffer slot k = 0 .. D and for the probabilities the
figure is the max-norm relative error  max |got - want| / max |want|.  The yardstick is computed, not fixed: the same oracle evaluated
in fp32 (fp32 weights, fp32 inputs) against the fp64 one gives err32[k], and

    gate[k] = MARGIN * max(err32[k], dense_oracle.REL_MAX_TOL),    MARGIN = 4.

Where the 4 comes from: the device's fp16-pair forms carry up to about 4 x the rounding units of a plain fp32 evaluation of the same
op -- tests/nnconv_cases.py: C0 is 21 units for the edge-group kernel against 5 - 6 for the CSR kernel and for torch -- and every
train-mode BatchNorm behind an op amplifies both roundings alike, so a correct device forward stays within 4 x what the plain fp32
evaluation of the same network loses on the same graph.  The floor REL_MAX_TOL (2e-6) is the project's per-op max-norm gate: where
the fp32 oracle happens to be closer than that, the device is not asked for more than any single op is.
A BatchNorm's running statistics are held the same way, per buffer: the fp32 oracle's updated buffer against the fp64 oracle's is
the yardstick, floor and margin as above.
"""
import contextlib
from dataclasses import dataclass
from typing import Dict, List

import numpy as np
import torch

from oracle import greedy_oracle as go
from oracle import tilingnn_oracle as orc
from tests.dense_oracle import REL_MAX_TOL
from tilingnn_amd import dist as tdist
from tilingnn_amd.weights import make_state_dict

N_TYPES, FE, FX = 13, 15, 3
MARGIN = 4.0
SEED_NET = 2
EG_MAX_IN_DEGREE = 2048                 # csrc/forward_plan.h: groups_ok
KINDS = ("islands", "one_way", "hub", "branch_missing", "deg2049", "tiny")
SCHEMES = ("fused", "split", "split_nopack", "allreduce", "per_op")
ONE_ALLTOALL = ("fused", "split", "split_nopack")
TINY_RANGES = (2, 15, 17, 96)
HUB_SOURCE_ROW = 7                      # of rank 2: the row every rank reads
HUB_FAN_IN = 200                        # remote sources of one row of rank 0


def world_of(kind):
    return 2 if kind == "width64" else 4


def width_of(kind):
    return 64 if kind == "width64" else 32


def rows_per_rank(kind):
    return 704 if kind == "deg2049" else 96


# ---- generators ------------------------------------------------------------------------------------------------------------------
def _generate(kind, world, per, seed=0, fan_in_row=5):
    rng = np.random.default_rng(seed)
    n = world * per
    x = np.zeros((n, FX))
    t = rng.integers(0, 2, n)
    x[np.arange(n), t] = 1
    x[:, 2] = np.where(t == 0, 1.0, 0.5)
    rank = np.arange(n) // per

    def intra(k):                      # k in-edges per node from its own range
        dst = np.repeat(np.arange(n), k)
        return np.stack([rank[dst] * per + rng.integers(0, per, dst.size), dst])

    def cross(src_rank, dst_rank, m):
        return np.stack([src_rank * per + rng.integers(0, per, m), dst_rank * per + rng.integers(0, per, m)])
    adj, col = [intra(4)], [intra(5)]
    if kind == "islands":
        for e in (adj, col):
            e += [cross(0, 2, 150), cross(2, 0, 150)]
    elif kind == "one_way":
        for e in (adj, col):
            e += [cross(r + 1, r, 120) for r in range(world - 1)]
    elif kind == "hub":
        h = 2 * per + HUB_SOURCE_ROW
        for e in (adj, col):
            e += [np.stack([np.full(40, h), r * per + rng.choice(per, 40, replace=False)]) for r in range(world)]
            e += [np.stack([per + rng.choice(n - per, HUB_FAN_IN, replace=False), np.full(HUB_FAN_IN, fan_in_row)])]
    elif kind == "branch_missing":
        adj = [a[:, rank[a[1]] != 1] for a in adj] + [cross(1, 0, 100), cross(0, 2, 100), cross(3, 2, 50)]
        col = [c[:, rank[c[1]] != 3] for c in col] + [cross(3, 0, 100), cross(1, 2, 100), cross(0, 1, 50)]
    elif kind == "deg2049":
        g = per + 3                                              # the row of rank 1 with 2 049 distinct adjacency sources
        others = np.delete(np.arange(n), g)
        adj = [a[:, a[1] != g] for a in adj] + [np.stack([rng.choice(others, EG_MAX_IN_DEGREE + 1, replace=False),
                                                          np.full(EG_MAX_IN_DEGREE + 1, g)])]
        for r in range(world):                                   # a few cross edges of both sets in both directions, none into g
            c_adj = cross((r + 1) % world, r, 120)
            adj.append(c_adj[:, c_adj[1] != g])
            col.append(cross((r + 1) % world, r, 120))
            col.append(cross(r, (r + 1) % world, 60))
    else:
        raise ValueError(kind)
    adj, col = np.concatenate(adj, 1), np.concatenate(col, 1)
    adj = adj[:, rng.permutation(adj.shape[1])]
    col = col[:, rng.permutation(col.shape[1])]
    et = rng.integers(0, N_TYPES, adj.shape[1])
    attr = np.zeros((adj.shape[1], FE))
    attr[:, 1] = np.where(et % 2 == 0, float(np.float32(0.57735)), 1.0)      # (fp32-representable: both oracles and the device read the same numbers)
    attr[np.arange(et.size), 2 + et] = 1
    return x, adj.astype(np.int64), attr, col.astype(np.int64)


def tiny_alive(per=96):
    """The alive mask over `hub` at 4 x 96 rows that leaves ranges of 2, 15, 17 and 96 rows."""
    alive = np.zeros(4 * per, dtype=bool)
    for r, k in enumerate(TINY_RANGES):
        alive[r * per: r * per + k] = True
    return alive


@dataclass
class Case:
    kind: str
    world: int
    width: int
    graph: tuple                       # (x, adj, attr, col) of the GLOBAL graph the oracle evaluates (tiny: the sub-layout)
    shards: List[tdist.Shard]          # send lists exchanged (LocalSimComm.setup)
    base: tuple = None                 # tiny: the graph and the shards in front of the compaction, the alive mask
    base_shards: List[tdist.Shard] = None
    alive: np.ndarray = None


_CASES: Dict[str, Case] = {}


def case(kind) -> Case:
    """The kind's global graph and its shards (built once; nobody changes them)."""
    if kind in _CASES:
        return _CASES[kind]
    world, per = world_of(kind), rows_per_rank(kind)
    if kind == "tiny":
        base = _generate("hub", world, per, seed=3, fan_in_row=1)
        base_shards = [tdist.make_shard(*base, r, world) for r in range(world)]
        alive = tiny_alive(per)
        shards = [tdist.compact_shard(s, alive) for s in base_shards]
        sub = go.compute_sub_layout(base[0], base[1], base[2], base[3], np.zeros((base[3].shape[1], 1)), np.flatnonzero(alive))
        c = Case(kind, world, 32, (sub[0], sub[1], sub[2], sub[3]), shards, base, base_shards, alive)
    else:
        graph = _generate("one_way" if kind == "width64" else kind, world, per)
        shards = [tdist.make_shard(*graph, r, world) for r in range(world)]
        c = Case(kind, world, width_of(kind), graph, shards)
    tdist.LocalSimComm.setup(c.shards)
    _CASES[kind] = c
    return c


# ---- the case table --------------------------------------------------------------------------------------------------------------
def _table():
    rows = [(k, s, 3) for k in KINDS for s in SCHEMES]
    rows += [(k, s, 20) for k in ("one_way", "branch_missing") for s in ("fused", "split")]
    rows += [("width64", s, 3) for s in ("allreduce", "per_op")]
    return rows


CASE_TABLE = _table()
REFERENCE_ROWS = sorted({(k, d) for k, _, d in CASE_TABLE})


# ---- which plan a rank's forward takes (csrc/forward_plan.h: the terms of plan_forward that depend on the shard) -------------------
def shard_graph_facts(shard):
    """(largest adjacency in-degree, number of distinct attribute rows) of a shard."""
    ea = int(shard.adj.shape[1])
    deg = int(np.bincount(shard.adj[1], minlength=shard.n_own).max()) if ea else 0
    n_types = int(np.unique(shard.adj_attr, axis=0).shape[0]) if ea else 0
    return deg, n_types


def expected_plan(shard_max_in_degree, n_types, scheme="split", width=32, side_stream=True):
    """plan_forward for a shard whose graph was prepared with edge groups and without type columns (what FusedShardForward.step
    prepares for the one-all-to-all schemes at the default switches): fused_shard, groups_ok, f16, eg, lean_head, split, pack_in_nnconv.
    The all-reduce scheme never takes the fp16 pairs (f16 needs !sharded || fused_shard); per_op runs no forward plan: its NNConv alone
    picks the edge-group kernel under the same in-degree condition (ops.nnconv_mean)."""
    fused_shard = scheme in ONE_ALLTOALL and width == 32
    groups_ok = width == 32 and shard_max_in_degree <= EG_MAX_IN_DEGREE
    if scheme == "per_op":
        return {"eg": groups_ok and shard_max_in_degree >= 1 and n_types >= 1}
    f16 = fused_shard and groups_ok and shard_max_in_degree >= 1
    eg = f16 and groups_ok
    lean_head = f16
    split = fused_shard and scheme != "fused" and side_stream
    return {"fused_shard": fused_shard, "groups_ok": groups_ok, "f16": f16, "eg": eg, "lean_head": lean_head, "split": split,
            "pack_in_nnconv": eg and split and scheme == "split" and lean_head}


def plans_of(kind, scheme="split"):
    c = case(kind)
    return [expected_plan(*shard_graph_facts(s), scheme=scheme, width=c.width) for s in c.shards]


def has_mixed_plans(kind, scheme="split"):
    """Ranks of one forward run different kernels (groups_ok alone changes none: without f16 nobody reads the groups)."""
    plans = [{k: v for k, v in p.items() if k != "groups_ok"} for p in plans_of(kind, scheme)]
    return any(p != plans[0] for p in plans[1:])


# ---- the reference and the gate ------------------------------------------------------------------------------------------------
@contextlib.contextmanager
def _dedup_nnconv(on):
    """oracle.nnconv_mean_dedup (pinned equal to the port) where the plain form's [Ea, C, C] tensor makes the oracle slow."""
    plain = orc.nnconv_mean
    if on:
        orc.nnconv_mean = orc.nnconv_mean_dedup
    try:
        yield
    finally:
        orc.nnconv_mean = plain


def rel(got, want):
    return orc.rel_max_err(got, want)


def _is_running(key):
    return key.endswith(("running_mean", "running_var"))


@dataclass
class Reference:
    kind: str
    depth: int
    sd: dict                           # the fp32 state dict every rank's replica loads
    slots: List[torch.Tensor]          # fp64, [n_total, width] each: middle[0 .. D]
    probs: torch.Tensor
    running: Dict[str, torch.Tensor]   # the fp64 oracle's buffers after update_running
    err32: List[float]
    err32_probs: float
    err32_running: Dict[str, float]

    def gate(self, k):
        return MARGIN * max(self.err32[k], REL_MAX_TOL)

    @property
    def gate_probs(self):
        return MARGIN * max(self.err32_probs, REL_MAX_TOL)

    def gate_running(self, key):
        return MARGIN * max(self.err32_running[key], REL_MAX_TOL)


_REFERENCES: Dict[tuple, Reference] = {}


def reference(kind, depth) -> Reference:
    """Computed once per (kind, depth), shared by every scheme's test, never changed."""
    if (kind, depth) in _REFERENCES:
        return _REFERENCES[(kind, depth)]
    c = case(kind)
    x, adj, attr, col = (torch.from_numpy(np.ascontiguousarray(a)) for a in c.graph)
    sd = make_state_dict(FE, depth, c.width, 1, FX, seed=SEED_NET)
    out = {}
    with torch.no_grad(), _dedup_nnconv(kind == "deg2049"):
        for dtype in (torch.float64, torch.float32):
            cap, sdc = {}, orc.cast_sd(sd, dtype)
            probs, _ = orc.tilingnn_forward(sdc, x.to(dtype), adj, attr.to(dtype), col, update_running=True, capture=cap)
            slots = [cap["init"]] + [cap[f"mid.{k}"] for k in range(1, depth + 1)]
            out[dtype] = (slots, probs, {k: v for k, v in sdc.items() if _is_running(k)})
    s64, p64, r64 = out[torch.float64]
    s32, p32, r32 = out[torch.float32]
    ref = Reference(kind, depth, sd, s64, p64, r64, [rel(a, b) for a, b in zip(s32, s64)], rel(p32, p64),
                    {k: rel(r32[k], r64[k]) for k in r64})
    _REFERENCES[(kind, depth)] = ref
    return ref


def check_against_gate(ref: Reference, slots, probs, label="", rows=None):
    """slots: D + 1 tensors [n_total, width] (None: the scheme keeps no skip buffer), probs [n_total, 1]; prints err / err32 per slot
    and returns the list of (what, err, gate) that exceed the gate.  rows: receives the printed rows."""
    bad = []
    figures = [(f"slot {k}", rel(slots[k], ref.slots[k]), ref.err32[k], ref.gate(k)) for k in range(ref.depth + 1)] if slots is not None else []
    figures.append(("probs", rel(probs, ref.probs), ref.err32_probs, ref.gate_probs))
    for what, err, e32, gate in figures:
        line = "%-34s %-8s err %.3e  err32 %.3e  err/err32 %7.2f  gate %.3e" % (label, what, err, e32, err / max(e32, 1e-300), gate)
        print(line)
        if rows is not None:
            rows.append(line)
        if not err <= gate:
            bad.append((what, err, gate))
    return bad
