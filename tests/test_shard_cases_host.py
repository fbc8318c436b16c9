"""tests/shard_cases.py on the CPU: every kind has the partition it is named for (asserted on the Shard objects), the Python schedule
of tilingnn_amd.dist over the oracle backend equals the fp64 oracle on it, the gate accepts a plain fp32 implementation of the sharded
forward and rejects three mutants of the halo exchange, and the plan restatement finds ranks on different plans in exactly the two
kinds built for it.  So a failure of tests/test_shard_shapes.py on these shapes is the device path's."""
import numpy as np
import pytest
import torch

from tests import shard_cases as sc
from tests.dist_cpu_backend import OracleBackend
from tests.test_dist_cpu import _param_holder
from tilingnn_amd import dist as tdist

ALL_KINDS = sc.KINDS + ("width64",)


# ---- preconditions ---------------------------------------------------------------------------------------------------------------
def _halo(s):
    return s.n_rows - s.n_own


def _send(s):
    return [int(a.shape[0]) for a in s.send_ids]


@pytest.mark.parametrize("kind", ALL_KINDS)
def test_shards_partition_the_graph(kind):
    """The identities of tests/test_dist_cpu.py::test_shards_partition_the_graph, on every kind (tiny: against the sub-layout)."""
    c = sc.case(kind)
    x, adj, attr, col = c.graph
    n, world = x.shape[0], c.world
    shards = c.shards
    bounds = shards[0].bounds
    assert sum(s.n_own for s in shards) == n and all(s.n_total == n for s in shards)
    assert sum(s.adj.shape[1] for s in shards) == adj.shape[1]
    assert sum(s.col.shape[1] for s in shards) == col.shape[1]
    for s in shards:
        lo, hi = tdist.node_range(n, s.rank, world, bounds)
        assert (s.lo, s.n_own) == (lo, hi - lo)
        glob = np.concatenate([np.arange(lo, hi), s.halo_ids])
        for loc, full, feat in ((s.adj, adj, attr), (s.col, col, None)):
            keep = (full[1] >= lo) & (full[1] < hi)
            np.testing.assert_array_equal(glob[loc[0]], full[0][keep])       # local ids map back to the global edges, in global order
            np.testing.assert_array_equal(loc[1] + lo, full[1][keep])
            if feat is not None:
                np.testing.assert_array_equal(s.adj_attr, feat[keep])
        np.testing.assert_array_equal(s.x, x[lo:hi])
        assert ((s.halo_ids < lo) | (s.halo_ids >= hi)).all() and sum(s.recv_counts) == s.halo_ids.shape[0]
        owners = tdist.owner_of(s.halo_ids, n, world, bounds)
        assert (np.diff(owners) >= 0).all() and (np.diff(s.halo_ids) > 0).all()
        assert s.recv_counts == [int(np.count_nonzero(owners == p)) for p in range(world)]
        for p in range(world):                                               # what p sends me == my halo rows owned by p
            np.testing.assert_array_equal(shards[p].send_ids[s.rank] + shards[p].lo, s.halo_ids[owners == p])
    # the attribute rows: 13 one-hot types, the edge order is not sorted by destination
    assert np.unique(attr, axis=0).shape[0] == sc.N_TYPES and (np.diff(adj[1]) < 0).any() and (np.diff(col[1]) < 0).any()


def test_islands():
    s = sc.case("islands").shards
    for r in (1, 3):
        assert _halo(s[r]) == 0 and sum(_send(s[r])) == 0 and s[r].recv_counts == [0, 0, 0, 0]
    for r, peer in ((0, 2), (2, 0)):
        assert s[r].recv_counts[peer] > 0 and _halo(s[r]) == s[r].recv_counts[peer] and _send(s[r])[peer] > 0
        assert s[r].recv_counts[1] == 0 and _send(s[r])[1] == 0                # they exchange ACROSS rank 1
    assert all(s[r].adj.shape[1] > 0 and s[r].col.shape[1] > 0 for r in range(4))


@pytest.mark.parametrize("kind", ["one_way", "width64"])
def test_one_way(kind):
    c = sc.case(kind)
    s, last = c.shards, c.world - 1
    assert _halo(s[last]) == 0 and sum(_send(s[last])) > 0
    assert sum(_send(s[0])) == 0 and _halo(s[0]) > 0
    for r in range(c.world):
        assert all(k == 0 for p, k in enumerate(s[r].recv_counts) if p != r + 1)      # every cross edge runs from r + 1 into r
    assert c.width == (64 if kind == "width64" else 32)


def test_hub():
    c = sc.case("hub")
    s, world = c.shards, c.world
    row = sc.HUB_SOURCE_ROW
    assert all(row in s[2].send_ids[p] for p in range(world) if p != 2)              # sent to world - 1 peers
    counts = np.bincount(np.concatenate(s[2].send_ids), minlength=s[2].n_own)        # what FusedShardForward's send_row_ptr counts
    assert counts[row] == world - 1 == counts.max()
    assert _halo(s[0]) > 2 * s[0].n_own
    deg = np.bincount(s[0].adj[1], minlength=s[0].n_own)
    assert deg[5] >= sc.HUB_FAN_IN and np.unique(s[0].adj[0][s[0].adj[1] == 5]).shape[0] >= sc.HUB_FAN_IN


def test_branch_missing():
    s = sc.case("branch_missing").shards
    assert s[1].adj.shape[1] == 0 and s[1].adj_attr.shape == (0, sc.FE) and sc.shard_graph_facts(s[1]) == (0, 0)
    assert s[1].col.shape[1] > 0 and sum(_send(s[1])) > 0 and _halo(s[1]) > 0        # a source for others, a reader of others
    assert s[3].col.shape[1] == 0 and s[3].adj.shape[1] > 0 and sum(_send(s[3])) > 0
    assert all(s[r].adj.shape[1] > 0 and s[r].col.shape[1] > 0 for r in (0, 2))


def test_deg2049():
    c = sc.case("deg2049")
    s = c.shards
    assert all(x.n_own == 704 for x in s) and c.graph[0].shape[0] == 2816
    degs = [np.bincount(x.adj[1], minlength=x.n_own) for x in s]
    assert int(degs[1].max()) == 2049 == sc.EG_MAX_IN_DEGREE + 1 and int(np.sort(degs[1])[-2]) <= 16
    g = int(degs[1].argmax())
    assert np.unique(s[1].adj[0][s[1].adj[1] == g]).shape[0] == 2049                 # distinct sources
    assert all(int(degs[r].max()) <= 16 for r in (0, 2, 3)) and all(int(d.min()) >= 1 for d in degs)
    assert all(_halo(x) > 0 and sum(_send(x)) > 0 for x in s)
    assert max(x.n_total for x in s) <= 2816


def test_tiny():
    c = sc.case("tiny")
    s = c.shards
    assert tuple(x.n_own for x in s) == sc.TINY_RANGES and int(c.alive.sum()) == sum(sc.TINY_RANGES) == s[0].n_total
    assert _halo(s[0]) > 4 * s[0].n_own                                              # 2 rows behind a much larger halo
    assert all(x.adj.shape[1] > 0 and x.col.shape[1] > 0 for x in s)
    assert all(x.bounds is not None and list(np.diff(x.bounds)) == list(sc.TINY_RANGES) for x in s)
    assert sum(_send(s[0])) >= 0 and sum(_halo(x) for x in s) == sum(sum(_send(x)) for x in s)
    # the numpy compaction is the sub-layout's own partition: shards cut straight from the sub-layout's bounds agree
    np.testing.assert_array_equal(np.concatenate([x.x for x in s]), c.graph[0])


# ---- the schedule and the gate ----------------------------------------------------------------------------------------------------
class Recorder(OracleBackend):
    """The oracle backend keeping every skip-buffer slot of its rank; `mutate`: a fault in the rows this rank packs for the exchange
    behind layer 0 (the third pack of a forward: middle[0], then middle[1] and the collision branch's rows)."""

    def __init__(self, dtype, mutate=None, dedup_rows=False):
        super().__init__(dtype, dedup_rows=dedup_rows)
        self.slots, self.mutate, self.packs = [], mutate, 0

    def bn_apply(self, v, stat):
        out = super().bn_apply(v, stat)
        self.slots.append(out.clone())
        return out

    def merge(self, a1, s1, a2, s2, resid, out):
        super().merge(a1, s1, a2, s2, resid, out)
        self.slots.append(out.clone())

    def pack_rows(self, src, idx, out, col_offset):
        super().pack_rows(src, idx, out, col_offset)
        self.packs += 1
        if self.mutate and self.packs == 3:
            assert idx.numel() >= 2
            if self.mutate == "zeroed":
                out[0] = 0
            elif self.mutate == "swapped":
                out[[0, 1]] = out[[1, 0]]
            elif self.mutate == "scaled":
                out[0] *= 1 + 1e-3


def _run(kind, depth, dtype, mutate=None, mutant_rank=1):
    c = sc.case(kind)
    ref = sc.reference(kind, depth)
    net = _param_holder(ref.sd, depth, c.width, sc.FE, sc.FX)
    backends = [Recorder(dtype, mutate if r == mutant_rank else None, dedup_rows=kind == "deg2049") for r in range(c.world)]
    parts = tdist.LocalSimComm.run([tdist.ShardProgram(net, s, b, update_running=False) for s, b in zip(c.shards, backends)])
    slots = [torch.cat([b.slots[k] for b in backends]) for k in range(depth + 1)]
    return ref, slots, torch.cat(parts)


@pytest.mark.parametrize("kind", ALL_KINDS)
def test_python_schedule_equals_the_fp64_oracle(kind):
    ref, slots, probs = _run(kind, 3, torch.float64)
    assert probs.shape == ref.probs.shape and float((probs - ref.probs).abs().max()) < 1e-9
    for k in range(4):
        assert slots[k].shape == ref.slots[k].shape and sc.rel(slots[k], ref.slots[k]) < 1e-9, k


@pytest.mark.parametrize("kind,depth", sc.REFERENCE_ROWS)
def test_gate_accepts_a_plain_fp32_implementation(kind, depth):
    ref, slots, probs = _run(kind, depth, torch.float32)
    assert all(e > 0 for e in ref.err32) and ref.err32_probs > 0
    assert sc.check_against_gate(ref, slots, probs, f"{kind} depth {depth} fp32 oracle backend") == []


@pytest.mark.parametrize("mutant", ["zeroed", "swapped", "scaled"])
def test_gate_rejects_a_wrong_halo_row(mutant):
    """One rank's message behind layer 0, one row wrong: some slot is more than 10 x over its gate."""
    ref, slots, probs = _run("one_way", 3, torch.float32, mutate=mutant)
    over = [sc.rel(slots[k], ref.slots[k]) / ref.gate(k) for k in range(4)]
    print(mutant, ["%.1f" % v for v in over])
    assert over[0] < 1 and over[1] < 1                  # the fault enters behind slot 1
    assert max(over) > 10


# ---- plans -----------------------------------------------------------------------------------------------------------------------
def test_expected_plan_terms():
    on = sc.expected_plan(16, 13, "split")
    assert on == {"fused_shard": True, "groups_ok": True, "f16": True, "eg": True, "lean_head": True, "split": True, "pack_in_nnconv": True}
    assert sc.expected_plan(2048, 13, "split") == on and not sc.expected_plan(16, 13, "split_nopack")["pack_in_nnconv"]
    off = sc.expected_plan(0, 0, "split")                                    # f16 needs max_in_degree >= 1
    assert off["groups_ok"] and off["split"] and not (off["f16"] or off["eg"] or off["lean_head"] or off["pack_in_nnconv"])
    over = sc.expected_plan(2049, 13, "split")                               # groups_ok needs <= 2 048
    assert not (over["groups_ok"] or over["f16"] or over["eg"] or over["lean_head"] or over["pack_in_nnconv"]) and over["split"]
    assert not sc.expected_plan(16, 13, "fused")["split"] and sc.expected_plan(16, 13, "fused")["f16"]
    assert [k for k, v in sc.expected_plan(16, 13, "allreduce").items() if v] == ["groups_ok"]
    assert not any(sc.expected_plan(16, 13, "split", width=64).values())     # width 64: the all-reduce scheme whatever was asked
    assert sc.expected_plan(16, 13, "per_op") == {"eg": True} and sc.expected_plan(2049, 13, "per_op") == {"eg": False}


@pytest.mark.parametrize("kind", ALL_KINDS)
def test_mixed_plans_occur_where_they_are_built_in(kind):
    mixed = kind in ("branch_missing", "deg2049")
    for scheme in sc.ONE_ALLTOALL:
        assert sc.has_mixed_plans(kind, scheme) == mixed, scheme
    assert not sc.has_mixed_plans(kind, "allreduce")
    if kind == "branch_missing":
        plans = sc.plans_of(kind, "split")
        assert [p["f16"] for p in plans] == [True, False, True, True] and [p["pack_in_nnconv"] for p in plans] == [True, False, True, True]
    if kind == "deg2049":
        plans = sc.plans_of(kind, "split")
        assert [p["eg"] for p in plans] == [True, False, True, True] and [p["groups_ok"] for p in plans] == [True, False, True, True]


def test_case_table():
    t = sc.CASE_TABLE
    assert len(t) == len(set(t)) == 6 * 5 + 4 + 2
    assert {(k, s) for k, s, d in t if d == 3 and k != "width64"} == {(k, s) for k in sc.KINDS for s in sc.SCHEMES}
    assert {(k, s) for k, s, d in t if d == 20} == {(k, s) for k in ("one_way", "branch_missing") for s in ("fused", "split")}
    assert {s for k, s, d in t if k == "width64"} == {"allreduce", "per_op"}
