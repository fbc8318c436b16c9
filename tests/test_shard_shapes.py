"""The sharded device forward (tilingnn_amd.dist: FusedShardForward -> tgnn_forward_sharded, and ShardProgram over HipBackend) at the
partitions of tests/shard_cases.py -- uneven, one-way, empty, one rank on another plan than its peers -- against the fp64 oracle on the
global graph.  Virtual ranks on one GPU: a thread per rank over dist.ThreadSimCollectives (per_op: LocalSimComm), every rank with its
own replica of the net.  The gate is shard_cases' (4 x the fp32 oracle's own error per slot, floor 2e-6); its derivation is there, and
tests/test_shard_cases_host.py shows on the CPU that a plain fp32 implementation passes it and a wrong halo row does not.

Per row of the case table: owned rows of every slot and the probabilities within the gate; the halo rows of slots k < D bit for bit the
owning rank's rows (copies in the all-reduce scheme and per_op's buffers; in the one-all-to-all schemes every rank merges its halo rows
itself from the raw rows and the rank-ordered sums -- the same arithmetic on the same numbers); BatchNorm buffers bit-identical on all
ranks, updated once, rank 0's within the gate of the oracle's; on ranks that take the fp16 pairs the slots' bound words are the exact
maxima over the rows the rank gathers (halo rows included, 0 of them too).

One measured run of the table: profiles/shard_shapes_errors.txt."""
import ctypes as C

import numpy as np
import pytest
import torch

from tests import shard_cases as sc
from tests.test_forward_bounds import _bits, _slots, _words
from tests.test_hip_parity import make_net, run_thread_ranks

pytestmark = pytest.mark.gpu

_TABLE = []
_TINY = {}


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "GPU tests need a GPU"
    return torch.device("cuda:0")


@pytest.fixture(scope="module", autouse=True)
def error_table():
    yield
    if _TABLE:
        print("\n# sharded forward against the fp64 oracle: err = max |got - want| / max |want| over the owned rows of all ranks; err32 = the fp32 oracle's")
        for line in _TABLE:
            print(line)


def _assert_same_shard(got, inp, want):
    """tests/test_sharded_solve.py::test_device_shard_compaction_equals_the_numpy_one's comparison, send lists included."""
    assert (got.n_total, got.lo, got.n_own, got.recv_counts) == (want.n_total, want.lo, want.n_own, want.recv_counts)
    np.testing.assert_array_equal(got.halo_ids, want.halo_ids)
    np.testing.assert_array_equal(got.bounds, want.bounds)
    np.testing.assert_array_equal(inp["x"].cpu().numpy(), want.x.astype(np.float32))
    np.testing.assert_array_equal(inp["adj"].cpu().numpy(), want.adj)
    np.testing.assert_array_equal(inp["attr"].cpu().numpy(), want.adj_attr.astype(np.float32))
    np.testing.assert_array_equal(inp["col"].cpu().numpy(), want.col)
    assert len(got.send_ids) == len(want.send_ids)
    for a, b in zip(got.send_ids, want.send_ids):
        np.testing.assert_array_equal(a, b)
    np.testing.assert_array_equal(inp["send_idx"].cpu().numpy(), np.concatenate(want.send_ids).astype(np.int32))


def _device_shards(kind, dev):
    """(shards, their inputs in HBM).  tiny: cut by the device (compact_shard_device + setup + refresh_send_idx), held equal to numpy's."""
    from tilingnn_amd import dist as tdist
    c = sc.case(kind)
    be = tdist.HipBackend(dev)
    if kind != "tiny":
        return c.shards, [be.upload(s) for s in c.shards]
    if not _TINY:
        cut = [tdist.compact_shard_device(s, be.upload(s), c.alive) for s in c.base_shards]
        shards, inputs = [s for s, _ in cut], [inp for _, inp in cut]
        tdist.LocalSimComm.setup(shards)
        for s, inp in zip(shards, inputs):
            tdist.refresh_send_idx(s, inp)
        for got, inp, want in zip(shards, inputs, c.shards):
            _assert_same_shard(got, inp, want)
        _TINY["cut"] = (shards, inputs)
    return _TINY["cut"]


def _running(net):
    return {k: v.detach().cpu() for k, v in net.state_dict().items()
            if k.endswith(("running_mean", "running_var", "num_batches_tracked")) and ".nnConv.nn." not in k}


@pytest.mark.parametrize("kind,scheme,depth", sc.CASE_TABLE)
def test_sharded_forward_against_the_fp64_oracle(dev, general_schedule, kind, scheme, depth):
    from tilingnn_amd import _lib
    from tilingnn_amd import dist as tdist
    c = sc.case(kind)
    ref = sc.reference(kind, depth)
    world, width = c.world, c.width
    shards, inputs = _device_shards(kind, dev)
    facts = [sc.shard_graph_facts(s) for s in c.shards]
    plans = [sc.expected_plan(*f, scheme=scheme, width=width) for f in facts]
    nets = [make_net(dev, depth=depth, width=width, seed=sc.SEED_NET)[0] for _ in range(world)]     # every rank holds its own replica
    label = f"{kind} {scheme} depth {depth}"
    own = [s.n_own for s in shards]
    bad = []                                             # everything that is wrong with this case, asserted empty at the end

    if scheme == "per_op":
        be = tdist.HipBackend(dev)
        programs = [tdist.ShardProgram(nets[r], shards[r], be, inputs=inputs[r]) for r in range(world)]
        parts = tdist.LocalSimComm.run(programs)
        torch.cuda.synchronize()
        slots = None
        # no workspace: the gathered adjacency-branch buffer holds the last EXCHANGED slot, middle[D - 1], halo rows included
        full = torch.cat([p.h1[:n] for p, n in zip(programs, own)])
        for p, s in zip(programs, shards):
            if not torch.equal(p.h1[s.n_own:], full[torch.from_numpy(s.halo_ids).to(dev)]):
                bad.append(("halo rows of slot", depth - 1, "rank", s.rank))
        if not sc.rel(full.cpu(), ref.slots[depth - 1]) <= ref.gate(depth - 1):
            bad.append((f"slot {depth - 1}", sc.rel(full.cpu(), ref.slots[depth - 1]), ref.gate(depth - 1)))
    else:
        hub = tdist.ThreadSimCollectives.Hub(world)
        runners = [tdist.FusedShardForward(nets[r], shards[r], dev, tdist.ThreadSimCollectives(hub, r), inputs=inputs[r],
                                           fused=scheme != "allreduce") for r in range(world)]
        assert all(rn.fused == (scheme in sc.ONE_ALLTOALL and width == 32) for rn in runners)
        if scheme in ("split", "split_nopack"):
            assert _lib.side_stream(dev).value, "no side stream: the split exchange is not taken"
        for rn in runners:
            rn.two_streams = scheme in ("split", "split_nopack")
            rn.pack_in_nnconv = scheme != "split_nopack"
        c0 = _lib.forward_path_counts()
        parts = run_thread_ranks(dev, runners, hub)
        assert _lib.forward_path_counts()[0] == c0[0] + world
        code = C.c_uint32(0)
        _lib.check(_lib.lib.tgnn_spin_error_poll(_lib.current_stream(dev), C.byref(code)))
        assert code.value == 0
        assert [rn.n_types for rn in runners] == [f[1] for f in facts]
        dims = nets[0]._dims()
        maps = [_lib.forward_workspace_map(dims, s.n_own, s.n_rows, rn.n_types) for s, rn in zip(shards, runners)]
        per_rank = [_slots(rn.workspace, m, s.n_rows, depth, c=width) for s, rn, m in zip(shards, runners, maps)]
        slots = [torch.cat([w[k, :n] for w, n in zip(per_rank, own)]) for k in range(depth + 1)]
        # ---- halo rows: the owning rank's own rows, bit for bit (the last slot's are nobody's)
        for s, w in zip(shards, per_rank):
            ids = torch.from_numpy(s.halo_ids).to(dev)
            for k in range(depth):
                if not torch.equal(w[k, s.n_own:], slots[k][ids]):
                    bad.append(("halo rows of slot", k, "rank", s.rank, "rows that differ", int((w[k, s.n_own:] != slots[k][ids]).any(dim=1).sum())))
        # ---- ranks on the fp16 pairs: word k of the workspace is the exact maximum over the rows the rank gathers
        for s, rn, m, w, plan in zip(shards, runners, maps, per_rank, plans):
            if plan["f16"]:
                words = _words(rn.workspace, m, depth)
                for k in range(depth + 1):
                    rows = s.n_rows if k < depth else s.n_own
                    if words[k] != _bits(w[k, :rows].abs().max()):
                        bad.append(("bound word", k, "rank", s.rank))
        slots = [t.cpu() for t in slots]

    assert len(parts) == world and all(p.shape == (n, 1) and bool(torch.isfinite(p).all()) for p, n in zip(parts, own))
    probs = torch.cat(parts).cpu()
    print()
    _TABLE.append("%s: rows %s halo %s send %s ea %s ec %s plans %s" % (
        label, own, [s.n_rows - s.n_own for s in shards], [sum(len(a) for a in s.send_ids) for s in shards],
        [int(i["adj"].shape[1]) for i in inputs], [int(i["col"].shape[1]) for i in inputs],
        ["+".join(k for k, v in p.items() if v and k not in ("fused_shard", "groups_ok")) or "fp32" for p in plans]))
    bad += sc.check_against_gate(ref, slots, probs, label, rows=_TABLE)

    # ---- running statistics: the same bits on every rank (sums added in rank order everywhere), one update, rank 0's against the oracle's
    stats = [_running(n) for n in nets]
    assert stats[0] and all(set(st) == set(stats[0]) for st in stats)
    for key, v in stats[0].items():
        for r in range(1, world):
            assert torch.equal(stats[r][key], v), (key, "rank", r)
        if key.endswith("num_batches_tracked"):
            assert int(v) == 1, key
        else:
            err = sc.rel(v, ref.running[key])
            if not err <= ref.gate_running(key):
                bad.append((key, err, ref.gate_running(key)))
    assert bad == [], bad
