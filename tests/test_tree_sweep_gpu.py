"""The branch sweeps of the tree search on the device, raw: tgnn_tree_sweep_many (csrc/tree_sweep.hip) through
`CompleteGraphOnDevice.tree_sweep_into`.  Every sweep call of three restated searches on the small graph
(tests/tree_search_restatement.py, the configurations of tests/test_tree_search_host.py) is replayed: trace, stats, accepted,
killed and the four rows of every child slot afterwards, every other slot untouched, and d holes of every evaluated position
against ONE tgnn_union_hole_delta call over the prefix masks.  Then the fork, the bytes (nine branches in one call on dirty outputs
and workspaces against nine solo calls), graphs either side of the LDS limit, the sweep without geometry, a labelled first
position, the error bits and the refusals.  Every comparison is exact integer equality.  The per-visit rule itself runs on the
host under sanitizers in tests/test_tree_search_host.py."""
import functools
import math
import os

import numpy as np
import pytest
import torch

from tests import hole_delta_cases as hc
from tests import topology_oracle as to
from tests import tree_search_restatement as ts
from tests.golden_util import GOLDEN
from tests.test_tree_search_host import CONFIGS, restated

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
NOT_REACHED, BREAK, VETOED, REJECTED, ACCEPTED, SKIPPED = range(6)
UNKNOWN = -2 ** 31


def _made_up_graph(tiles):
    """A CompleteGraphOnDevice over hand-made tiles (no TileGraph behind it), as tests/test_hole_sweep_gpu.py makes one."""
    from tilingnn_amd.tiling.region import contact_geometry, sweep_direction, union_geometry
    from tilingnn_amd.util.data_util import CompleteGraphOnDevice
    n = len(tiles)
    geo = union_geometry(tiles, np.zeros((2, 0), dtype=np.int64), n)
    touch = contact_geometry(geo[0], geo[1])
    theta = sweep_direction(geo[0], geo[1])
    od = CompleteGraphOnDevice.__new__(CompleteGraphOnDevice)
    od.device, od.n_tiles = torch.device(DEV), n
    up = lambda a: torch.from_numpy(a if a.size else np.zeros(1, dtype=a.dtype)).to(DEV)
    od._union = tuple(up(a) for a in geo)
    od._topology = tuple(up(a) for a in touch) + (math.cos(theta), math.sin(theta))
    return od


class Harness:
    """A pool of `n_slots` states of ONE layout and one call per step, straight from arrays.  tile_of: the tile of every node;
    col: collision edges [2, E].  Outputs and the workspace are filled with the byte `fill` before every call: what is read must
    be written; `guards_intact`: the two words of it behind the accepted and behind the killed list were still that byte after
    the last call.  geometry=False: no tile state (check_holes == 0)."""

    def __init__(self, od, tile_of, col, n_slots, geometry=True):
        self.od, self.s, self.n, self.geometry = od, n_slots, len(tile_of), geometry
        n = self.n
        col = np.asarray(col).reshape(2, -1)
        by_src = np.argsort(col[0], kind="stable")                          # (HostSweep.__init__)
        nbr_ptr = np.searchsorted(col[0][by_src], np.arange(n + 1))
        nbr = col[1][by_src]
        self.n_nbr = int(nbr.shape[0])
        up = lambda a: torch.from_numpy(np.ascontiguousarray(a, dtype=np.int32)).to(DEV)
        self.tile_of_node = up(tile_of)
        self.nbr_ptr, self.nbr_idx = up(nbr_ptr), up(nbr if self.n_nbr else np.zeros(1))
        self.unlabelled = torch.ones(n_slots, n, dtype=torch.int32, device=DEV)
        self.tile_alive = self.label = self.chi_cache = None
        if geometry:
            self.tile_alive = torch.zeros(n_slots, od.n_tiles, dtype=torch.int32, device=DEV)
            self.label = torch.full((n_slots, od.n_tiles), -1, dtype=torch.int32, device=DEV)
            self.chi_cache = torch.full((n_slots, od.n_tiles), UNKNOWN, dtype=torch.int32, device=DEV)

    def state(self):
        rows = (self.unlabelled, self.tile_alive, self.label, self.chi_cache) if self.geometry else (self.unlabelled,)
        return tuple(t.cpu().numpy().copy() for t in rows)

    def call(self, parents, slots, visits, p, u, check_holes=1, fill=0xF9):
        """visits / p / u: per branch the visiting order (nodes), prob_m by position and uniforms.  -> dict of numpy outputs."""
        from tilingnn_amd._lib import lib
        from tilingnn_amd.util.data_util import tree_sweep_call
        k = len(parents)
        visit_ptr = np.concatenate([[0], np.cumsum([len(v) for v in visits])]).astype(np.int32)
        v = int(visit_ptr[-1])
        cat = lambda parts, dt: torch.from_numpy(np.concatenate([np.asarray(x, dtype=dt) for x in parts] + [np.zeros(1, dtype=dt)])).to(DEV)
        dirty = lambda count: torch.full((4 * max(count, 1),), fill, dtype=torch.uint8, device=DEV).view(torch.int32)
        out = {"stats": dirty(8 * k), "err": dirty(k), "accepted": dirty(v + 2), "killed": dirty(v + 2), "trace": dirty(2 * v)}
        ws = dirty(int(lib.tgnn_tree_sweep_workspace_bytes(k)) // 4)
        i32 = lambda a: torch.from_numpy(np.asarray(a, dtype=np.int32)).to(DEV)
        args = (self.n, self.tile_of_node if self.geometry else None, self.nbr_ptr, self.nbr_idx, self.n_nbr, self.s, self.unlabelled,
                self.tile_alive, self.label, self.chi_cache, k, i32(parents), i32(slots), i32(visit_ptr), cat(visits, np.int32),
                cat(p, np.float64), cat(u, np.float64), v, check_holes, out["stats"], out["accepted"], out["killed"], out["trace"],
                out["err"], ws)
        if self.geometry:
            self.od.tree_sweep_into(*args)
        else:
            tree_sweep_call(torch.device(DEV), None, *args)
        torch.cuda.synchronize()
        res = {name: t.cpu().numpy() for name, t in out.items()}
        self.guards_intact = all((res[name][v:].view(np.uint8) == fill).all() for name in ("accepted", "killed"))
        res["stats"], res["trace"], res["visit_ptr"] = res["stats"][:8 * k].reshape(k, 8), res["trace"][:2 * v].reshape(v, 2), visit_ptr
        res["accepted"], res["killed"], res["err"] = res["accepted"][:v], res["killed"][:v], res["err"][:k]
        return res


class Fixture:
    def __init__(self, graph):
        from tilingnn_amd.util.data_util import graph_on_device
        self.graph = graph
        self.rings = [np.asarray(t.tile_poly.exterior)[:-1] for t in graph.tiles]
        self.n = len(graph.tiles)
        self.col = graph.arrays.colli_edges
        self.on_device = graph_on_device(graph, DEV)
        self.touch_ptr, self.touch_idx = (t.cpu().numpy() for t in self.on_device._topology_geometry()[:2])


@pytest.fixture(scope="module")
def small():
    from tilingnn_amd.tiling.tile_graph import TileGraph
    g = TileGraph(2)
    g.load_graph_state(os.path.join(GOLDEN, "complete_graph_small.pkl"), sidecar=False)
    return Fixture(g)


def _labels(fx, selected):
    """-1 for a dead tile, else the lowest alive tile of its component (tiles that share a point are connected)."""
    alive = np.zeros(fx.n, dtype=bool)
    alive[selected] = True
    parent = list(range(fx.n))

    def find(a):
        while parent[a] != a:
            parent[a] = parent[parent[a]]
            a = parent[a]
        return a

    for i in np.flatnonzero(alive):
        for j in fx.touch_idx[fx.touch_ptr[i]:fx.touch_ptr[i + 1]]:
            if alive[j]:
                a, b = find(int(i)), find(int(j))
                if a != b:
                    parent[max(a, b)] = min(a, b)
    return np.array([find(i) if alive[i] else -1 for i in range(fx.n)], dtype=np.int32)


# ------------------------------------------------------------------------------------------------ the restated searches, replayed
@pytest.mark.parametrize("config", range(3))
@pytest.mark.parametrize("seed", range(3))
def test_every_sweep_call_of_a_restated_search(small, config, seed):
    fx, cfg = small, CONFIGS[config]
    s = restated(fx.rings, fx.col, cfg, seed)
    reuse = cfg["top_k"] == 1                                                # one child per parent: it takes its parent's slot
    n_states = cfg["roots"] + sum(len(step) for step in s.steps)
    run = Harness(fx.on_device, np.arange(fx.n), fx.col, cfg["roots"] if reuse else n_states)
    slot_of = {uid: uid for uid in range(cfg["roots"])}
    selected = {uid: [] for uid in range(cfg["roots"])}
    evaluated, masks, mask_row = [], [], {}
    calls = 0
    for step in s.steps:
        for br in step:
            slot_of[br.uid] = slot_of[br.parent] if reuse else br.uid
        before = run.state()
        out = run.call([slot_of[b.parent] for b in step], [slot_of[b.uid] for b in step], [b.nodes for b in step], [b.p for b in step],
                       [b.u for b in step], check_holes=int(cfg["check_holes"]))
        calls += 1
        after = run.state()
        children = [slot_of[b.uid] for b in step]
        others = np.setdiff1d(np.arange(run.s), children)
        assert all((x[others] == y[others]).all() for x, y in zip(before, after))            # parents that are not reused, and every bystander
        for k, br in enumerate(step):
            v0, v1 = int(out["visit_ptr"][k]), int(out["visit_ptr"][k + 1])
            trace, reached = out["trace"][v0:v1], len(br.trace)
            assert out["err"][k] == 0
            assert trace[:reached, 0].tolist() == [code for code, _ in br.trace]
            assert br.nodes[:reached].tolist() == [node for _, node in br.trace]
            assert (trace[reached:] == 0).all()
            assert out["stats"][k].tolist() == [reached, br.vetoes, br.draws, len(br.accepted), len(br.killed), br.skipped, 0, 0]
            assert out["accepted"][v0:v1].tolist() == br.accepted + [-1] * (v1 - v0 - len(br.accepted))
            assert out["killed"][v0:v1].tolist() == br.killed + [-1] * (v1 - v0 - len(br.killed))
            child = slot_of[br.uid]
            assert (after[0][child] != 0).tolist() == br.unlabelled.tolist()
            alive = np.zeros(fx.n, dtype=np.int32)
            alive[br.selected] = 1
            assert (after[1][child] == alive).all() and (after[2][child] == _labels(fx, br.selected)).all()
            # the selection before every evaluated position, for the map
            chosen = list(selected[br.parent])
            for (code, node), (_, d) in zip(br.trace, trace):
                if code in (VETOED, ACCEPTED):
                    key = tuple(sorted(chosen))
                    if key not in mask_row:
                        mask_row[key] = len(masks)
                        masks.append(key)
                    evaluated.append((mask_row[key], node, code, int(d)))
                if code == ACCEPTED:
                    chosen.append(node)
            assert chosen == br.selected
            selected[br.uid] = chosen
    rows = np.zeros((len(masks), fx.n), dtype=np.int32)
    for r, tiles in enumerate(masks):
        rows[r, list(tiles)] = 1
    delta, state = (t.cpu().numpy() for t in fx.on_device.hole_deltas(torch.from_numpy(rows).to(DEV)))      # ONE call
    for r, node, code, d in evaluated:
        assert state[r, node] == 0                                          # a candidate of that mask
        if cfg["check_holes"]:
            assert d == delta[r, node, 1] and (code == VETOED) == (d > 0)
        else:
            assert d == 0 and code == ACCEPTED
    assert calls == len(s.steps)
    print(f"\ntree sweep replay config {config} seed {seed}: {calls} calls, {sum(len(x) for x in s.steps)} branches, "
          f"{len(evaluated)} evaluated positions on {len(masks)} selections")


# ------------------------------------------------------------------------------------------------ the fork and the bytes
def _a_state_and_nine_branches(fx, run):
    """Slot 0 after one sweep from the empty selection (so the branches meet labelled nodes, tiles and cache entries), and nine
    branches from it with their own orders, probabilities and uniforms."""
    rng = np.random.default_rng(9)
    first = rng.permutation(fx.n)
    out = run.call([0], [0], [first], [np.full(fx.n, 0.5)], [rng.random(fx.n)])
    assert out["err"][0] == 0 and out["stats"][0][3] > 0
    ids = np.flatnonzero(run.state()[0][0])
    assert 0 < ids.size < fx.n
    branches = []
    for _ in range(9):
        order = rng.permutation(ids)
        branches.append((order, rng.random(ids.size) * 1.2, rng.random(ids.size)))
    return branches


def test_a_child_in_its_parents_slot_is_a_child_in_a_fresh_slot(small):
    fx = small
    a, b = (Harness(fx.on_device, np.arange(fx.n), fx.col, 4) for _ in range(2))
    branch = _a_state_and_nine_branches(fx, a)[0]
    _a_state_and_nine_branches(fx, b)
    parent = b.state()
    in_place = a.call([0], [0], [branch[0]], [branch[1]], [branch[2]])
    fresh = b.call([0], [3], [branch[0]], [branch[1]], [branch[2]])
    assert all(in_place[name].tobytes() == fresh[name].tobytes() for name in in_place) and in_place["stats"][0][3] > 0
    sa, sb = a.state(), b.state()
    assert all((x[0] == y[3]).all() for x, y in zip(sa, sb))                # the child's four rows
    assert all(x[:3].tobytes() == y[:3].tobytes() for x, y in zip(parent, sb))      # the parent and the bystanders: byte for byte


def test_nine_branches_in_one_call_are_nine_solo_calls_on_any_bytes(small):
    fx = small
    batches = [Harness(fx.on_device, np.arange(fx.n), fx.col, 10) for _ in range(3)]
    solos = [Harness(fx.on_device, np.arange(fx.n), fx.col, 10) for _ in range(9)]
    branches = _a_state_and_nine_branches(fx, batches[0])
    for h in batches[1:] + solos:
        _a_state_and_nine_branches(fx, h)
    visits, p, u = ([b[i] for b in branches] for i in range(3))
    outs = [h.call([0] * 9, list(range(1, 10)), visits, p, u, fill=fill) for h, fill in zip(batches, (0x00, 0x7F, 0xFF))]
    for other, h in zip(outs[1:], batches[1:]):
        assert all(other[name].tobytes() == outs[0][name].tobytes() for name in outs[0])
        assert all(x.tobytes() == y.tobytes() for x, y in zip(h.state(), batches[0].state()))
    after, ptr = batches[0].state(), outs[0]["visit_ptr"]
    vetoes = skips = 0
    for k in range(9):
        one = solos[k].call([0], [k + 1], [visits[k]], [p[k]], [u[k]], fill=0x33)
        v0, v1 = int(ptr[k]), int(ptr[k + 1])
        assert one["err"][0] == 0 and outs[0]["err"][k] == 0 and (one["stats"][0] == outs[0]["stats"][k]).all()
        assert (one["trace"] == outs[0]["trace"][v0:v1]).all()
        assert (one["accepted"] == outs[0]["accepted"][v0:v1]).all() and (one["killed"] == outs[0]["killed"][v0:v1]).all()
        assert all((x[k + 1] == y[k + 1]).all() for x, y in zip(solos[k].state(), after))       # the cache is part of the state
        vetoes += int(one["stats"][0][1])
        skips += int(one["stats"][0][5])
    assert vetoes > 0 and skips > 0


# ------------------------------------------------------------------------------------------------ either side of the LDS limit
@functools.lru_cache(maxsize=None)
def _grid(extra):
    """The 96 x 64 grid of unit squares, and with `extra` the same grid with one more square far away: (tiles, graph)."""
    w, h = 96, 64
    x, y = [c.reshape(-1) for c in np.meshgrid(np.arange(w), np.arange(h))]
    tiles = [hc.box(a, b, a + 1, b + 1) for a, b in zip(x, y)] + [hc.box(200, 0, 201, 1)] * extra
    assert len(tiles) == 6144 + extra
    return tiles, _made_up_graph(tiles)


@pytest.mark.parametrize("extra", [0, 1])
def test_graphs_either_side_of_the_lds_limit(extra):
    """The labels live in LDS for the walk on graphs of up to 6 144 tiles and in the slot's row beyond: the 96 x 64 grid of unit
    squares and the same grid with one more square far away.  By the reasoning of tests/test_hole_sweep_gpu.py: the left, right
    and lower neighbours of an interior cell enclose nothing, the upper one would close the ring around it (d holes +1: passed
    over), the cell itself fills the gap; in the next call the upper neighbour completes a solid plus."""
    w = 96
    tiles, od = _grid(extra)
    n = len(tiles)
    run = Harness(od, np.arange(n), np.zeros((2, 0)), 2)
    cell = 40 * w + 50
    order = np.array([cell - 1, cell + 1, cell - w, cell + w, cell])
    first = run.call([0], [1], [order], [np.ones(5)], [np.zeros(5)])
    assert first["err"][0] == 0
    assert first["trace"].tolist() == [[ACCEPTED, 0], [ACCEPTED, 0], [ACCEPTED, 0], [VETOED, 1], [ACCEPTED, 0]]
    assert first["stats"][0].tolist() == [5, 1, 0, 4, 0, 0, 0, 0]
    assert first["accepted"].tolist() == [cell - 1, cell + 1, cell - w, cell, -1] and (first["killed"] == -1).all()
    unl, alive, label, _ = run.state()
    chosen = [cell - w, cell - 1, cell, cell + 1]
    assert unl[0].all() and not alive[0].any() and (label[0] == -1).all()   # the parent
    assert np.flatnonzero(alive[1]).tolist() == chosen and np.flatnonzero(unl[1] == 0).tolist() == chosen
    assert (label[1][chosen] == cell - w).all() and (np.delete(label[1], chosen) == -1).all()
    second = run.call([1], [1], [[cell + w, cell]], [[1.0, 0.5]], [[0.75, 0.0]])
    assert second["err"][0] == 0 and second["trace"].tolist() == [[ACCEPTED, 0], [BREAK, 0]]
    assert second["stats"][0].tolist() == [2, 0, 1, 1, 0, 0, 0, 0]
    assert (run.state()[2][1][chosen + [cell + w]] == cell - w).all()


# ------------------------------------------------------------------------------------------------ one acceptance for both entries
def _collision_rows(n, col):
    col = np.asarray(col).reshape(2, -1).astype(np.int64)
    by_src = np.argsort(col[0], kind="stable")
    return np.searchsorted(col[0][by_src], np.arange(n + 1)), col[1][by_src]


def _walk_on_the_host(rings, col, order):
    """The walk both entries make from the empty selection when every node that is not vetoed is accepted and the first labelled
    node ends it, written out again with the loop-tracing oracle as the veto (as tests/hole_guard_restatement.py and
    tests/tree_search_restatement.py write theirs).  -> trace [len(order), 2], accepted, killed, acceptances that merged components."""
    starts, nbr = _collision_rows(len(rings), col)
    unlabelled = np.ones(len(rings), dtype=bool)
    trace, tiles, accepted, killed = np.zeros((len(order), 2), dtype=np.int32), [], [], []
    components = merges = 0
    for pos, node in enumerate(int(i) for i in order):
        if not unlabelled[node]:
            trace[pos] = BREAK, 0
            break
        now, holes = to.topology(tiles + [rings[node]])
        if holes > 0:
            trace[pos] = VETOED, holes
            continue
        trace[pos] = ACCEPTED, holes
        merges += now < components                                          # it joined two components or more
        components = now
        tiles.append(rings[node])
        unlabelled[node] = False
        accepted.append(node)
        for v in nbr[starts[node]:starts[node + 1]]:
            if unlabelled[v]:
                unlabelled[v] = False
                killed.append(int(v))
    return trace, accepted, killed, merges


def _both_entries_walk_alike(od, rings, col, order):
    """The hole entry with thr = 1, u = 0 and the tree entry with check_holes, p = 0, u = 1 on the same order from the empty
    state: the same lists, trace and state bytes -- after the host has said that the order meets a veto, a merge and a kill."""
    from tests.test_hole_sweep_gpu import Harness as HoleHarness
    n, v = len(rings), len(order)
    trace, accepted, killed, merges = _walk_on_the_host(rings, col, order)
    assert (trace[:, 0] == VETOED).any() and merges > 0 and killed and (trace[:, 0] == BREAK).any()
    hole, tree = HoleHarness(od, [(np.arange(n), col)]), Harness(od, np.arange(n), col, 1)
    a = hole.call([order], [np.ones(v)], [np.zeros(v)])
    b = tree.call([0], [0], [order], [np.zeros(v)], [np.ones(v)])
    assert a["err"][0] == 0 and b["err"][0] == 0
    assert (a["trace"] == b["trace"]).all() and (a["trace"] == trace).all()
    assert a["stats"][0][[0, 1, 3, 4]].tolist() == b["stats"][0][[0, 1, 3, 4]].tolist()     # (the draws differ: one per test, one at the break)
    assert a["accepted"][:v].tolist() == accepted + [-7] * (v - len(accepted)) and b["accepted"].tolist() == accepted + [-1] * (v - len(accepted))
    assert a["killed"][:n].tolist() == killed + [-7] * (n - len(killed)) and b["killed"].tolist() == killed + [-1] * (v - len(killed))
    assert tree.guards_intact
    assert all(x.tobytes() == y.tobytes() for x, y in zip(hole.state(), tree.state()))      # unlabelled, tile_alive, label, chi_cache
    return len(accepted), len(killed), int((trace[:, 0] == VETOED).sum()), merges


@pytest.mark.parametrize("seed", range(3))
def test_both_entries_run_the_same_acceptance_on_the_small_graph(small, seed):
    """A seeded permutation of the nodes, those that an earlier node of it labels moved behind the others: the walk goes on until
    most of the graph is labelled and then meets its break."""
    fx = small
    starts, nbr = _collision_rows(fx.n, fx.col)
    free, front, back = np.ones(fx.n, dtype=bool), [], []
    for node in np.random.default_rng(seed).permutation(fx.n):
        (front if free[node] else back).append(int(node))
        if free[node]:
            free[node] = False
            free[nbr[starts[node]:starts[node + 1]]] = False
    counts = _both_entries_walk_alike(fx.on_device, fx.rings, fx.col, np.array(front + back))
    print(f"\nboth entries, small graph seed {seed}: %d accepted, %d killed, %d vetoes, %d merges" % counts)


@pytest.mark.parametrize("extra", [0, 1])
def test_both_entries_run_the_same_acceptance_either_side_of_the_lds_limit(extra):
    """Labels in LDS and in place: the plus of test_graphs_either_side_of_the_lds_limit -- the lower neighbour joins the left and
    the right one, the upper one is vetoed -- with a far cell that the centre labels and the walk then meets."""
    w = 96
    tiles, od = _grid(extra)
    cell, far = 40 * w + 50, 10 * w + 7
    order = np.array([cell - 1, cell + 1, cell - w, cell + w, cell, 7, far, 9])
    counts = _both_entries_walk_alike(od, tiles, np.array([[cell, far], [far, cell]]), order)
    assert counts == (5, 1, 1, 1)


# ------------------------------------------------------------------------------------------------ small cases
SIX = [hc.box(2 * i, 0, 2 * i + 1, 1) for i in range(6)]                    # six squares apart: no veto
SIX_COL = np.array([[0, 0, 0, 0, 3, 4, 2, 5], [4, 2, 4, 5, 0, 0, 0, 0]])


def test_without_check_holes_and_without_geometry():
    run = Harness(_made_up_graph(SIX), np.arange(6), SIX_COL, 3, geometry=False)
    out = run.call([0, 0], [1, 2], [[1, 0, 3, 2, 4, 5], [3, 0, 1]], [[1.0, 1.0, 1.0, 0.5, 0.5, 0.5], [1.0] * 3], [[0.25, 0.75, 0, 0, 0, 0], [0.0] * 3],
                   check_holes=0)
    assert out["err"].tolist() == [0, 0]
    assert out["trace"][:6].tolist() == [[ACCEPTED, 0], [ACCEPTED, 0], [ACCEPTED, 0], [SKIPPED, 0], [BREAK, 0], [NOT_REACHED, 0]]
    assert out["stats"][0].tolist() == [5, 0, 2, 3, 3, 1, 0, 0] and out["stats"][1].tolist() == [3, 0, 1, 2, 1, 1, 0, 0]
    assert out["accepted"][:6].tolist() == [1, 0, 3, -1, -1, -1] and out["killed"][:6].tolist() == [4, 2, 5, -1, -1, -1]
    assert out["trace"][6:].tolist() == [[ACCEPTED, 0], [SKIPPED, 0], [ACCEPTED, 0]]
    assert run.state()[0].tolist() == [[1] * 6, [0] * 6, [0, 0, 1, 0, 1, 1]]
    # the same call with the geometry keeps the tile state as well
    full = Harness(_made_up_graph(SIX), np.arange(6), SIX_COL, 3)
    same = full.call([0, 0], [1, 2], [[1, 0, 3, 2, 4, 5], [3, 0, 1]], [[1.0, 1.0, 1.0, 0.5, 0.5, 0.5], [1.0] * 3], [[0.25, 0.75, 0, 0, 0, 0], [0.0] * 3],
                     check_holes=0)
    assert all(same[name].tobytes() == out[name].tobytes() for name in out)
    assert full.state()[1].tolist() == [[0] * 6, [1, 1, 0, 1, 0, 0], [0, 1, 0, 1, 0, 0]]
    assert full.state()[2][1].tolist() == [0, 1, -1, 3, -1, -1]


@pytest.mark.parametrize("u,code", [(0.25, SKIPPED), (0.75, BREAK), (0.5, BREAK)])
def test_a_first_position_that_is_already_labelled(u, code):
    """One draw, then passed over (u < p) or the end of the walk; 0.5 < 0.5 is false."""
    run = Harness(_made_up_graph(SIX), np.arange(6), SIX_COL, 2)
    first = run.call([0], [0], [[0, 4, 2, 5]], [[1.0, 0.0, 0.0, 0.0]], [[0.5] * 4])     # node 0 and its three neighbours; 0.5 < 0 ends it
    assert first["stats"][0].tolist() == [2, 0, 1, 1, 3, 0, 0, 0] and first["killed"].tolist() == [4, 2, 5, -1]
    out = run.call([0], [1], [[4, 1, 3, 2]], [[0.5, 1.0, 1.0, 1.5]], [[u, 0.9, 0.9, 0.9]])
    assert out["err"][0] == 0 and out["trace"][0].tolist() == [code, 0]
    if code == BREAK:
        assert out["stats"][0].tolist() == [1, 0, 1, 0, 0, 0, 0, 0] and (out["trace"][1:] == 0).all()
        assert run.state()[0][1].tolist() == run.state()[0][0].tolist() == [0, 1, 0, 1, 0, 0]
    else:                                                                   # (0.9 < 1.5: the quirk passes over node 2 as well)
        assert out["trace"][:, 0].tolist() == [SKIPPED, ACCEPTED, ACCEPTED, SKIPPED] and out["stats"][0].tolist() == [4, 0, 2, 2, 0, 2, 0, 0]
        assert out["accepted"].tolist() == [1, 3, -1, -1]


def test_error_bits_slot_node_tile_and_collision_entry():
    od = _made_up_graph(SIX)
    for parents, slots in (([2], [0]), ([0], [2]), ([-1], [0]), ([0], [-5])):
        run = Harness(od, np.arange(6), SIX_COL, 2)
        out = run.call(parents + [0], slots + [1], [[0, 1], [1]], [[1.0, 1.0], [1.0]], [[0.0, 0.0], [0.0]])
        assert out["err"].tolist() == [1, 0] and out["stats"][0].tolist() == [0] * 8         # per branch; nothing of a slot is touched
        assert out["stats"][1].tolist() == [1, 0, 0, 1, 0, 0, 0, 0]
        assert run.state()[0][0].all() and run.state()[0][1].tolist() == [1, 0, 1, 1, 1, 1]
    for wrong in (6, -1, 2 ** 31 - 1):
        out = Harness(od, np.arange(6), SIX_COL, 2).call([0], [1], [[1, wrong, 2]], [[1.0] * 3], [[0.0] * 3])
        assert out["err"][0] == 1 and out["trace"][:, 0].tolist() == [ACCEPTED, NOT_REACHED, NOT_REACHED]
    assert Harness(od, np.array([0, 1, 2, 3, 4, 99]), SIX_COL, 2).call([0], [1], [[5]], [[1.0]], [[0.0]])["err"][0] == 1
    run = Harness(od, np.arange(6), SIX_COL, 2)
    run.nbr_idx[1] = 77                                                     # the second entry of node 0's row
    assert run.call([0], [1], [[0, 1, 3, 2]], [[1.0] * 4], [[0.0] * 4])["err"][0] == 1
    run = Harness(od, np.arange(6), SIX_COL, 2)
    run.nbr_ptr[1] = 99                                                     # node 0's row ends outside the array
    out = run.call([0], [1], [[0]], [[1.0]], [[0.0]])
    assert out["err"][0] == 1 and run.state()[0][1].all()
    # a collision row that ends behind the array, and one that ends before it begins, on the 3 x 3 set: met BEFORE the acceptance
    # (csrc/hole_sweep_block.h: block_accept) -- the node stays unlabelled, its tile dead, and the lists end where they did
    nine = _made_up_graph(hc.sets()["3x3 full"])
    col = np.array([[2, 8, 8], [6, 0, 6]])                                  # node 2 labels 6; node 8, whose row is the last, 0 and 6
    for end in (3 + 1, 0):
        run = Harness(nine, np.arange(9), col, 2)
        assert run.nbr_ptr.tolist() == [0, 0, 0, 1, 1, 1, 1, 1, 1, 3]
        run.nbr_ptr[9] = end
        out = run.call([0], [1], [[2, 8, 1, 3]], [[1.0] * 4], [[0.0] * 4])
        assert out["err"][0] == 1 and run.guards_intact
        assert out["accepted"].tolist() == [2, -1, -1, -1] and out["killed"].tolist() == [6, -1, -1, -1]
        unl, alive, _, _ = run.state()
        assert unl[1].tolist() == [1, 1, 0, 1, 1, 1, 0, 1, 1] and alive[1].tolist() == [0, 0, 1, 0, 0, 0, 0, 0, 0]
    # a visiting list shorter than what an acceptance labels: reported, the lists are not overrun
    out = Harness(od, np.arange(6), SIX_COL, 2).call([0], [1], [[0, 1]], [[1.0] * 2], [[0.0] * 2])
    assert out["err"][0] == 1


# ------------------------------------------------------------------------------------------------ refusals
def test_abi_rejects_bad_arguments_and_empty_calls():
    from tilingnn_amd._lib import lib
    f64 = torch.zeros(64, dtype=torch.float64, device=DEV)
    i32 = torch.full((64,), -7, dtype=torch.int32, device=DEV)
    p = lambda t: t.data_ptr()

    def call(k=2, n_tiles=4, n_nodes=4, n_visit=4, n_slots=3, tol=1e-6, dx=1.0, dy=0.0, ws_bytes=256, ring=p(f64), state=p(i32), out=p(i32),
             check_holes=1, tiles=p(i32)):
        return lib.tgnn_tree_sweep_many(ring, ring and p(i32), n_tiles, ring and p(i32), ring and p(i32), tol, dx, dy, n_nodes, tiles, p(i32), p(i32),
                                        0, n_slots, state, state, state, state, k, p(i32), p(i32), p(i32), p(i32), p(f64), p(f64), n_visit,
                                        check_holes, out, out, out, out, out, p(i32), ws_bytes, None)

    assert call(ws_bytes=4) == -1 and b"tgnn_tree_sweep_many" in lib.tgnn_last_error()       # a workspace that is too small
    assert call(ring=None) == -1 and call(state=None) == -1 and call(out=None) == -1 and call(tiles=None) == -1
    assert call(tol=-1.0) == -1 and call(dx=0.5, dy=0.5) == -1 and call(dx=float("nan")) == -1
    assert call(k=-1) == -1 and call(n_tiles=-1) == -1 and call(n_nodes=-1) == -1 and call(n_visit=2 ** 31) == -1 and call(n_slots=0) == -1
    # nothing to walk: nothing is queued, whatever the pointers
    assert call(k=0, ring=None, ws_bytes=0) == 0 and call(n_visit=0, out=None) == 0 and call(n_nodes=0, state=None) == 0
    torch.cuda.synchronize()
    assert (i32 == -7).all().item()
    assert lib.tgnn_tree_sweep_workspace_bytes(2) == 8 and lib.tgnn_tree_sweep_workspace_bytes(0) == 0
