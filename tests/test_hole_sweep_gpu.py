"""The hole-free greedy sweep on the device, raw: tgnn_hole_sweep_many (csrc/hole_sweep.hip) through
`CompleteGraphOnDevice.hole_sweep_into`.  Every round of the recipe solve (tests/hole_guard_restatement.py: round_probs) on the
small graph and on ring 9 has its trace checked in both directions against ONE tgnn_union_hole_delta call over the prefix masks
(the selection before each visit); then the bytes (a second call, dirty workspaces, a layout alone against the same layout in a
batch, an inactive layout), graphs either side of the LDS limit reasoned on the cells, both error bits, and the refusals.  Every
comparison is exact integer equality.  The per-visit code itself runs on the host under sanitizers in
tests/test_hole_sweep_host.py."""
import gzip
import math
import os
import shutil

import numpy as np
import pytest
import torch

from tests import hole_delta_cases as hc
from tests import hole_guard_restatement as hg
from tests.golden_util import GOLDEN

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
NOT_REACHED, BREAK, VETOED, REJECTED, ACCEPTED = range(5)


def _made_up_graph(tiles, touch=None, theta=None):
    """A CompleteGraphOnDevice over hand-made tiles (no TileGraph behind it), as tests/test_union_hole_delta_gpu.py makes one."""
    from tilingnn_amd.tiling.region import contact_geometry, sweep_direction, union_geometry
    from tilingnn_amd.util.data_util import CompleteGraphOnDevice
    n = len(tiles)
    geo = union_geometry(tiles, np.zeros((2, 0), dtype=np.int64), n)
    touch = contact_geometry(geo[0], geo[1]) if touch is None else touch
    theta = sweep_direction(geo[0], geo[1]) if theta is None else theta
    od = CompleteGraphOnDevice.__new__(CompleteGraphOnDevice)
    od.device, od.n_tiles = torch.device(DEV), n
    up = lambda a: torch.from_numpy(a if a.size else np.zeros(1, dtype=a.dtype)).to(DEV)
    od._union = tuple(up(a) for a in geo)
    od._topology = tuple(up(a) for a in touch) + (math.cos(theta), math.sin(theta))
    return od


class Harness:
    """The state of K layouts and one call per round, straight from arrays.  layouts: (tile of every node, collision edges
    [2, E] in local node numbers) per layout.  Outputs are filled with -7 before every call: what is read must be written."""

    def __init__(self, od, layouts):
        self.od, self.k = od, len(layouts)
        sizes = [len(t) for t, _ in layouts]
        self.node_ptr_h = np.concatenate([[0], np.cumsum(sizes)]).astype(np.int64)
        self.n = n = int(self.node_ptr_h[-1])
        nbr_ptr, nbr = np.zeros(n + 1, dtype=np.int64), []
        for k, (_, col) in enumerate(layouts):
            col = np.asarray(col).reshape(2, -1)
            by_src = np.argsort(col[0], kind="stable")                      # (HostSweep.__init__)
            n0 = self.node_ptr_h[k]
            nbr_ptr[n0 + 1:n0 + sizes[k] + 1] = nbr_ptr[n0] + np.searchsorted(col[0][by_src], np.arange(1, sizes[k] + 1))
            nbr.append(col[1][by_src])
        nbr = np.concatenate(nbr) if nbr else np.zeros(0)
        self.n_nbr = int(nbr.shape[0])
        up = lambda a: torch.from_numpy(np.ascontiguousarray(a, dtype=np.int32)).to(DEV)
        self.node_ptr, self.tile_of_node = up(self.node_ptr_h), up(np.concatenate([t for t, _ in layouts]))
        self.nbr_ptr, self.nbr_idx = up(nbr_ptr), up(nbr if self.n_nbr else np.zeros(1))
        self.unlabelled = torch.ones(n, dtype=torch.int32, device=DEV)
        self.tile_alive = torch.zeros(self.k, od.n_tiles, dtype=torch.int32, device=DEV)
        self.label = torch.full((self.k, od.n_tiles), -1, dtype=torch.int32, device=DEV)
        self.chi_cache = torch.full((self.k, od.n_tiles), -2 ** 31, dtype=torch.int32, device=DEV)

    def state(self):
        return tuple(t.cpu().numpy().copy() for t in (self.unlabelled, self.tile_alive, self.label, self.chi_cache))

    def call(self, visits, thr, u, active=None, ws_fill=None):
        """visits / thr / u: per layout the visiting order (local nodes), thresholds and uniforms.  -> dict of numpy outputs."""
        from tilingnn_amd._lib import lib
        k, n = self.k, self.n
        visit_ptr = np.concatenate([[0], np.cumsum([len(v) for v in visits])]).astype(np.int32)
        v = int(visit_ptr[-1])
        cat = lambda parts, dt: torch.from_numpy(np.concatenate([np.asarray(p, dtype=dt) for p in parts] + [np.zeros(1, dtype=dt)])).to(DEV)
        active = np.ones(k, dtype=np.int32) if active is None else np.asarray(active, dtype=np.int32)
        i32 = lambda count: torch.full((max(count, 1),), -7, dtype=torch.int32, device=DEV)
        out = {"stats": i32(8 * k), "err": i32(k), "accepted": i32(v), "killed": i32(n), "trace": i32(2 * v)}
        ws = torch.zeros(int(lib.tgnn_hole_sweep_workspace_bytes(k)) // 4, dtype=torch.int32, device=DEV)
        if ws_fill is not None:
            ws.view(torch.uint8).fill_(ws_fill)
        self.od.hole_sweep_into(k, self.node_ptr, n, self.tile_of_node, self.nbr_ptr, self.nbr_idx, self.n_nbr, self.unlabelled,
                                self.tile_alive, self.label, self.chi_cache, torch.from_numpy(active).to(DEV), torch.from_numpy(visit_ptr).to(DEV),
                                cat(visits, np.int32), cat(thr, np.float64), cat(u, np.float64), v, out["stats"], out["accepted"],
                                out["killed"], out["trace"], out["err"], ws)
        torch.cuda.synchronize()
        res = {name: t.cpu().numpy() for name, t in out.items()}
        res["stats"], res["trace"], res["visit_ptr"] = res["stats"][:8 * k].reshape(k, 8), res["trace"][:2 * v].reshape(v, 2), visit_ptr
        return res


class Fixture:
    def __init__(self, graph):
        from tilingnn_amd.util.data_util import graph_on_device
        self.graph = graph
        self.n = len(graph.tiles)
        self.col = graph.arrays.colli_edges
        self.on_device = graph_on_device(graph, DEV)


@pytest.fixture(scope="module")
def ring9(tmp_path_factory):
    from tilingnn_amd.tiling.tile_graph import TileGraph
    path = str(tmp_path_factory.mktemp("labyrinth") / "complete_graph_ring9.pkl")
    with gzip.open(os.path.join(GOLDEN, "complete_graph_ring9.pkl.gz"), "rb") as src, open(path, "wb") as dst:
        shutil.copyfileobj(src, dst)
    g = TileGraph(2)
    g.load_graph_state(path, sidecar=False)
    return Fixture(g)


@pytest.fixture(scope="module")
def small():
    from tilingnn_amd.tiling.tile_graph import TileGraph
    g = TileGraph(2)
    g.load_graph_state(os.path.join(GOLDEN, "complete_graph_small.pkl"), sidecar=False)
    return Fixture(g)


# ------------------------------------------------------------------------------------------------ the trace against the map
def _check_rounds_against_the_map(records, hole_deltas, tile_of):
    """records: per round (trace [V, 2], visit_node [V], stats row, the layout's unlabelled nodes after the round).  The prefix
    masks -- the selection before each visit changes only at an acceptance -- go to the map in ONE call; then every position."""
    masks, chosen = [[]], []
    for trace, visit, _, _ in records:
        for (code, _), node in zip(trace, visit):
            if code == ACCEPTED:
                chosen.append(int(tile_of[node]))
                masks.append(list(chosen))
    rows = np.zeros((len(masks), hole_deltas.n_tiles), dtype=np.int32)
    for r, tiles in enumerate(masks):
        rows[r, tiles] = 1
    delta, state = hole_deltas(rows)
    at = visits = vetoes = 0
    for trace, visit, stats, left in records:
        reached = trace[:, 0] != NOT_REACHED
        assert reached[:int(reached.sum())].all()                           # a prefix of the order
        assert int(stats[0]) == int(reached.sum()) and int(stats[1]) == int((trace[:, 0] == VETOED).sum())
        assert int(stats[2]) == int(np.isin(trace[:, 0], (REJECTED, ACCEPTED)).sum())      # a draw per test, none per veto
        assert int(stats[3]) == int((trace[:, 0] == ACCEPTED).sum())
        assert (trace[~reached] == 0).all() and (trace[:, 0] == BREAK).sum() <= 1
        if (trace[:, 0] == BREAK).any():
            assert trace[int(reached.sum()) - 1, 0] == BREAK
        for (code, d), node in zip(trace, visit):
            if code in (NOT_REACHED, BREAK):
                continue
            t = int(tile_of[node])
            assert state[at, t] == 0, (at, t)                               # a candidate of that mask
            assert d == delta[at, t, 1], (at, t, d, delta[at, t].tolist())
            assert (code == VETOED) == (delta[at, t, 1] > 0)
            visits += 1
            vetoes += code == VETOED
            at += code == ACCEPTED
        verdict = bool((delta[at, tile_of[left], 1] > 0).all())             # (True for no node left)
        assert bool(stats[5]) == verdict
    assert at == len(masks) - 1
    return visits, vetoes


class _Map:
    def __init__(self, od):
        self.od, self.n_tiles = od, od.n_tiles

    def __call__(self, rows):
        delta, state = self.od.hole_deltas(torch.from_numpy(rows).to(DEV))
        return delta.cpu().numpy(), state.cpu().numpy()


def _recipe_solve(fx, seed):
    """The recipe solve of the whole graph as the layout, driven round by round through DeviceHoleSweep (one raw call a round);
    the rounds' records for `_check_rounds_against_the_map`."""
    from tilingnn_amd.util.algorithms import DeviceHoleSweep
    dsw = DeviceHoleSweep(fx.graph, [(fx.n, fx.col, np.arange(fx.n))], [np.random.RandomState(seed)], DEV)
    sw, records, rnd = dsw.sweeps[0], [], 0
    while sw.unlabelled.any():
        rnd += 1
        ids = sw.ids()
        dsw.round([hg.round_probs(seed, rnd, fx.n, ids)])
        v = int(dsw.visit_ptr[1])
        left = np.flatnonzero(dsw.unlabelled.cpu().numpy()[:fx.n])
        records.append((dsw.trace[:v].copy(), dsw.visit_node[:v].copy(), dsw._stats_h[:8].copy(), left))
    return dsw, records, rnd


@pytest.mark.parametrize("seed", range(8))
def test_small_graph_every_round_against_the_map(seed, small):
    dsw, records, rounds = _recipe_solve(small, seed)
    visits, vetoes = _check_rounds_against_the_map(records, _Map(small.on_device), np.arange(small.n))
    assert vetoes == dsw.vetoes[0] and dsw.launches[0] == dsw.calls == rounds
    print(f"\nhole sweep small seed {seed}: {rounds} rounds, {visits} visits, {vetoes} vetoes, {len(dsw.sweeps[0].order)} tiles")


def test_ring9_every_round_against_the_map(ring9):
    dsw, records, rounds = _recipe_solve(ring9, 0)
    visits, vetoes = _check_rounds_against_the_map(records, _Map(ring9.on_device), np.arange(ring9.n))
    print(f"\nhole sweep ring 9 seed 0: {rounds} rounds, {visits} visits, {vetoes} vetoes, {len(dsw.sweeps[0].order)} tiles")
    assert (rounds, vetoes, len(dsw.sweeps[0].order)) == (65, 3589, 326)    # what DESIGN section 39 quotes for the host guard


# ------------------------------------------------------------------------------------------------ bytes
def test_same_bytes_alone_in_a_batch_and_on_dirty_workspaces(ring9):
    """Nine copies of ring 9 with their own visiting orders, eight rounds: three batches (clean, 0x7F and 0xFF workspaces) and
    nine single-layout runs give the same output and state bytes every round; layout 4 sits out rounds 3 and 4 untouched."""
    fx, K = ring9, 9
    layout = (np.arange(fx.n), fx.col)
    batches = [Harness(fx.on_device, [layout] * K) for _ in range(3)]
    solos = [Harness(fx.on_device, [layout]) for _ in range(K)]
    rng = np.random.default_rng(5)
    vetoes = 0
    for rnd in range(8):
        unl = batches[0].unlabelled.cpu().numpy().reshape(K, fx.n)
        active = np.array([int(unl[k].any() and not (k == 4 and rnd in (3, 4))) for k in range(K)], dtype=np.int32)
        visits, thr, u = [], [], []
        for k in range(K):
            ids = np.flatnonzero(unl[k]) if active[k] else np.zeros(0, dtype=np.int64)
            p = rng.random(ids.size)
            order = np.argsort(-p)
            visits.append(ids[order]); thr.append(np.exp(p[order] - 1)); u.append(rng.random(ids.size))
        before = batches[0].state()
        outs = [b.call(visits, thr, u, active=active, ws_fill=fill) for b, fill in zip(batches, (None, 0x7F, 0xFF))]
        for other, b in zip(outs[1:], batches[1:]):
            assert all(other[name].tobytes() == outs[0][name].tobytes() for name in outs[0])
            assert all(x.tobytes() == y.tobytes() for x, y in zip(b.state(), batches[0].state()))
        after = batches[0].state()
        ptr = outs[0]["visit_ptr"]
        for k in range(K):
            rows = slice(k * fx.n, (k + 1) * fx.n)
            if not active[k]:                                               # nothing of it is written, output or state
                assert (outs[0]["stats"][k] == -7).all() and outs[0]["err"][k] == -7 and (outs[0]["killed"][rows] == -7).all()
                assert (after[0][rows] == before[0][rows]).all() and (after[1][k] == before[1][k]).all() and (after[2][k] == before[2][k]).all()
                assert (after[3][k] == before[3][k]).all()
                continue
            one = solos[k].call([visits[k]], [thr[k]], [u[k]])
            assert one["err"][0] == 0 and (one["stats"][0] == outs[0]["stats"][k]).all()
            v0, v1 = int(ptr[k]), int(ptr[k + 1])
            n_acc, n_killed = int(one["stats"][0][3]), int(one["stats"][0][4])
            assert (one["trace"] == outs[0]["trace"][v0:v1]).all()
            assert (one["accepted"][:n_acc] == outs[0]["accepted"][v0:v0 + n_acc]).all()
            assert (one["killed"][:n_killed] == outs[0]["killed"][rows][:n_killed]).all()
            s = solos[k].state()
            assert (s[0] == after[0][rows]).all() and (s[1][0] == after[1][k]).all() and (s[2][0] == after[2][k]).all()
            assert (s[3][0] == after[3][k]).all()                            # what the cache knows is part of the state
            vetoes += int(one["stats"][0][1])
    assert vetoes > 0 and not batches[0].unlabelled.cpu().numpy().reshape(K, fx.n)[4].all()


# ------------------------------------------------------------------------------------------------ either side of the LDS limit
@pytest.mark.parametrize("extra", [0, 1])
def test_graphs_either_side_of_the_lds_limit(extra):
    """The labels live in LDS for the walk on graphs of up to 6 144 tiles and in the caller's array beyond: the 96 x 64 grid of
    unit squares of tests/test_union_hole_delta_gpu.py and the same grid with one more square far away.  By reasoning on the
    cells: the left, right and lower neighbours of an interior cell enclose nothing (they meet in corners of the cell), the upper
    one would close the ring around it, d holes +1, a veto without a draw; the cell itself fills the gap, d holes 0; and in the
    next round the upper neighbour completes a solid plus, d holes 0."""
    w, h = 96, 64
    x, y = [c.reshape(-1) for c in np.meshgrid(np.arange(w), np.arange(h))]
    tiles = [hc.box(a, b, a + 1, b + 1) for a, b in zip(x, y)] + [hc.box(200, 0, 201, 1)] * extra
    n = len(tiles)
    od = _made_up_graph(tiles)
    cell = 40 * w + 50
    order = np.array([cell - 1, cell + 1, cell - w, cell + w, cell])
    run = Harness(od, [(np.arange(n), np.zeros((2, 0)))])
    # (had the veto consumed a draw, the cell would meet 0.875 and be rejected)
    first = run.call([order], [np.array([1.0, 1.0, 1.0, 1.0, 0.5])], [np.array([0.5, 0.25, 0.125, 0.0, 0.875])], ws_fill=0x55)
    assert first["err"][0] == 0
    assert first["trace"].tolist() == [[ACCEPTED, 0], [ACCEPTED, 0], [ACCEPTED, 0], [VETOED, 1], [ACCEPTED, 0]]
    assert first["stats"][0].tolist() == [5, 1, 4, 4, 0, 0, 0, 0]          # four draws for five visits; other cells are free
    assert first["accepted"][:4].tolist() == [cell - 1, cell + 1, cell - w, cell]
    unl, alive, label, _ = run.state()
    chosen = [cell - w, cell - 1, cell, cell + 1]
    assert np.flatnonzero(alive[0]).tolist() == chosen and np.flatnonzero(unl == 0).tolist() == chosen
    assert (label[0][chosen] == cell - w).all() and (np.delete(label[0], chosen) == -1).all()
    second = run.call([[cell + w]], [[1.0]], [[0.0]])
    assert second["err"][0] == 0 and second["trace"].tolist() == [[ACCEPTED, 0]] and second["stats"][0].tolist() == [1, 0, 1, 1, 0, 0, 0, 0]
    assert (run.state()[2][0][chosen + [cell + w]] == cell - w).all()
    # ... and the same trace-against-map check
    left = [np.flatnonzero(s) for s in (unl, run.state()[0])]
    records = [(first["trace"], order, first["stats"][0], left[0]), (second["trace"], np.array([cell + w]), second["stats"][0], left[1])]
    assert _check_rounds_against_the_map(records, _Map(od), np.arange(n)) == (6, 1)


def test_components_merge_to_the_lowest_tile():
    """Labels after acceptances that join components whose lowest tiles differ: a row of seven squares taken as 6, 0, 3 (three
    components), then 5 and 4 (6-5-4-3 merge to 3), then 1 and 2 (everything merges to 0)."""
    tiles = [hc.box(i, 0, i + 1, 1) for i in range(7)]
    run = Harness(_made_up_graph(tiles), [(np.arange(7), np.zeros((2, 0)))])
    order = [6, 0, 3, 5, 4, 1, 2]
    want = [[-1] * 6 + [6], [0] + [-1] * 5 + [6], [0, -1, -1, 3, -1, -1, 6], [0, -1, -1, 3, -1, 5, 5], [0, -1, -1, 3, 3, 3, 3],
            [0, 0, -1, 3, 3, 3, 3], [0] * 7]
    for node, labels in zip(order, want):
        out = run.call([[node]], [[1.0]], [[0.0]])
        assert out["err"][0] == 0 and out["trace"].tolist() == [[ACCEPTED, 0]]
        assert run.state()[2][0].tolist() == labels


def test_killed_nodes_in_row_order_and_the_break():
    """A layout's collision rows: an acceptance clears the node's unlabelled neighbours in row order, once each, and the walk
    ends at the first node it meets that is labelled."""
    tiles = [hc.box(2 * i, 0, 2 * i + 1, 1) for i in range(6)]              # six squares apart: no veto
    col = np.array([[0, 0, 0, 0, 3, 4, 2, 5], [4, 2, 4, 5, 0, 0, 0, 0]])
    run = Harness(_made_up_graph(tiles), [(np.arange(6), col)])
    out = run.call([[1, 0, 3, 2, 4]], [[0.5, 1.0, 1.0, 1.0, 1.0]], [[0.75, 0.0, 0.0, 0.0, 0.0]])
    assert out["err"][0] == 0
    assert out["trace"][:, 0].tolist() == [REJECTED, ACCEPTED, ACCEPTED, BREAK, NOT_REACHED]
    assert out["stats"][0].tolist() == [4, 0, 3, 2, 3, 0, 0, 0]
    assert out["accepted"][:2].tolist() == [0, 3] and out["killed"][:3].tolist() == [4, 2, 5]
    assert run.state()[0].tolist() == [0, 1, 0, 0, 0, 0]


# ------------------------------------------------------------------------------------------------ error bits
def _fan(count):
    """Thin triangles fanned around the origin, which is a vertex of every one (tests/test_union_hole_delta_gpu.py)."""
    return [np.array([[0, 0], [math.cos(t), math.sin(t)], [math.cos(t + 0.2), math.sin(t + 0.2)]]) for t in 0.3 + 0.36 * np.arange(count)]


def test_error_bits_index_and_wedge_overflow():
    from tilingnn_amd._lib import TgnnError
    from tilingnn_amd.tiling.region import contact_geometry, union_geometry
    from tilingnn_amd.util.algorithms import DeviceHoleSweep
    fan = _fan(17)
    od = _made_up_graph(fan, theta=0.1234)
    layout, sixteen = (np.arange(17), np.zeros((2, 0))), (np.arange(16), np.zeros((2, 0)))
    # with the visited tile counted, 16 tiles around one point fit the wedge list and 17 do not (a layout of the first sixteen:
    # the stop rule looks at no seventeenth either)
    run = Harness(od, [sixteen])
    out = run.call([np.arange(16)], [np.ones(16)], [np.zeros(16)])
    assert out["err"][0] == 0 and out["trace"].tolist() == [[ACCEPTED, 0]] * 16 and out["stats"][0].tolist() == [16, 0, 16, 16, 0, 1, 0, 0]
    run = Harness(od, [layout, sixteen])
    out = run.call([np.arange(17), np.arange(16)], [np.ones(17), np.ones(16)], [np.zeros(17), np.zeros(16)])
    assert out["err"].tolist() == [2, 0]                                    # per layout
    assert out["trace"][:17].tolist() == [[ACCEPTED, 0]] * 16 + [[NOT_REACHED, 0]] and out["trace"][17:].tolist() == [[ACCEPTED, 0]] * 16

    class Graph:                                                            # ... which the binding raises on
        pass

    graph = Graph()
    graph._on_device = {torch.device(DEV): od}
    dsw = DeviceHoleSweep(graph, [(17, np.zeros((2, 0)), np.arange(17))], [np.random.RandomState(0)], DEV)
    with pytest.raises(TgnnError, match="wedge"):
        dsw.round([np.ones(17)])
    # an out-of-range contact entry, node, tile and collision entry: the index bit, nothing read or written out of range
    tiles = hc.sets()["3x3 full"]
    geo = union_geometry(tiles, np.zeros((2, 0), dtype=np.int64), 9)
    touch_ptr, touch_idx = contact_geometry(geo[0], geo[1])
    for wrong in (9, -1, 2 ** 31 - 1):
        broken = touch_idx.copy()
        broken[touch_ptr[4]] = wrong                                        # in the centre's row
        run = Harness(_made_up_graph(tiles, touch=(touch_ptr, broken)), [(np.arange(9), np.zeros((2, 0)))])
        assert run.call([[0, 4]], [[1.0, 1.0]], [[0.0, 0.0]])["err"][0] == 1, wrong
    good = _made_up_graph(tiles)
    assert Harness(good, [(np.arange(9), np.zeros((2, 0)))]).call([[0, 9]], [[1.0, 1.0]], [[0.0, 0.0]])["err"][0] == 1
    assert Harness(good, [(np.array([0, 1, 2, 3, 4, 5, 6, 7, 99]), np.zeros((2, 0)))]).call([[8]], [[1.0]], [[0.0]])["err"][0] == 1
    run = Harness(good, [(np.arange(9), np.array([[0], [8]]))])
    run.nbr_idx[0] = 77
    assert run.call([[0]], [[1.0]], [[0.0]])["err"][0] == 1
    # a collision row that ends behind the array, and one that ends before it begins: met BEFORE the acceptance
    # (csrc/hole_sweep_block.h: block_accept) -- the node stays unlabelled, its tile dead, and the lists end where they did
    col = np.array([[2, 8, 8], [6, 0, 6]])                                  # node 2 labels 6; node 8, whose row is the last, 0 and 6
    for end in (3 + 1, 0):
        run = Harness(good, [(np.arange(9), col)])
        assert run.nbr_ptr.tolist() == [0, 0, 0, 1, 1, 1, 1, 1, 1, 3]
        run.nbr_ptr[9] = end
        out = run.call([[2, 8, 1, 3]], [[1.0] * 4], [[0.0] * 4])
        assert out["err"][0] == 1
        assert out["accepted"].tolist() == [2, -7, -7, -7] and out["killed"].tolist() == [6] + [-7] * 8
        unl, alive, _, _ = run.state()
        assert unl.tolist() == [1, 1, 0, 1, 1, 1, 0, 1, 1] and alive[0].tolist() == [0, 0, 1, 0, 0, 0, 0, 0, 0]


# ------------------------------------------------------------------------------------------------ refusals
def test_abi_rejects_bad_arguments_and_empty_calls():
    from tilingnn_amd._lib import lib
    f64 = torch.zeros(64, dtype=torch.float64, device=DEV)
    i32 = torch.full((64,), -7, dtype=torch.int32, device=DEV)
    p = lambda t: t.data_ptr()

    def call(k=2, n_tiles=4, n_nodes=4, n_visit=4, tol=1e-6, dx=1.0, dy=0.0, ws_bytes=256, ring=p(f64), state=p(i32), out=p(i32)):
        return lib.tgnn_hole_sweep_many(ring, p(i32), n_tiles, p(i32), p(i32), tol, dx, dy, k, p(i32), n_nodes, p(i32), p(i32), p(i32), 0,
                                        state, state, state, state, p(i32), p(i32), p(i32), p(f64), p(f64), n_visit, out, out, out, out, out,
                                        p(i32), ws_bytes, None)

    assert call(ws_bytes=4) == -1 and b"tgnn_hole_sweep_many" in lib.tgnn_last_error()       # a workspace that is too small
    assert call(ring=None) == -1 and call(state=None) == -1 and call(out=None) == -1
    assert call(tol=-1.0) == -1 and call(dx=0.5, dy=0.5) == -1 and call(dx=float("nan")) == -1
    assert call(k=-1) == -1 and call(n_tiles=-1) == -1 and call(n_nodes=-1) == -1 and call(n_visit=2 ** 31) == -1
    # nothing to walk: nothing is queued, whatever the pointers
    assert call(k=0, ring=None, ws_bytes=0) == 0 and call(n_visit=0, out=None) == 0 and call(n_nodes=0, state=None) == 0
    torch.cuda.synchronize()
    assert (i32 == -7).all().item()
    assert lib.tgnn_hole_sweep_workspace_bytes(2) == 8 and lib.tgnn_hole_sweep_workspace_bytes(0) == 0


def test_an_empty_visiting_list_writes_nothing(small):
    run = Harness(small.on_device, [(np.arange(small.n), small.col)] * 2)
    before = run.state()
    out = run.call([[], [3]], [[], [1.0]], [[], [0.0]])
    assert (out["stats"][0] == -7).all() and out["err"][0] == -7 and out["stats"][1].tolist()[:5] == [1, 0, 1, 1, int(out["stats"][1][4])]
    after = run.state()
    assert (after[1][0] == before[1][0]).all() and (after[2][0] == before[2][0]).all() and after[0][:small.n].all()
    assert after[1][1].sum() == 1 and after[1][1][3] == 1
