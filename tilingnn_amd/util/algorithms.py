"""`solve_by_probablistic_greedy` -- the greedy assembly loop around `ML_Solver.predict`
(/root/reference/util/algorithms.py:18-62), with the layout resident on the GPU.

Per round the reference rebuilds the sub-layout of the still unlabelled nodes with four Python comprehensions and
dict look-ups over ALL edges (`BrickLayout.compute_sub_layout`, tiling/brick_layout.py:248-286) and ships it to the
device again.  Here the five arrays of the original layout are uploaded once; a round is
    alive mask -> `tgnn_sublayout_compact` (flags, scans, scatters: csrc/graph_prep.hip) -> `ml_solver.predict` on the
    device-resident sub-layout -> probabilities to the host -> the acceptance sweep.
The sweep itself stays on the host ON PURPOSE: it is sequential by definition (descending probability, stop at the
first node a previous acceptance has killed), touches a handful of nodes per round, and consumes numpy's global RNG
stream one `np.random.uniform()` per visited node (algorithms.py:51) -- the stream the reference consumes, so that a
seeded run selects the same tiles.

Same return values as the reference: (selection_predict, score, predict_order).  The score is
`Losses.solution_score` (losses.py:120-148 -> tilingnn_amd/solver/ml_solver/losses.py, sums on the GPU) whenever the
layout carries what it needs -- its complete graph (tile rings, max_area, max_align_length) and the area of its super
contour (`layout.super_contour_area`, or the reference class's `get_super_contour_poly()`); a bare `DeviceLayout` has
neither and scores `None` unless `score_fn(selection, origin_layout)` is given.

`check_holes=True` adds the reference's hole veto (algorithms.py:150-152) to that sweep: `HoleGuard` keeps, per node, what adding
its tile would do to the holes of the selection (csrc/union_hole_delta.hip) and the sweep passes over the tiles that would
enclose a gap, before the draw.  `device_sweep=True` runs that guarded sweep on the device instead (`DeviceHoleSweep`,
csrc/hole_sweep.hip): one launch and one read-back per ROUND, the same decisions and the same RNG stream; and
`solve_many_hole_free` runs it for K layouts of one complete graph in one loop, one block per layout.

`solve_many_by_device_greedy` runs K such device-greedy solves (the crops of one silhouette, Tiling-Shape.py:60-64) in one loop
over `PackedLayouts`: one compaction, one read-back and one acceptance call per round for all of them (csrc/greedy_many.hip).

`solve_by_treesearch` is the reference's tree search (algorithms.py:66-181), the consumer the hole veto was written for: a queue
of partial selections, one branch per top probability map of a popped state, every distinct finished tiling returned; the
branches of a step are swept side by side on the device (`DeviceTreeSweep`, csrc/tree_sweep.hip: a block per branch).
"""
import ctypes as C

import numpy as np
import torch

from .. import _lib, ops
from .._lib import check, lib, ptr


class DeviceLayout:
    """The data side of a BrickLayout (brick_layout.py:242-246) living on the GPU: what `ML_Solver.predict` reads."""

    def __init__(self, node_feature, align_edge_index, align_edge_features, collide_edge_index, inverse_index=None):
        self.node_feature = node_feature
        self.align_edge_index = align_edge_index
        self.align_edge_features = align_edge_features
        self.collide_edge_index = collide_edge_index
        self.collide_edge_features = None                     # never read by the network (TilinGNN.py:51)
        self.inverse_index = inverse_index                    # sub-layout node -> original node
        self.super_contour_area = None                        # set by CompleteGraphOnDevice.layouts_in_regions(with_area=True)

    def get_data_as_torch_tensor(self, device):
        return (self.node_feature, self.align_edge_index, self.align_edge_features, self.collide_edge_index,
                self.collide_edge_features)

    @staticmethod
    def upload(layout, device) -> "DeviceLayout":
        """From the numpy arrays of a BrickLayout / LayoutArrays, with the conversion of util/data_util.py:110-117."""
        t = lambda a, dt: torch.from_numpy(np.ascontiguousarray(a)).to(dt).to(device)
        adj = np.asarray(layout.align_edge_index).reshape(2, -1)
        col = np.asarray(layout.collide_edge_index).reshape(2, -1)
        fe = np.asarray(layout.align_edge_features).shape[-1] if np.asarray(layout.align_edge_features).size else 1
        return DeviceLayout(t(layout.node_feature, torch.float32), t(adj, torch.int64),
                            t(np.asarray(layout.align_edge_features).reshape(-1, fe), torch.float32), t(col, torch.int64))


class SubLayoutBuilder:
    """compute_sub_layout on the device: buffers sized once for the original layout, reused every round."""

    def __init__(self, origin: DeviceLayout):
        self.o = origin
        x, adj, attr, col = origin.node_feature, origin.align_edge_index, origin.align_edge_features, origin.collide_edge_index
        dev = x.device
        self.n, self.fx = int(x.shape[0]), int(x.shape[1])
        self.ea, self.ec, self.fe = int(adj.shape[1]), int(col.shape[1]), int(attr.shape[1]) if attr.numel() else 1
        self.x_out = torch.empty(self.n, self.fx, dtype=torch.float32, device=dev)
        self.inverse = torch.empty(self.n, dtype=torch.int64, device=dev)
        self.adj_out = torch.empty(2 * max(self.ea, 1), dtype=torch.int64, device=dev)
        self.attr_out = torch.empty(max(self.ea, 1) * self.fe, dtype=torch.float32, device=dev)
        self.col_out = torch.empty(2 * max(self.ec, 1), dtype=torch.int64, device=dev)
        self._tail = torch.zeros(4, dtype=torch.int64, device=dev)       # counts [3] | error flag: ONE read-back per round
        self.counts = self._tail[:3]
        self.err = self._tail[3:].view(torch.int32)[:1]
        self.ws_bytes = lib.tgnn_sublayout_workspace_bytes(self.n, self.ea, self.ec)
        self.ws = torch.empty(self.ws_bytes, dtype=torch.uint8, device=dev)
        self._host = torch.empty(4, dtype=torch.int64, pin_memory=True)    # (`.cpu()` stages through a pageable tensor: ~10 us more per round)

    def build(self, alive: torch.Tensor) -> DeviceLayout:
        """alive: int32 [N] on the device (!= 0 = unlabelled).  One host sync (the three counts)."""
        o = self.o
        check(lib.tgnn_sublayout_compact(ptr(alive), self.n, ptr(o.node_feature), self.fx,
                                         ptr(o.align_edge_index) if self.ea else None, self.ea,
                                         ptr(o.align_edge_features) if self.ea else None, self.fe,
                                         ptr(o.collide_edge_index) if self.ec else None, self.ec,
                                         ptr(self.x_out), ptr(self.inverse), ptr(self.adj_out), ptr(self.attr_out),
                                         ptr(self.col_out), ptr(self.counts), ptr(self.err), ptr(self.ws), self.ws_bytes,
                                         _lib.current_stream(alive.device)))
        self._host.copy_(self._tail, non_blocking=True)
        torch.cuda.current_stream(alive.device).synchronize()
        n2, ea2, ec2, err = self._host.tolist()
        if err:
            raise IndexError("edge index out of range in the layout")
        return DeviceLayout(self.x_out[:n2], self.adj_out[:2 * ea2].view(2, ea2), self.attr_out[:ea2 * self.fe].view(ea2, self.fe),
                            self.col_out[:2 * ec2].view(2, ec2), self.inverse[:n2])


class HostSweep:
    """The state and the acceptance sweep of the reference's loop (algorithms.py:23-54), over the ORIGINAL node numbering: the
    running geometric mean of the probabilities (:33-34), the descending walk that stops at the first node labelled in this
    round (:41-48), the test against numpy's global RNG stream (:51), label_collision_neighbor (:196-207).  Shared by the
    single-GPU loop below and by tilingnn_amd.dist.solve_sharded (every rank runs the same sweep on the gathered probabilities
    with the same seed, so every rank takes the same decisions)."""

    def __init__(self, n: int, collide_edge_index: np.ndarray, uniform=None):
        # uniform: the draw of :51; default numpy's GLOBAL stream, as the reference (np.random.RandomState(seed).uniform gives the
        # stream np.random.seed(seed) would: what thread-simulated ranks, which share one interpreter, use instead)
        self.uniform = uniform if uniform is not None else np.random.uniform
        col = np.asarray(collide_edge_index).reshape(2, -1)
        self.n, self.has_col = n, bool(col.size)
        if self.has_col:                                        # collision neighbours in edge order (algorithms.py:199)
            by_src = np.argsort(col[0], kind="stable")
            self.starts = np.searchsorted(col[0][by_src], np.arange(n + 1))
            self.nbr = col[1][by_src]
        self.prob_saved = np.ones(n)                            # SelectionSolution.unlabelled_nodes (:285)
        self.unlabelled = np.ones(n, dtype=bool)
        self.selection = np.zeros(n)
        self.order = []
        self.round_cnt = 1

    def ids(self) -> np.ndarray:
        return np.flatnonzero(self.unlabelled)

    def round(self, ids: np.ndarray, prob, guard=None) -> list:
        """One round: `prob` = the network's probabilities of the nodes `ids` (ascending original numbers).  Returns the original
        numbers of the nodes labelled in this round (selected ones and their collision neighbours).  guard: a `HoleGuard`; a
        node it vetoes is passed over BEFORE the draw (the reference's order, algorithms.py:150-152), so it consumes no random
        number and stays unlabelled; without one the path and the RNG stream are the ones they always were."""
        prob = np.asarray(prob, dtype=np.float64).reshape(-1)
        prob_per_node = np.power(np.power(self.prob_saved[ids], self.round_cnt - 1) * prob, 1 / self.round_cnt)     # (:33-34)
        self.prob_saved[ids] = prob_per_node
        unlabelled, killed = self.unlabelled, []
        for idx in np.argsort(-prob_per_node):                  # (:41)
            origin_idx = ids[idx]
            if not unlabelled[origin_idx]:                      # (:47-48)
                break
            if guard and guard.vetoed(origin_idx):              # (:150-152)
                continue
            if np.exp((prob_per_node[idx] - 1) * 1.0) > self.uniform():     # (:51)
                unlabelled[origin_idx] = False
                self.selection[origin_idx] = 1
                self.order.append(int(origin_idx))
                killed.append(origin_idx)
                if guard:
                    guard.accept(origin_idx)
                if self.has_col:                                # label_collision_neighbor (:196-207)
                    for v in self.nbr[self.starts[origin_idx]:self.starts[origin_idx + 1]]:
                        if unlabelled[v]:
                            unlabelled[v] = False
                            killed.append(v)
        self.round_cnt += 1
        return killed


def _tiles_of_nodes(inverse_index, n, n_tiles, who=""):
    """inverse_index (node -> tile) of the n nodes of a layout as int64 tiles, every one inside the graph."""
    tiles = np.fromiter((inverse_index[i] for i in range(n)), dtype=np.int64, count=n)
    if n and (tiles.min() < 0 or tiles.max() >= n_tiles):
        raise ValueError(f"{who}inverse_index names a tile outside [0, {n_tiles})")
    return tiles


class _AheadDraws:
    """The RNG hand-over of a device walk: keeps the generator's state and draws n uniforms in one call (`u`); `settle(consumed)`,
    once the walk has said how many it consumed, rewinds the generator and draws exactly those.  numpy's `uniform(size=n)` is n
    scalar draws bit for bit, so the decisions AND the generator's state afterwards are those of scalar draws
    (tests/test_hole_sweep_host.py and tests/test_tree_search_host.py pin both)."""

    def __init__(self, rng, n):
        self.rng, self.state = rng, rng.get_state()
        self.u = rng.uniform(size=n)

    def settle(self, consumed):
        self.rng.set_state(self.state)                          # the stream moves by what the walk consumed, no more
        self.rng.uniform(size=int(consumed))


class _Staging:
    """A device buffer and a pinned host buffer of int32 words per direction, cut into the same named fields.  fields_in,
    fields_out: (name, int32 words, dtype) in buffer order -- f64 fields first, so that they stay 8-byte aligned.  `dev[name]`:
    the device views; `host[name]`: numpy views of the pinned buffers; `send()` queues the ONE host-to-device copy, `fetch()` the
    ONE device-to-host copy and waits for the stream."""

    def __init__(self, device, fields_in, fields_out):
        self.device, self.dev, self.host = device, {}, {}
        self._in, self._out = self._cut(fields_in), self._cut(fields_out)

    def _cut(self, fields):
        words = sum(w for _, w, _ in fields) + 1
        dev = torch.zeros(words, dtype=torch.int32, device=self.device)
        host = torch.zeros(words, dtype=torch.int32, pin_memory=True)
        at = 0
        for name, w, dtype in fields:
            self.dev[name], self.host[name] = dev[at:at + w].view(dtype), host[at:at + w].view(dtype).numpy()
            at += w
        return dev, host

    def send(self):
        self._in[0].copy_(self._in[1], non_blocking=True)

    def fetch(self):
        self._out[1].copy_(self._out[0], non_blocking=True)
        torch.cuda.current_stream(self.device).synchronize()


class _SweepStaging(_Staging):
    """What a call of a device walk over K visiting lists of V positions in all sends -- rate [V] f64 (thr or prob_m by position)
    | u [V] f64 | visit_node [V] | visit_ptr [K + 1] | one [K] table per name of `tables` -- and brings back -- stats [K][8] |
    err [K] | accepted [V] | killed [V] | trace [V][2].  `v`: the positions listed so far."""

    def __init__(self, device, K, V, tables):
        f64, i32 = torch.float64, torch.int32
        super().__init__(device, [("rate", 2 * V, f64), ("u", 2 * V, f64), ("visit_node", V, i32), ("visit_ptr", K + 1, i32)]
                         + [(name, K, i32) for name in tables],
                         [("stats", 8 * K, i32), ("err", K, i32), ("accepted", V, i32), ("killed", V, i32), ("trace", 2 * V, i32)])

    def begin(self):
        self.v, self.ahead = 0, {}
        self.host["visit_ptr"][0] = 0

    def add(self, k, nodes, rate, rng):
        """List k of the call (in order of k): `nodes` in visiting order, `rate` by position, a uniform per position from rng."""
        h, v, n = self.host, self.v, len(nodes)
        self.ahead[k] = _AheadDraws(rng, n)
        h["visit_node"][v:v + n], h["rate"][v:v + n], h["u"][v:v + n] = nodes, rate, self.ahead[k].u
        self.v = v + n

    def result(self, k, entry, killed_at=None):
        """Of list k, after fetch(): its error bits raised as `entry`'s, else its generator settled and (stats row [8], accepted
        nodes, killed nodes) as numpy copies.  killed_at: where its killed list starts (default: where its visiting list does)."""
        h = self.host
        if h["err"][k]:
            from .data_util import _TOPOLOGY_ERROR_BITS, _raise_device_error
            _raise_device_error(entry, int(h["err"][k]), _TOPOLOGY_ERROR_BITS)
        row = h["stats"][8 * k:8 * k + 8].copy()
        self.ahead[k].settle(row[2])
        v0 = int(h["visit_ptr"][k])
        k0 = v0 if killed_at is None else killed_at
        return row, h["accepted"][v0:v0 + int(row[3])].astype(np.int64), h["killed"][k0:k0 + int(row[4])].astype(np.int64)


class HoleGuard:
    """The hole veto of the reference's assembly (algorithms.py:150-152, check_holes -> exist_hole: refuse a tile whose union
    with the selection has an interior ring) for the sweep of `HostSweep`: holds, per node of the layout, what adding its tile
    would do to the holes of the current selection (`CompleteGraphOnDevice.hole_deltas`, csrc/union_hole_delta.hip) and vetoes
    the nodes with d holes > 0.  The selection starts empty with 0 holes and only tiles with d holes <= 0 are accepted, so every
    prefix of the order has 0 holes -- and with 0 holes "the union has an interior ring" IS d holes > 0.  Built from the layout's
    `complete_graph` and `inverse_index` (node -> tile).  `accept(node)` queues ONE kernel call and reads its map back once (the
    map and the error word in one copy); `launches` and `vetoes` count both."""

    def __init__(self, complete_graph, inverse_index, n: int, device=None):
        from .data_util import graph_on_device
        self.on_device = graph_on_device(complete_graph, device)
        dev, n_tiles = self.on_device.device, self.on_device.n_tiles
        self.tiles = _tiles_of_nodes(inverse_index, n, n_tiles)
        self._alive = torch.zeros(n_tiles, dtype=torch.int32, device=dev)
        self._out = torch.zeros(3 * n_tiles + 1, dtype=torch.int32, device=dev)          # delta [n_tiles][2] | state [n_tiles] | error word
        self._host = torch.empty(3 * n_tiles + 1, dtype=torch.int32, pin_memory=True)
        self.dholes = np.zeros(n, dtype=np.int32)               # the empty selection: every tile adds {+1, 0}
        self.state = np.zeros(n, dtype=np.int32)
        self.launches = self.vetoes = 0

    def vetoed(self, node) -> bool:
        if self.dholes[node] > 0:
            self.vetoes += 1
            return True
        return False

    def all_vetoed(self, nodes) -> bool:
        """Whether every one of `nodes` is vetoed under the current selection (the stop rule; counts nothing)."""
        return bool((self.dholes[nodes] > 0).all())

    def accept(self, node):
        od, n_tiles = self.on_device, self.on_device.n_tiles
        self._alive[int(self.tiles[node])] = 1
        self._out[-1:].zero_()
        od.hole_deltas_into(self._alive[None, :], self._out[:2 * n_tiles], self._out[2 * n_tiles:3 * n_tiles], self._out[-1:])
        self._host.copy_(self._out, non_blocking=True)
        torch.cuda.current_stream(od.device).synchronize()
        self.launches += 1
        words = self._host.numpy()
        if words[-1]:
            from .data_util import _TOPOLOGY_ERROR_BITS, _raise_device_error
            _raise_device_error("tgnn_union_hole_delta", int(words[-1]), _TOPOLOGY_ERROR_BITS)
        self.state = words[2 * n_tiles:3 * n_tiles][self.tiles]
        if (self.state == 3).any():
            raise ValueError("HoleGuard: two accepted tiles collide")
        self.dholes = words[:2 * n_tiles].reshape(n_tiles, 2)[self.tiles, 1]


class DeviceHoleSweep:
    """`HostSweep.round(ids, prob, guard)` with a `HoleGuard`, for K layouts cut from ONE complete graph, ON THE DEVICE
    (csrc/hole_sweep.hip: tgnn_hole_sweep_many): per round ONE host-to-device copy (who is active, the visiting orders, the
    thresholds, the uniforms), one call -- a block per layout walks its order and computes a node's d holes when it gets there --
    and ONE device-to-host copy (counters, accepted and killed nodes, the trace).  The decisions are the host sweep's, one for one.
    layouts: (n nodes, collide_edge_index as numpy, inverse_index) per layout; rngs: per layout what draws its uniforms,
    `np.random` itself or a `RandomState`, handed over per round by `_AheadDraws`: the selection AND the generator's state
    afterwards are the host sweep's.
    State per layout as `HostSweep` keeps it (`sweeps[k]`: prob_saved, unlabelled, selection, order, round_cnt) and on the device
    `unlabelled` [N] int32 (the alive mask the sub-layout compaction reads), `tile_alive`, `label`, `chi_cache` [K, n_tiles].
    `vetoes`, `launches` [K]: per layout the vetoes counted and the rounds it was active in; `calls`: sweep calls queued;
    `trace`: the last round's [V, 2] {code, d holes} with `visit_ptr`, `visit_node` beside it (numpy views of the staging
    buffers, valid until the next round)."""

    def __init__(self, complete_graph, layouts, rngs, device=None):
        from .data_util import graph_on_device
        self.on_device = od = graph_on_device(complete_graph, device)
        dev, n_tiles = od.device, od.n_tiles
        layouts = list(layouts)
        self.k = K = len(layouts)
        self.rngs = list(rngs)
        if len(self.rngs) != K:
            raise ValueError(f"rngs: one per layout ({K}), got {len(self.rngs)}")
        self.sweeps = [HostSweep(int(n), col) for n, col, _ in layouts]
        sizes = [sw.n for sw in self.sweeps]
        self.node_ptr_h = np.concatenate([[0], np.cumsum(sizes, dtype=np.int64)])
        self.n = N = int(self.node_ptr_h[-1])
        tiles = np.zeros(max(N, 1), dtype=np.int32)
        nbr_ptr, nbr_idx = np.zeros(N + 1, dtype=np.int64), []
        for k, ((n, _, inverse), sw) in enumerate(zip(layouts, self.sweeps)):
            n0 = int(self.node_ptr_h[k])
            tiles[n0:n0 + n] = _tiles_of_nodes(inverse, n, n_tiles, f"layout {k}: ")
            if sw.has_col:                                      # the rows HostSweep walks (edge order), local numbers
                nbr_ptr[n0 + 1:n0 + n + 1] = nbr_ptr[n0] + sw.starts[1:]
                nbr_idx.append(sw.nbr)
            else:
                nbr_ptr[n0 + 1:n0 + n + 1] = nbr_ptr[n0]
        nbr_idx = np.concatenate(nbr_idx) if nbr_idx else np.zeros(0, dtype=np.int64)
        self.n_nbr = int(nbr_idx.shape[0])
        if max(N, self.n_nbr, n_tiles) >= 2 ** 31 - 1:
            raise ValueError("DeviceHoleSweep: more than 2^31 nodes or collision entries")
        up = lambda a: torch.from_numpy(np.ascontiguousarray(a, dtype=np.int32)).to(dev)
        self.node_ptr, self.tile_of_node = up(self.node_ptr_h), up(tiles)
        self.nbr_ptr, self.nbr_idx = up(nbr_ptr), up(nbr_idx if self.n_nbr else np.zeros(1))
        i32 = torch.int32
        self.unlabelled = torch.ones(max(N, 1), dtype=i32, device=dev)
        self.tile_alive = torch.zeros(max(K, 1), n_tiles, dtype=i32, device=dev)
        self.label = torch.full((max(K, 1), n_tiles), -1, dtype=i32, device=dev)
        self.chi_cache = torch.full((max(K, 1), n_tiles), -2 ** 31, dtype=i32, device=dev)     # TGNN_SWEEP_CHI_UNKNOWN
        self._staging = _SweepStaging(dev, K, N, ("active",))
        self._stats_h = self._staging.host["stats"]             # (the last round's stats rows; tests read them)
        self._ws = torch.empty(max(K, 1), dtype=i32, device=dev)
        self.vetoes, self.launches = np.zeros(K, dtype=np.int64), np.zeros(K, dtype=np.int64)
        self.calls = 0
        self.trace = self.visit_ptr = self.visit_node = None

    def active(self):
        return [bool(sw.unlabelled.any()) for sw in self.sweeps]

    def round(self, probs) -> list:
        """One round of every layout with probs[k] not None: probs[k] = the network's probabilities of the nodes
        `sweeps[k].ids()`.  Returns per layout the original numbers of the nodes labelled in this round (None where it did not
        run).  A layout all of whose remaining nodes are vetoed afterwards is finished: its `unlabelled` is cleared on the host."""
        K, N, od = self.k, self.n, self.on_device
        st = self._staging
        h, d = st.host, st.dev
        ran = []
        st.begin()
        for k, (sw, prob) in enumerate(zip(self.sweeps, probs)):
            ids = sw.ids() if prob is not None else ()
            h["active"][k] = int(len(ids) > 0)
            if len(ids):
                prob = np.asarray(prob, dtype=np.float64).reshape(-1)
                per_node = np.power(np.power(sw.prob_saved[ids], sw.round_cnt - 1) * prob, 1 / sw.round_cnt)     # (HostSweep.round)
                sw.prob_saved[ids] = per_node
                order = np.argsort(-per_node)
                st.add(k, ids[order], np.exp((per_node[order] - 1) * 1.0), self.rngs[k])
                ran.append(k)
            elif prob is not None:
                sw.round_cnt += 1                               # (a round over no node: HostSweep.round counts it)
            h["visit_ptr"][k + 1] = st.v
        out = [None if p is None else [] for p in probs]
        if not ran:
            return out
        st.send()
        od.hole_sweep_into(K, self.node_ptr, N, self.tile_of_node, self.nbr_ptr, self.nbr_idx, self.n_nbr, self.unlabelled,
                           self.tile_alive, self.label, self.chi_cache, d["active"], d["visit_ptr"], d["visit_node"], d["rate"], d["u"],
                           st.v, d["stats"], d["accepted"], d["killed"], d["trace"], d["err"], self._ws)
        st.fetch()
        self.calls += 1
        self.trace, self.visit_ptr, self.visit_node = h["trace"].reshape(-1, 2), h["visit_ptr"], h["visit_node"]
        for k in ran:
            sw = self.sweeps[k]
            row, acc, gone = st.result(k, f"tgnn_hole_sweep_many (layout {k})", int(self.node_ptr_h[k]))
            sw.unlabelled[acc] = False
            sw.unlabelled[gone] = False
            sw.selection[acc] = 1
            sw.order.extend(int(i) for i in acc)
            sw.round_cnt += 1
            self.vetoes[k] += row[1]
            self.launches[k] += 1
            out[k] = [int(i) for i in acc] + [int(i) for i in gone]
            if row[5]:                                          # all vetoed: nothing can change any more (solve_by_probablistic_greedy)
                sw.unlabelled[:] = False
        return out


def solve_by_probablistic_greedy(ml_solver, origin_layout, score_fn=None, on_round=None, check_holes=False, device_sweep=False):
    """algorithms.py:18-62.  `origin_layout`: BrickLayout-like numpy arrays (uploaded once) or a DeviceLayout.
    check_holes: the reference's hole veto (:150-152) in this sweep, through a `HoleGuard` (kept as
    `solve_by_probablistic_greedy.last_guard`): a tile that would enclose a gap is passed over, so the selection never has a
    hole; the layout must carry its `complete_graph` and `inverse_index`.  A round after which every unlabelled node is vetoed
    ends the loop with those nodes unselected: nothing can change any more.  Like the reference's, the veto cannot close a
    tiling around a hole the target region itself has.
    device_sweep (with check_holes): the same loop with the guarded sweep on the device -- `DeviceHoleSweep` with K = 1 and
    numpy's GLOBAL stream in place of `HostSweep` + `HoleGuard`: one launch and one read-back per round instead of one per
    accepted tile; the same selection, order, round count, vetoes and generator state afterwards.  `.last_guard` is then the
    `DeviceHoleSweep` (`vetoes[0]`, `launches[0]`)."""
    if device_sweep and not check_holes:
        raise ValueError("device_sweep runs the guarded sweep of check_holes=True on the device; without check_holes there is "
                         "nothing for it to run")
    if check_holes and getattr(origin_layout, "complete_graph", None) is None:
        raise ValueError("check_holes needs the layout's complete graph (tile rings) and inverse_index: a BrickLayout, not a "
                         "bare DeviceLayout")
    device = ml_solver.device
    origin = origin_layout if isinstance(origin_layout, DeviceLayout) else DeviceLayout.upload(origin_layout, device)
    n = int(origin.node_feature.shape[0])
    col_host = origin.collide_edge_index.cpu().numpy()
    sweep = HostSweep(n, col_host)
    builder = SubLayoutBuilder(origin)
    alive_dev = torch.ones(n, dtype=torch.int32, device=origin.node_feature.device)
    guard = None
    if device_sweep:
        dsw = DeviceHoleSweep(origin_layout.complete_graph, [(n, col_host, origin_layout.inverse_index)], [np.random],
                              origin.node_feature.device)
        solve_by_probablistic_greedy.last_guard = dsw
        sweep = dsw.sweeps[0]
        while sweep.unlabelled.any():
            temp_layout = builder.build(dsw.unlabelled)         # (the sweep's own mask on the device: nothing to upload)
            if on_round is not None:
                on_round(temp_layout)
            dsw.round([ml_solver.predict(temp_layout)])
        score = create_score(sweep.selection, origin_layout, score_fn, device)
        return sweep.selection, score, sweep.order
    if check_holes:
        guard = HoleGuard(origin_layout.complete_graph, origin_layout.inverse_index, n, origin.node_feature.device)
        solve_by_probablistic_greedy.last_guard = guard
    while sweep.unlabelled.any():
        temp_layout = builder.build(alive_dev)
        ids = sweep.ids()                                       # == temp_layout.inverse_index (kept on the device)
        if on_round is not None:
            on_round(temp_layout)
        killed = sweep.round(ids, ml_solver.predict(temp_layout), guard)
        if killed:
            alive_dev[torch.from_numpy(np.asarray(killed, dtype=np.int64)).to(alive_dev.device)] = 0
        if guard and guard.all_vetoed(sweep.ids()):             # (the map is at hand: no launch)
            sweep.unlabelled[:] = False
    score = create_score(sweep.selection, origin_layout, score_fn, device)
    return sweep.selection, score, sweep.order


def solve_by_device_greedy(ml_solver, origin_layout, seed=0, score_fn=None, on_round=None, max_rounds=100000, finish=True):
    """The assembly loop with the acceptance BATCHED on the device (csrc/greedy.hip: tgnn_greedy_round) -- the documented
    substitute of the reference's sequential sweep (algorithms.py:41-54) for large layouts (BASELINE config 5: "batched greedy
    selection"): per round every node that precedes all its unlabelled collision neighbours in the reference's visiting order
    and passes the reference's test exp(p - 1) > u is accepted at once, u from a counter-based generator keyed by (seed, round,
    node).  NOT the reference's RNG stream -- `solve_by_probablistic_greedy` stays the default where seeded parity matters --
    but the same invariants: a collision-free selection, maximal when the loop ends, the same running geometric mean of the
    probabilities (:33-34).  O(log N) rounds of {compaction, forward, four small launches}; nothing but one count per round
    travels to the host.  Same return values: (selection, score, predict_order); the order = by round, then by node number.
    finish (no `on_round` given): once a sub-layout has no adjacency edge or no collision edge left -- from there on ML_Solver.predict
    answers 1 for every node without the network (ml_solver.py:31-32) -- the remaining rounds run as ONE launch on that sub-layout
    (tgnn_greedy_finish: the same means, order, draws and round numbers, hence the same selection and round count)."""
    device = ml_solver.device
    origin = origin_layout if isinstance(origin_layout, DeviceLayout) else DeviceLayout.upload(origin_layout, device)
    dev = origin.node_feature.device
    n = int(origin.node_feature.shape[0])
    builder = SubLayoutBuilder(origin)
    alive = torch.ones(n, dtype=torch.int32, device=dev)
    selected = torch.zeros(n, dtype=torch.int32, device=dev)
    saved = torch.ones(n, dtype=torch.float64, device=dev)
    tail = torch.zeros(2, dtype=torch.int64, device=dev)        # accepted so far | error flag
    ws_bytes = int(lib.tgnn_greedy_round_workspace_bytes(n))
    ws = torch.empty(ws_bytes, dtype=torch.uint8, device=dev)
    rounds = 0
    while True:
        sub = builder.build(alive)                              # (one sync: the sub-layout's sizes)
        n2 = int(sub.node_feature.shape[0])
        if n2 == 0:
            break
        rounds += 1
        if rounds > max_rounds:
            raise RuntimeError(f"solve_by_device_greedy: {n2} nodes still unlabelled after {max_rounds} rounds")
        if on_round is not None:
            on_round(sub)
        ea2, ec2 = int(sub.align_edge_index.shape[1]), int(sub.collide_edge_index.shape[1])
        if finish and on_round is None and (ea2 == 0 or ec2 == 0) and n2 <= int(lib.tgnn_greedy_finish_max_nodes()):
            out = torch.zeros(2, dtype=torch.int32, device=dev)
            check(lib.tgnn_greedy_finish(ptr(sub.inverse_index), n2, ptr(sub.collide_edge_index) if ec2 else None, ec2, rounds,
                                         max_rounds - rounds + 1, int(seed) & (2 ** 64 - 1), ptr(saved), ptr(alive), ptr(selected),
                                         ptr(tail[:1]), ptr(tail[1:].view(torch.int32)[:1]), ptr(out), _lib.current_stream(dev)))
            ran, left = out.cpu().tolist()
            rounds += ran - 1
            if left:
                raise RuntimeError(f"solve_by_device_greedy: {left} nodes still unlabelled after {max_rounds} rounds")
            break
        probs = ml_solver.predict_on_device(sub)                # [n2] float32 on the device
        ec2 = int(sub.collide_edge_index.shape[1])
        check(lib.tgnn_greedy_round(ptr(probs), 1, ptr(sub.inverse_index), n2, ptr(sub.collide_edge_index) if ec2 else None, ec2,
                                    rounds, int(seed) & (2 ** 64 - 1), ptr(saved), ptr(alive), ptr(selected), ptr(tail[:1]),
                                    ptr(tail[1:].view(torch.int32)[:1]), ptr(ws), ws_bytes, _lib.current_stream(dev)))
    sel_round = selected.cpu().numpy()
    if int(tail[1].item()):
        raise IndexError("collision edge index out of range in a sub-layout")
    selection = (sel_round > 0).astype(np.float64)
    picked = np.flatnonzero(sel_round > 0)
    order = [int(v) for v in picked[np.lexsort((picked, sel_round[picked]))]]
    score = create_score(selection, origin_layout, score_fn, device)
    solve_by_device_greedy.last_rounds = rounds
    return selection, score, order


class PackedLayouts:
    """K layouts packed ONCE for `solve_many_by_device_greedy` (csrc/greedy_many.hip): their arrays concatenated on the device,
    offset tables node_ptr / adj_ptr / col_ptr [K + 1] (int64, host lists `*_h` and device tensors), edge ends in each layout's
    LOCAL numbering, layout k's edge index its own [2][E_k] block at element 2 * ptr[k] of the flat index buffer.
    `layouts`: DeviceLayouts or BrickLayout-like numpy layouts (converted as DeviceLayout.upload does; all-numpy input is
    concatenated on the host and uploaded in four copies instead of 4 K)."""

    def __init__(self, layouts, device):
        layouts = list(layouts)
        self.k = len(layouts)
        device = torch.device(device)
        on_dev = [l for l in layouts if isinstance(l, DeviceLayout)]
        if on_dev:
            device = on_dev[0].node_feature.device
            layouts = [l if isinstance(l, DeviceLayout) else DeviceLayout.upload(l, device) for l in layouts]
        self.device = device
        xs, adjs, attrs, cols = [], [], [], []
        for l in layouts:
            if on_dev:
                x, adj, attr, col = l.node_feature, l.align_edge_index.reshape(2, -1), l.align_edge_features, l.collide_edge_index.reshape(2, -1)
            else:
                x = np.ascontiguousarray(l.node_feature, dtype=np.float32)
                adj = np.asarray(l.align_edge_index).reshape(2, -1).astype(np.int64, copy=False)
                col = np.asarray(l.collide_edge_index).reshape(2, -1).astype(np.int64, copy=False)
                attr = np.asarray(l.align_edge_features)
                attr = attr.reshape(-1, attr.shape[-1] if attr.size else 1).astype(np.float32, copy=False)
            xs.append(x); adjs.append(adj); attrs.append(attr); cols.append(col)
        self.fx = max([int(x.shape[1]) for x in xs if x.ndim == 2] or [1])
        self.fe = max([int(a.shape[1]) for a, e in zip(attrs, adjs) if e.shape[1]] or [1])
        for k, (x, adj, attr) in enumerate(zip(xs, adjs, attrs)):
            if x.shape[0] and (x.ndim != 2 or x.shape[1] != self.fx):
                raise ValueError(f"layout {k}: node_feature must be [N, {self.fx}], got {tuple(x.shape)}")
            if adj.shape[1] and (attr.shape[0] != adj.shape[1] or attr.shape[1] != self.fe):
                raise ValueError(f"layout {k}: align_edge_features must be [{adj.shape[1]}, {self.fe}], got {tuple(attr.shape)}")
        ptr_of = lambda sizes: [0] + [int(v) for v in np.cumsum(sizes, dtype=np.int64)]
        self.node_ptr_h = ptr_of([x.shape[0] for x in xs])
        self.adj_ptr_h = ptr_of([a.shape[1] for a in adjs])
        self.col_ptr_h = ptr_of([c.shape[1] for c in cols])
        self.n, self.ea, self.ec = self.node_ptr_h[-1], self.adj_ptr_h[-1], self.col_ptr_h[-1]
        none = lambda shape: tuple(0 if v == -1 else v for v in shape)
        if on_dev:
            cat = lambda ts, shape, dt: (torch.cat([t.reshape(shape).to(dt) for t in ts]) if ts else torch.empty(none(shape), dtype=dt, device=device)).contiguous()
            self.x = cat([x for x in xs if x.shape[0]], (-1, self.fx), torch.float32)
            self.adj = cat([a for a in adjs if a.shape[1]], (-1,), torch.int64)
            self.attr = cat([a for a, e in zip(attrs, adjs) if e.shape[1]], (-1, self.fe), torch.float32)
            self.col = cat([c for c in cols if c.shape[1]], (-1,), torch.int64)
        else:
            cat = lambda arrs, shape, dt: torch.from_numpy(np.ascontiguousarray(
                np.concatenate([np.asarray(a, dtype=dt).reshape(shape) for a in arrs]) if arrs else np.zeros(none(shape), dtype=dt))).to(device)
            self.x = cat([x for x in xs if x.shape[0]], (-1, self.fx), np.float32)
            self.adj = cat([a for a in adjs if a.shape[1]], (-1,), np.int64)
            self.attr = cat([a for a, e in zip(attrs, adjs) if e.shape[1]], (-1, self.fe), np.float32)
            self.col = cat([c for c in cols if c.shape[1]], (-1,), np.int64)
        ptrs = torch.tensor([self.node_ptr_h, self.adj_ptr_h, self.col_ptr_h], dtype=torch.int64).to(device)
        self.node_ptr, self.adj_ptr, self.col_ptr = ptrs[0], ptrs[1], ptrs[2]

    def nodes(self, k: int) -> int:
        return self.node_ptr_h[k + 1] - self.node_ptr_h[k]

    def ptr_tables_c(self):
        """(node_ptr, adj_ptr, col_ptr) [K + 1] as C int64 arrays on the host, built once: what `tgnn_batch_union` checks its
        arguments against (ops.batch_union)."""
        tables = getattr(self, "_ptr_tables_c", None)
        if tables is None:
            tables = self._ptr_tables_c = tuple((C.c_int64 * (self.k + 1))(*p) for p in
                                                (self.node_ptr_h, self.adj_ptr_h, self.col_ptr_h))
        return tables

    def layout(self, k: int) -> DeviceLayout:
        """Layout k as a view of the packed arrays."""
        return self.view(k, self.x, self.adj, self.attr, self.col, *(p[k + 1] - p[k] for p in (self.node_ptr_h, self.adj_ptr_h, self.col_ptr_h)))

    def view(self, k, x, adj, attr, col, n, ea, ec, inverse=None) -> DeviceLayout:
        """The first n nodes / ea / ec edges of layout k's part of buffers laid out like the packed arrays (a sub-layout)."""
        n0, a0, c0 = self.node_ptr_h[k], self.adj_ptr_h[k], self.col_ptr_h[k]
        return DeviceLayout(x[n0:n0 + n], adj[2 * a0:2 * (a0 + ea)].view(2, ea), attr[a0:a0 + ea], col[2 * c0:2 * (c0 + ec)].view(2, ec),
                            None if inverse is None else inverse[n0:n0 + n])


def _forward_many_checked(network, subs, streams, union=False, union_prep=False):
    """`forward_many` + what `forward_checked` adds to a forward, ONCE for all layouts: a stale-result status of an earlier
    unchecked forward is answered by queueing the forwards again; the health word of the persistent kernels is polled (this
    synchronises the current stream) and, if set, the forwards are repeated on the general launch schedule."""
    args = [(s.node_feature, s.align_edge_index, s.align_edge_features, s.collide_edge_index) for s in subs]
    kw = {"union": True} if union else {}                       # (union: after a starved kernel the fall-back window keeps every layout out of it)
    if union and union_prep:
        kw["union_prep"] = True                                 # (the sub-layouts' graphs from one library call: forward_many)
    try:
        outs = network.forward_many(args, streams=streams, **kw)
    except _lib.TgnnError as exc:
        if exc.code != _lib.ERR_STALE_RESULT:
            raise
        outs = network.forward_many(args, streams=streams, **kw)
    dev = subs[0].node_feature.device
    code = C.c_uint32(0)
    check(lib.tgnn_spin_error_poll(_lib.current_stream(dev), C.byref(code)))
    if code.value:
        import warnings
        warnings.warn("tilingnn_amd: a persistent forward kernel gave up waiting for its blocks (another process holds compute "
                      f"units; reason bits {code.value}); the forwards are repeated on the general launch schedule, which the "
                      "next forwards of this process take as well", RuntimeWarning)
        outs = network.forward_many(args, streams=streams, **kw)
    return outs


def solve_many_by_device_greedy(ml_solver, layouts, seed=0, seeds=None, score_fn=None, max_rounds=100000, streams=3):
    """K independent `solve_by_device_greedy` runs in ONE loop (csrc/greedy_many.hip): per round one compaction call for all
    layouts (`tgnn_sublayout_compact_many`), ONE copy of the K x 3 counts and the K error words to the host, the sub-layouts that
    still need the network scored side by side (`network.forward_many`), the health poll of `forward_checked` once, one
    acceptance call (`tgnn_greedy_round_many`); layouts that reach the state from which ML_Solver.predict answers 1 without the
    network finish in one launch (`tgnn_greedy_finish_many`) and leave; the loop ends when no layout is active.
    THE SAME COMPUTATION as K single solves: result k equals `solve_by_device_greedy(ml_solver, layouts[k], seed=s_k)` -- selection,
    predict_order, round count and score (`forward_many` gives the solo forward's bits, the draws are keyed by (seed, round,
    local node), the sums run over fixed trees).  One difference that does not reach any output: in train mode `forward_many`
    leaves the BatchNorm running statistics untouched where K `forward` calls update them; train-mode outputs do not read them.
    `layouts`: a list of DeviceLayouts / BrickLayout-like numpy layouts, or a PackedLayouts; seeds: one per layout (default:
    `seed` for all).  Returns a list of K (selection, score, predict_order); `.last_rounds` = the K round counts,
    `.last_first_probs` = the first round's probabilities per layout ([n_k] float32 on the device: what predict_on_device
    gives for the whole layout).  `ml_solver.union_forward = True` (an attribute like `device_greedy_seed`, default False): every
    round's small sub-layouts are scored inside one persistent kernel launch (`forward_many(union=True)`) -- the same bits, fewer
    launches.  `ml_solver.union_prep = True` beside it: their graphs are prepared by one library call and one read-back per round
    (`forward_many(union=True, union_prep=True)`) -- the same graphs.  A network with several probability maps: the best map of
    every sub-layout of a round comes from ONE loss call and one read-back (`Losses.unsupervised_losses_many` over the round's
    compacted buffers) -- the single-layout losses' bits, hence the same picks."""
    device = ml_solver.device
    originals = None if isinstance(layouts, PackedLayouts) else list(layouts)
    solve_many_by_device_greedy.last_rounds = []
    solve_many_by_device_greedy.last_first_probs = []
    if originals is not None and not originals:
        return []
    pk = layouts if isinstance(layouts, PackedLayouts) else PackedLayouts(originals, device)
    K = pk.k
    if K == 0:
        return []
    seeds_h = [int(seed)] * K if seeds is None else [int(s) for s in seeds]
    if len(seeds_h) != K:
        raise ValueError(f"seeds: one per layout ({K}), got {len(seeds_h)}")
    # a layout without nodes: whatever the single-layout loop makes of it (it never enters a round here)
    empty = {k: solve_by_device_greedy(ml_solver, originals[k] if originals is not None else pk.layout(k), seed=seeds_h[k],
                                       score_fn=score_fn, max_rounds=max_rounds) for k in range(K) if pk.nodes(k) == 0}
    dev = pk.device
    stream = lambda: _lib.current_stream(dev)
    n_tot, ea_tot, ec_tot = pk.n, pk.ea, pk.ec
    i64, i32 = torch.int64, torch.int32
    x_out = torch.empty(max(n_tot, 1), pk.fx, dtype=torch.float32, device=dev)
    inverse = torch.empty(max(n_tot, 1), dtype=i64, device=dev)
    adj_out = torch.empty(2 * max(ea_tot, 1), dtype=i64, device=dev)
    attr_out = torch.empty(max(ea_tot, 1), pk.fe, dtype=torch.float32, device=dev)
    col_out = torch.empty(2 * max(ec_tot, 1), dtype=i64, device=dev)
    alive = torch.ones(max(n_tot, 1), dtype=i32, device=dev)
    selected = torch.zeros(max(n_tot, 1), dtype=i32, device=dev)
    saved = torch.ones(max(n_tot, 1), dtype=torch.float64, device=dev)
    # what the host reads: counts [K][3] | error words [K] int32 | finish results [K][2] int32 | accepted so far [K]
    tail = torch.zeros(6 * K, dtype=i64, device=dev)
    counts, err = tail[:3 * K], tail[3 * K:4 * K].view(i32)[:K]
    fin_out, n_selected = tail[4 * K:5 * K].view(i32), tail[5 * K:]
    tail_h = torch.empty(6 * K, dtype=i64, pin_memory=True)
    # what the host sends per round: probability pointers [K] | finish words [K] int32 | acceptance words [K] int32
    meta = torch.zeros(2 * K, dtype=i64, device=dev)
    meta_h = torch.zeros(2 * K, dtype=i64, pin_memory=True)
    prob_tab, fin_words, act_words = meta[:K], meta[K:].view(i32)[:K], meta[K:].view(i32)[K:]
    words_h = meta_h[K:].view(i32)
    seeds_dev = torch.from_numpy(np.array([s & (2 ** 64 - 1) for s in seeds_h], dtype=np.uint64).view(np.int64)).to(dev)
    cws_bytes = int(lib.tgnn_sublayout_compact_many_workspace_bytes(K, n_tot, ea_tot, ec_tot))
    rws_bytes = int(lib.tgnn_greedy_round_many_workspace_bytes(K, n_tot))
    cws = torch.empty(cws_bytes, dtype=torch.uint8, device=dev)
    rws = torch.empty(rws_bytes, dtype=torch.uint8, device=dev)
    fin_max = int(lib.tgnn_greedy_finish_max_nodes())
    active = [pk.nodes(k) > 0 for k in range(K)]
    rounds = [0] * K
    finished_in = {}                                            # layout -> the round its finishing launch started in
    first_probs = [None] * K
    words_h[K:] = torch.tensor([int(a) for a in active], dtype=i32)
    words_h[:K] = 0
    meta.copy_(meta_h, non_blocking=True)
    network = ml_solver.network
    union_forward = bool(getattr(ml_solver, "union_forward", False))
    union_prep = bool(getattr(ml_solver, "union_prep", False))
    rnd = 0

    def raise_errors(words):
        bad = [k for k in range(K) if words[k]]
        if bad:
            raise IndexError(f"edge index out of range in layout {bad[0]} of {K}" + (f" (and in layouts {bad[1:]})" if bad[1:] else ""))

    while any(active):
        check(lib.tgnn_sublayout_compact_many(K, ptr(act_words), ptr(pk.node_ptr), ptr(pk.adj_ptr), ptr(pk.col_ptr), n_tot, ea_tot, ec_tot,
                                              ptr(alive), ptr(pk.x), pk.fx, ptr(pk.adj), ptr(pk.attr), pk.fe, ptr(pk.col), ptr(x_out),
                                              ptr(inverse), ptr(adj_out), ptr(attr_out), ptr(col_out), ptr(counts), ptr(err), ptr(cws),
                                              cws_bytes, stream()))
        tail_h.copy_(tail, non_blocking=True)                   # the round's ONE read-back
        torch.cuda.current_stream(dev).synchronize()
        host = tail_h.numpy()
        raise_errors(host[3 * K:4 * K].view(np.int32)[:K])
        cnt = host[:3 * K].reshape(K, 3)
        rnd += 1
        fin, need_net, subs = [], [], {}
        for k in range(K):
            if not active[k]:
                continue
            n2, ea2, ec2 = (int(v) for v in cnt[k])
            if n2 == 0:
                active[k] = False
                rounds[k] = rnd - 1
                continue
            if rnd > max_rounds:
                raise RuntimeError(f"solve_many_by_device_greedy: layout {k}: {n2} nodes still unlabelled after {max_rounds} rounds")
            if (ea2 == 0 or ec2 == 0) and n2 <= fin_max:
                fin.append(k)
                active[k] = False
                finished_in[k] = rnd
                if rnd == 1:
                    first_probs[k] = torch.ones(n2, dtype=torch.float32, device=dev)
                continue
            rounds[k] = rnd
            if ea2 == 0 or ec2 == 0:                            # probability 1 without the network (ml_solver.py:31-32), too large to finish in one block
                if rnd == 1:
                    first_probs[k] = torch.ones(n2, dtype=torch.float32, device=dev)
                continue
            subs[k] = pk.view(k, x_out, adj_out, attr_out, col_out, n2, ea2, ec2, inverse)
            need_net.append(k)
        meta_h[:K] = 0
        keep = []
        if need_net:
            views = [subs[k] for k in need_net]
            if hasattr(network, "forward_many"):
                outs = _forward_many_checked(network, views, streams, union_forward, union_prep)
            else:
                outs = [ml_solver.predict_on_device(v).reshape(-1, 1) for v in views]
            best_of = _best_prob_maps_many(pk, need_net, outs, (x_out, adj_out, attr_out, col_out), counts) if outs[0].shape[1] > 1 else None
            for k, sub, out in zip(need_net, views, outs):
                best = best_of[k] if best_of is not None else 0
                meta_h[k] = out.data_ptr() + 4 * best
                if rnd == 1:
                    first_probs[k] = out[:, best].detach().contiguous()
            keep = outs
            ld_prob = int(outs[0].shape[1])
        else:
            ld_prob = 1
        words_h[:K] = torch.tensor([int(k in finished_in and finished_in[k] == rnd) for k in range(K)], dtype=i32)
        words_h[K:] = torch.tensor([int(a) for a in active], dtype=i32)
        meta.copy_(meta_h, non_blocking=True)                   # the round's ONE upload (the pinned buffer is rewritten only after the next round's synchronisation)
        if fin:
            check(lib.tgnn_greedy_finish_many(K, ptr(fin_words), ptr(pk.node_ptr), ptr(pk.col_ptr), n_tot, ec_tot, ptr(counts), ptr(inverse),
                                              ptr(col_out), rnd, max_rounds - rnd + 1, ptr(seeds_dev), ptr(saved), ptr(alive), ptr(selected),
                                              ptr(n_selected), ptr(err), ptr(fin_out), stream()))
        if any(active):
            check(lib.tgnn_greedy_round_many(K, ptr(act_words), ptr(prob_tab), ld_prob, ptr(pk.node_ptr), ptr(pk.col_ptr), n_tot, ec_tot,
                                             ptr(counts), ptr(inverse), ptr(col_out), rnd, ptr(seeds_dev), ptr(saved), ptr(alive),
                                             ptr(selected), ptr(n_selected), ptr(err), ptr(rws), rws_bytes, stream()))
        del keep
    tail_h.copy_(tail, non_blocking=True)
    sel_h = selected.cpu().numpy()                              # (synchronises: the copy above has landed too)
    host = tail_h.numpy()
    raise_errors(host[3 * K:4 * K].view(np.int32)[:K])
    fin_h = host[4 * K:5 * K].view(np.int32).reshape(K, 2)
    selections, orders = [], []
    for k in range(K):
        if k in finished_in:
            ran, left = int(fin_h[k, 0]), int(fin_h[k, 1])
            rounds[k] = finished_in[k] + ran - 1
            if left:
                raise RuntimeError(f"solve_many_by_device_greedy: layout {k}: {left} nodes still unlabelled after {max_rounds} rounds")
        sel_round = sel_h[pk.node_ptr_h[k]:pk.node_ptr_h[k + 1]]
        selections.append((sel_round > 0).astype(np.float64))
        picked = np.flatnonzero(sel_round > 0)
        orders.append([int(v) for v in picked[np.lexsort((picked, sel_round[picked]))]])
    scores = _scores_many(pk, selections, originals, score_fn, device)
    solve_many_by_device_greedy.last_rounds = rounds
    solve_many_by_device_greedy.last_first_probs = first_probs
    return [empty[k] if k in empty else (selections[k], scores[k], orders[k]) for k in range(K)]


def _best_prob_maps_many(pk, members, outs, buffers, counts):
    """`ML_Solver._best_prob_map` (get_best_prob_map, ml_solver.py:133-136) for the sub-layouts `members` of a round at once: ONE
    `Losses.unsupervised_losses_many` call over the round's compacted buffers, one read-back, then the reference's pick on the
    float32 losses -- per layout the losses, the checks and the pick of the single-layout call.  -> {layout: map}."""
    from ..solver.ml_solver.losses import Losses
    probs, live = [None] * pk.k, [False] * pk.k
    for k, out in zip(members, outs):
        probs[k], live[k] = out, True
    m = int(outs[0].shape[1])
    buf, losses, terms, err = Losses.many_outputs(pk.k, m, pk.device)
    Losses.unsupervised_losses_many(probs, pk, buffers=buffers, counts=counts, active=live, out=(losses, terms, err))
    results = Losses.results_many(*Losses.read_back_many(buf, pk.k, m), present=live)
    return {k: int(np.argsort(results[k][2])[0]) for k in members}


def _prob_map_ranks_many(pk, members, outs):
    """The whole ranking `_best_prob_maps_many` takes the head of: per layout `np.argsort` of its per-map unsupervised losses
    (float32, as `ML_Solver.get_unsupervised_losses_from_layout` gives them), from ONE `tgnn_unsupervised_loss_many` call and one
    read-back.  -> {layout: map indices, best first}.  What `ML_Solver.predict_top_maps` hands the tree search."""
    from ..solver.ml_solver.losses import Losses
    probs, live = [None] * pk.k, [False] * pk.k
    for k, out in zip(members, outs):
        probs[k], live[k] = out, True
    m = int(outs[0].shape[1])
    buf, losses, terms, err = Losses.many_outputs(pk.k, m, pk.device)
    Losses.unsupervised_losses_many(probs, pk, buffers=None, counts=None, active=live, out=(losses, terms, err))
    results = Losses.results_many(*Losses.read_back_many(buf, pk.k, m), present=live)
    return {k: np.argsort(results[k][2]) for k in members}


def _scores_many(pk, selections, originals, score_fn, device):
    """`create_score` for K selections: `score_fn` when given; `Losses.solution_score` -- its three sums for all layouts in one
    `tgnn_solution_score_sums_many` call, over the single-layout call's summation tree -- for the layouts that carry their
    complete graph and super-contour area; None for the others."""
    K = pk.k
    if originals is None:
        originals = [None] * K
    if score_fn is not None:
        return [score_fn(selections[k], originals[k]) for k in range(K)]
    import math
    from ..solver.ml_solver.losses import loss_weights
    areas = [None] * K
    for k, lay in enumerate(originals):
        if lay is None or getattr(lay, "complete_graph", None) is None or not pk.nodes(k):
            continue
        area = getattr(lay, "super_contour_area", None)
        if area is None and hasattr(lay, "get_super_contour_poly"):
            area = lay.get_super_contour_poly().area
        areas[k] = area
    scored = [k for k in range(K) if areas[k] is not None]
    if not scored:
        return [None] * K
    dev = pk.device
    perims = np.zeros(max(pk.n, 1), dtype=np.float32)
    for k in scored:
        lay, n = originals[k], pk.nodes(k)
        per = getattr(lay, "_tile_perimeters", None)
        if per is None or per.shape[0] != n:
            inv, cg = lay.inverse_index, lay.complete_graph
            per = np.array([cg.tiles[inv[i]].get_perimeter() for i in range(n)], dtype=np.float64)
            try:
                lay._tile_perimeters = per
            except AttributeError:
                pass
        perims[pk.node_ptr_h[k]:pk.node_ptr_h[k + 1]] = per.astype(np.float32)            # (losses.py: torch.from_numpy(perims).float())
    predict = torch.from_numpy(np.concatenate(selections).astype(np.float32) if pk.n else np.zeros(1, dtype=np.float32)).to(dev)
    per_dev = torch.from_numpy(perims).to(dev)
    words = torch.zeros(K, dtype=torch.int32)
    words[scored] = 1
    words = words.to(dev)
    sums = torch.zeros(K, 3, dtype=torch.float64, device=dev)
    ws_bytes = int(lib.tgnn_solution_score_sums_many_workspace_bytes(K))
    ws = torch.empty(ws_bytes, dtype=torch.uint8, device=dev)
    with torch.cuda.device(dev):
        check(lib.tgnn_solution_score_sums_many(K, ptr(words), ptr(pk.node_ptr), ptr(pk.adj_ptr), pk.n, pk.ea, ptr(predict),
                                                C.c_void_p(pk.x.data_ptr() + 4 * (pk.fx - 1)), pk.fx, ptr(per_dev),
                                                ptr(pk.adj) if pk.ea else None, C.c_void_p(pk.attr.data_ptr() + 4) if pk.ea else None,
                                                pk.fe, ptr(sums), ptr(ws), ws_bytes, _lib.current_stream(dev)))
    sums_h = sums.cpu().tolist()
    wc, wl, wa = loss_weights()
    scores = [None] * K
    for k in scored:
        s0, s1, s2 = sums_h[k]
        if math.isnan(s0) or math.isnan(s1):
            raise IndexError(f"edge index out of range [0, {pk.nodes(k)}) in the align_edge_index of layout {k}")
        cg = originals[k].complete_graph
        e_adj = pk.adj_ptr_h[k + 1] - pk.adj_ptr_h[k]
        filled_area = s0 * float(cg.max_area) / float(areas[k])                           # Losses.solution_score, term for term
        assert -1e-7 <= filled_area <= 1 + 1e-7, filled_area
        loss_align_length = s1 * float(cg.max_align_length) if e_adj else 0.0
        ratio = loss_align_length / s2
        assert -1e-7 < ratio < 1 + 1e-7, ratio
        scores[k] = float(wa * filled_area + wl * ratio)
    return scores


def create_score(selection, origin_layout, score_fn=None, device=None):
    """The score half of `create_solution` (algorithms.py:210-220)."""
    if score_fn is not None:
        return score_fn(selection, origin_layout)
    has_area = getattr(origin_layout, "super_contour_area", None) is not None or hasattr(origin_layout, "get_super_contour_poly")
    if getattr(origin_layout, "complete_graph", None) is None or not has_area:
        return None
    from ..solver.ml_solver.losses import Losses
    return Losses.solution_score(selection, origin_layout, device=device)


def solve_many_hole_free(ml_solver, layouts, seeds, score_fn=None, max_rounds=100000):
    """K hole-free solves -- `solve_by_probablistic_greedy(ml_solver, layouts[k], check_holes=True)` after
    `np.random.seed(seeds[k])` -- in ONE loop, for layouts cut from ONE complete graph: per round one compaction call for all
    layouts (`tgnn_sublayout_compact_many`) with its read-back of the sub-layouts' sizes, ONE `ml_solver.predict_many` over the
    active layouts' sub-layouts, ONE sweep call (`DeviceHoleSweep.round`, csrc/hole_sweep.hip: a block per layout) and its one
    read-back, whatever K.  Parallel across layouts, SEQUENTIAL within one -- the only shape in which the reference's veto is
    defined -- so result k is bit for bit the solo solve's: selection, predict_order, round count, vetoes.  Layout k draws from
    `np.random.RandomState(seeds[k])`, the stream `np.random.seed(seeds[k])` gives the global generator; numpy's global stream
    is not touched.  A layout without nodes returns what the single-layout loop returns for it.
    Every sub-layout handed to `predict_many` carries `.origin_index`, its layout's place in `layouts`.
    Returns a list of K (selection, score, predict_order); `.last_rounds`, `.last_vetoes` [K], `.last_sweep_calls` (sweep calls
    queued = the rounds of the longest solve), `.last_first_probs` (the first round's probabilities per layout, numpy),
    `.last_guard` (the `DeviceHoleSweep`)."""
    layouts = list(layouts)
    K = len(layouts)
    fn = solve_many_hole_free
    fn.last_rounds, fn.last_vetoes, fn.last_sweep_calls, fn.last_first_probs, fn.last_guard = [], [], 0, [], None
    if K == 0:
        return []
    seeds = [int(s) for s in seeds]
    if len(seeds) != K:
        raise ValueError(f"seeds: one per layout ({K}), got {len(seeds)}")
    for k, lay in enumerate(layouts):
        if getattr(lay, "complete_graph", None) is None or getattr(lay, "inverse_index", None) is None:
            raise ValueError(f"layout {k}: a hole-free solve needs the layout's complete_graph (tile rings) and inverse_index: a "
                             "BrickLayout, not a bare DeviceLayout")
        if lay.complete_graph is not layouts[0].complete_graph:
            raise ValueError(f"layout {k} is cut from another complete graph than layout 0: one call solves layouts of ONE graph")
    device = ml_solver.device
    sizes = [int(np.asarray(lay.node_feature).shape[0]) for lay in layouts]
    empty = {}
    for k in range(K):
        if sizes[k] == 0:                                       # what the single-layout loop makes of it (it draws nothing)
            keep = np.random.get_state()
            empty[k] = solve_by_probablistic_greedy(ml_solver, layouts[k], score_fn=score_fn, check_holes=True)
            np.random.set_state(keep)
    pk = PackedLayouts(layouts, device)
    dev = pk.device
    cols = [np.asarray(lay.collide_edge_index).reshape(2, -1) for lay in layouts]
    dsw = DeviceHoleSweep(layouts[0].complete_graph, [(sizes[k], cols[k], layouts[k].inverse_index) for k in range(K)],
                          [np.random.RandomState(s) for s in seeds], dev)
    fn.last_guard = dsw
    n_tot, ea_tot, ec_tot = pk.n, pk.ea, pk.ec
    i64, i32 = torch.int64, torch.int32
    x_out = torch.empty(max(n_tot, 1), pk.fx, dtype=torch.float32, device=dev)
    inverse = torch.empty(max(n_tot, 1), dtype=i64, device=dev)
    adj_out = torch.empty(2 * max(ea_tot, 1), dtype=i64, device=dev)
    attr_out = torch.empty(max(ea_tot, 1), pk.fe, dtype=torch.float32, device=dev)
    col_out = torch.empty(2 * max(ec_tot, 1), dtype=i64, device=dev)
    tail = torch.zeros(4 * K, dtype=i64, device=dev)            # counts [K][3] | error words [K] int32
    counts, err = tail[:3 * K], tail[3 * K:].view(i32)[:K]
    tail_h = torch.empty(4 * K, dtype=i64, pin_memory=True)
    act_words = torch.zeros(K, dtype=i32, device=dev)
    cws_bytes = int(lib.tgnn_sublayout_compact_many_workspace_bytes(K, n_tot, ea_tot, ec_tot))
    cws = torch.empty(cws_bytes, dtype=torch.uint8, device=dev)
    first_probs = [None] * K
    rounds = [0] * K
    sent = None
    rnd = 0
    while True:
        active = dsw.active()
        if not any(active):
            break
        rnd += 1
        if rnd > max_rounds:
            raise RuntimeError(f"solve_many_hole_free: layouts {[k for k in range(K) if active[k]]} still have unlabelled nodes "
                               f"after {max_rounds} rounds")
        if active != sent:                                      # (only when a layout has finished)
            act_words.copy_(torch.tensor([int(a) for a in active], dtype=i32), non_blocking=False)
            sent = active
        check(lib.tgnn_sublayout_compact_many(K, ptr(act_words), ptr(pk.node_ptr), ptr(pk.adj_ptr), ptr(pk.col_ptr), n_tot, ea_tot, ec_tot,
                                              ptr(dsw.unlabelled), ptr(pk.x), pk.fx, ptr(pk.adj), ptr(pk.attr), pk.fe, ptr(pk.col),
                                              ptr(x_out), ptr(inverse), ptr(adj_out), ptr(attr_out), ptr(col_out), ptr(counts), ptr(err),
                                              ptr(cws), cws_bytes, _lib.current_stream(dev)))
        tail_h.copy_(tail, non_blocking=True)
        torch.cuda.current_stream(dev).synchronize()
        host = tail_h.numpy()
        bad = [k for k in range(K) if host[3 * K:].view(np.int32)[k]]
        if bad:
            raise IndexError(f"edge index out of range in layout {bad[0]} of {K}")
        cnt = host[:3 * K].reshape(K, 3)
        members, subs = [k for k in range(K) if active[k]], []
        for k in members:
            n2, ea2, ec2 = (int(v) for v in cnt[k])
            sub = pk.view(k, x_out, adj_out, attr_out, col_out, n2, ea2, ec2, inverse)
            sub.origin_index = k
            subs.append(sub)
            rounds[k] = rnd
        probs = [None] * K
        for k, p in zip(members, ml_solver.predict_many(subs)):
            probs[k] = p
            if rnd == 1:
                first_probs[k] = np.array(p, copy=True)
        dsw.round(probs)
    results = []
    for k in range(K):
        if k in empty:
            results.append(empty[k])
            continue
        sw = dsw.sweeps[k]
        results.append((sw.selection, create_score(sw.selection, layouts[k], score_fn, device), sw.order))
    fn.last_rounds, fn.last_vetoes, fn.last_sweep_calls = rounds, [int(v) for v in dsw.vetoes], dsw.calls
    fn.last_first_probs = first_probs
    return results


# ------------------------------------------------------------------------------------------------ the tree search
TREE_EPS = 1e-7                                                 # (the reference's EPS, algorithms.py:16)
TREE_ALPHA = 100.0                                              # (get_nodes_order_array, :228)


def _tree_sampling_probabilities(prob_m):
    """get_nodes_order_array (:228-231): softmax(100 prob_m) clipped to [1e-7, 1 - 1e-7] and normalised -- with the builtin `sum`
    the reference uses, whose order of additions is not numpy's."""
    x = prob_m * TREE_ALPHA
    x = x - np.max(x)
    exp_x = np.exp(x)
    sampling_prob = np.clip(exp_x / np.sum(exp_x), a_min=1e-7, a_max=1 - 1e-7)
    return sampling_prob / sum(sampling_prob)


class DeviceTreeSweep:
    """The branch sweeps of `solve_by_treesearch` ON THE DEVICE (csrc/tree_sweep.hip: tgnn_tree_sweep_many), a sibling of
    `DeviceHoleSweep`: K branches of ONE layout per call, a block per branch, each on its own slot of a state pool.  Per call ONE
    host-to-device copy (slots, visiting orders, prob_m, uniforms), one library call -- the fork of every parent slot into its
    child slots and the walks -- and ONE device-to-host copy (counters, accepted and killed nodes, the trace).
    The pool: `unlabelled` [S, n] int32 (a slot's row is the alive mask the sub-layout compaction reads) and, with the
    geometry, `tile_alive`, `label`, `chi_cache` [S, n_tiles] as `DeviceHoleSweep` keeps them per layout.  `new_slot()` hands out
    a free slot (the pool doubles when none is left: every row is copied, no state is dropped), `release(slot)` takes one back,
    `reset(slot)` makes it the empty selection.
    `sweep(branches)`: branches = (parent slot, child slot, nodes in visiting order, prob_m by position, rng) each.  The slot
    contract of include/tgnn.h is checked here, on the host tables, before anything is copied.  The RNG hand-over is
    `DeviceHoleSweep`'s, per branch (`_AheadDraws`).  Returns per branch (stats row [8], accepted nodes, killed nodes) as numpy
    copies.
    geometry: keep the tile state (needed by check_holes; default: only with check_holes).  `calls`, `branches`, `vetoes` count
    the sweep calls queued, the branches swept and the vetoes met; `trace`, `visit_ptr`, `visit_node` are the last call's (views
    of the staging buffers, valid until the next call)."""

    def __init__(self, complete_graph, n, collide_edge_index, inverse_index, check_holes, device=None, slots=8, geometry=None):
        self.check_holes = bool(check_holes)
        self.geometry = self.check_holes if geometry is None else bool(geometry)
        if self.check_holes and not self.geometry:
            raise ValueError("DeviceTreeSweep: check_holes needs the geometry")
        self.n = n = int(n)
        host = HostSweep(n, collide_edge_index)                 # (the collision rows in edge order)
        self.has_col = host.has_col
        self.starts = host.starts if host.has_col else np.zeros(n + 1, dtype=np.int64)
        self.nbr = host.nbr if host.has_col else np.zeros(0, dtype=np.int64)
        self.n_nbr = int(self.nbr.shape[0])
        self.on_device, self.n_tiles, tiles = None, 0, None
        if self.geometry:
            from .data_util import graph_on_device
            self.on_device = graph_on_device(complete_graph, device)
            device, self.n_tiles = self.on_device.device, self.on_device.n_tiles
            tiles = _tiles_of_nodes(inverse_index, n, self.n_tiles)
        self.device = dev = torch.device(device)
        if max(n, self.n_nbr, self.n_tiles) >= 2 ** 31 - 1:
            raise ValueError("DeviceTreeSweep: more than 2^31 nodes or collision entries")
        up = lambda a: torch.from_numpy(np.ascontiguousarray(a, dtype=np.int32)).to(dev)
        self.tile_of_node = up(tiles) if tiles is not None else None
        self.nbr_ptr, self.nbr_idx = up(self.starts), up(self.nbr if self.n_nbr else np.zeros(1))
        self.n_slots = 0
        self.unlabelled = self.tile_alive = self.label = self.chi_cache = None
        self._free = []
        self._grow(max(int(slots), 1))
        self._cap_k = self._cap_v = 0
        self.calls = self.branches = self.vetoes = 0
        self.trace = self.visit_ptr = self.visit_node = None

    # ---------------------------------------------------------------- the pool
    def _grow(self, n_slots):
        dev, i32, old = self.device, torch.int32, self.n_slots
        rows = [(self.unlabelled, max(self.n, 1), 1)]
        if self.geometry:
            rows += [(self.tile_alive, self.n_tiles, 0), (self.label, self.n_tiles, -1), (self.chi_cache, self.n_tiles, -2 ** 31)]
        grown = []
        for had, width, fill in rows:
            t = torch.full((n_slots, width), fill, dtype=i32, device=dev)
            if had is not None:
                t[:old].copy_(had)
            grown.append(t)
        self.unlabelled = grown[0]
        if self.geometry:
            self.tile_alive, self.label, self.chi_cache = grown[1:]
        self._free.extend(range(n_slots - 1, old - 1, -1))      # (popped from the end: the lowest free slot first)
        self.n_slots = n_slots

    def new_slot(self) -> int:
        if not self._free:
            self._grow(2 * self.n_slots)
        return self._free.pop()

    def release(self, slot):
        self._free.append(int(slot))

    def reset(self, slot):
        """Slot `slot` becomes the empty selection (a root of a search)."""
        self.unlabelled[slot].fill_(1)
        if self.geometry:
            self.tile_alive[slot].zero_()
            self.label[slot].fill_(-1)
            self.chi_cache[slot].fill_(-2 ** 31)                # TGNN_SWEEP_CHI_UNKNOWN

    @staticmethod
    def check_slots(parents, children, n_slots):
        """The slot contract of tgnn_tree_sweep_many on the host tables."""
        parents, children = [int(s) for s in parents], [int(s) for s in children]
        for s in parents + children:
            if not 0 <= s < n_slots:
                raise ValueError(f"DeviceTreeSweep: slot {s} outside the pool of {n_slots}")
        if len(set(children)) != len(children):
            raise ValueError("DeviceTreeSweep: two branches of a call share a child slot")
        for k, (par, child) in enumerate(zip(parents, children)):
            if child == par:
                if parents.count(par) != 1:
                    raise ValueError(f"DeviceTreeSweep: branch {k} reuses its parent's slot {par}, which another branch forks as well")
            elif child in parents:
                raise ValueError(f"DeviceTreeSweep: the child slot {child} of branch {k} is a parent slot of the call")

    # ---------------------------------------------------------------- the staging buffers
    def _stage(self, k, v):
        if k <= self._cap_k and v <= self._cap_v:
            return
        self._cap_k, self._cap_v = max(k, 2 * self._cap_k), max(v, 2 * self._cap_v)
        self._staging = _SweepStaging(self.device, self._cap_k, self._cap_v, ("parent", "slot"))
        self._ws = torch.empty(self._cap_k, dtype=torch.int32, device=self.device)

    def sweep(self, branches) -> list:
        from .data_util import tree_sweep_call
        branches = list(branches)
        K = len(branches)
        if K == 0:
            return []
        self.check_slots([b[0] for b in branches], [b[1] for b in branches], self.n_slots)
        self._stage(K, sum(len(b[2]) for b in branches))
        st = self._staging
        h, d = st.host, st.dev
        st.begin()
        for k, (parent, child, nodes, prob_m, rng) in enumerate(branches):
            h["parent"][k], h["slot"][k] = parent, child
            st.add(k, nodes, prob_m, rng)
            h["visit_ptr"][k + 1] = st.v
        if st.v == 0:
            return [(np.zeros(8, dtype=np.int32), np.zeros(0, dtype=np.int64), np.zeros(0, dtype=np.int64))] * K
        st.send()
        args = (self.n, self.tile_of_node, self.nbr_ptr, self.nbr_idx, self.n_nbr, self.n_slots, self.unlabelled, self.tile_alive,
                self.label, self.chi_cache, K, d["parent"], d["slot"], d["visit_ptr"], d["visit_node"], d["rate"], d["u"], st.v,
                self.check_holes, d["stats"], d["accepted"], d["killed"], d["trace"], d["err"], self._ws)
        if self.geometry:
            self.on_device.tree_sweep_into(*args)
        else:
            tree_sweep_call(self.device, None, *args)
        st.fetch()
        self.calls += 1
        self.branches += K
        self.trace, self.visit_ptr, self.visit_node = h["trace"].reshape(-1, 2), h["visit_ptr"], h["visit_node"]
        out = [st.result(k, f"tgnn_tree_sweep_many (branch {k})") for k in range(K)]
        self.vetoes += sum(int(row[1]) for row, _, _ in out)
        return out


class _TreeState:
    """A queued partial selection of `solve_by_treesearch`: its slot of the device pool and what the host keeps beside it."""

    def __init__(self, slot, n):
        self.slot = slot
        self.saved = np.ones(n)                                 # SelectionSolution.unlabelled_nodes (:285): 1.0, kept as the reference has it
        self.unlabelled = np.ones(n, dtype=bool)
        self.order = []
        self.depth = 0

    def fork(self, slot):
        child = _TreeState.__new__(_TreeState)
        child.slot, child.saved, child.unlabelled, child.order, child.depth = slot, self.saved.copy(), self.unlabelled.copy(), list(self.order), self.depth
        return child


def solve_by_treesearch(ml_solver, origin_layout, is_random_network=False, time_limit=None, top_k=4, check_holes=False,
                        max_predictions=None, beam=8, roots=1, seed=0, literal=False, score_fn=None):
    """The reference's tree search (algorithms.py:66-181) with the branch sweeps on the device (`DeviceTreeSweep`,
    csrc/tree_sweep.hip): a queue of partial selections; a popped state is scored once (`ml_solver.predict_top_maps`: the
    probabilities of its min(top_k, M) best maps, best first) and expanded into one branch per map -- the saved
    log-probabilities are updated (:111-125), a visiting order is sampled (get_nodes_order_array, :223-234) and the branch is
    swept (:138-157): an already labelled node is passed over with probability prob_m and ends the walk otherwise, with
    check_holes a tile that would enclose a gap is passed over (:150-152), every other node is accepted.  A branch that still has
    unlabelled nodes and accepted something goes back on the queue; every other one is finished and recorded once per distinct
    selection.  Returns (results, predict_cnt): results = [(selection, score, predict_order)] sorted by score, best first, with a
    stable sort (left in the order found when the layout cannot be scored), predict_cnt = the states popped.
    Two repairs of the reference's dead calls: the solver hands back the top maps itself, and `is_random_network` must be False.
    The default is the BATCHED search: `roots` empty selections; per step min(beam, len(queue)) states are popped one at a time
    with `random.Random(seed)`; a state's exponent is 1 / its own number of predictions; branch number s (step, pop order, map
    rank) draws its order and its uniforms from `np.random.RandomState([seed, s])`; per step ONE `predict_top_maps` call, ONE
    sweep call for all branches and one read-back; neither global generator is touched.
    literal=True (beam = roots = 1) follows the reference decision for decision: pops from the `random` module, the exponent
    1 / predict_cnt of the global count, `np.random.choice` and the draws from numpy's global stream, the branches of a state
    swept one after another (a sweep call each: branch m + 1's choice follows branch m's draws in the stream).
    Stops when the queue is empty, after `max_predictions` pops or after `time_limit` seconds; one of the two must be given.
    check_holes needs the layout's `complete_graph` and `inverse_index`.  There is no host sweep to fall back to.
    `.last_sweep` is the `DeviceTreeSweep` (`calls`, `branches`, `vetoes`), `.last_steps` the number of steps."""
    import random as _random
    import time as _time
    if is_random_network:
        raise ValueError("solve_by_treesearch: is_random_network must be False (the reference's random-network predict does not exist)")
    if max_predictions is None and time_limit is None:
        raise ValueError("solve_by_treesearch: give max_predictions or time_limit; the queue need not run empty")
    if literal and (beam != 1 or roots != 1):
        raise ValueError("solve_by_treesearch: literal=True is the reference's search: beam == 1 and roots == 1")
    if beam < 1 or roots < 1 or top_k < 1:
        raise ValueError("solve_by_treesearch: beam, roots and top_k are at least 1")
    if check_holes and (getattr(origin_layout, "complete_graph", None) is None or getattr(origin_layout, "inverse_index", None) is None):
        raise ValueError("check_holes needs the layout's complete graph (tile rings) and inverse_index: a BrickLayout, not a "
                         "bare DeviceLayout")
    device = ml_solver.device
    origin = origin_layout if isinstance(origin_layout, DeviceLayout) else DeviceLayout.upload(origin_layout, device)
    dev = origin.node_feature.device
    n = int(origin.node_feature.shape[0])
    if n == 0:
        raise ValueError("solve_by_treesearch: a layout without nodes")
    col_host = origin.collide_edge_index.cpu().numpy()
    dsw = DeviceTreeSweep(getattr(origin_layout, "complete_graph", None), n, col_host, getattr(origin_layout, "inverse_index", None),
                          check_holes, dev, slots=max(8, roots + beam * top_k))
    fn = solve_by_treesearch
    fn.last_sweep, fn.last_steps = dsw, 0
    builders = []
    pop_rng = _random if literal else _random.Random(seed)
    queue = []
    for _ in range(roots):
        queue.append(_TreeState(dsw.new_slot(), n))             # (a fresh pool: every slot is the empty selection)
    results, seen = [], set()
    predict_cnt = n_branches = 0
    start = _time.time()

    def running():
        return (len(queue) > 0 and (max_predictions is None or predict_cnt < max_predictions)
                and (time_limit is None or _time.time() - start < time_limit))

    def finish(state, stats, acc, gone):
        state.unlabelled[acc] = False
        state.unlabelled[gone] = False
        state.order.extend(int(i) for i in acc)
        if state.unlabelled.any() and len(acc) > 0:             # (:166)
            queue.append(state)
            return
        dsw.release(state.slot)
        selection = np.zeros(n)
        selection[state.order] = 1
        key = selection.tobytes()                               # (:172: one entry per distinct selection)
        if key not in seen:
            seen.add(key)
            results.append((selection, create_score(selection, origin_layout, score_fn, device), state.order))

    while running():
        popped = []
        for _ in range(min(beam, len(queue))):
            if not running():
                break
            state = queue.pop(pop_rng.randint(0, len(queue) - 1))     # (:89-90)
            predict_cnt += 1
            state.depth += 1
            popped.append((state, predict_cnt))
        fn.last_steps += 1
        while len(builders) < len(popped):
            builders.append(SubLayoutBuilder(origin))
        subs = []
        for builder, (state, cnt) in zip(builders, popped):
            sub = builder.build(dsw.unlabelled[state.slot])     # (the slot's own row on the device: nothing to upload)
            sub.predict_index, sub.origin_index = cnt, 0
            subs.append(sub)
        maps = ml_solver.predict_top_maps(subs, top_k)
        pending, children, parents = [], [], []
        for (state, cnt), prob in zip(popped, maps):
            ids = np.flatnonzero(state.unlabelled)
            prob = np.asarray(prob)
            prob = prob.reshape(len(ids), -1)
            n_maps = prob.shape[1]
            for m in range(n_maps):
                log_prob_network = np.log(np.clip(prob[:, m], TREE_EPS, 1.0))                       # (:111; float32 stays float32)
                log_prob_m = state.saved[ids] + log_prob_network                                   # (:112)
                prob_m = np.exp(log_prob_m / (predict_cnt if literal else state.depth))             # (:113)
                child = state.fork(state.slot if n_maps == 1 else dsw.new_slot())
                child.saved[ids] = log_prob_m
                rng = np.random if literal else np.random.RandomState([seed, n_branches])
                n_branches += 1
                order = rng.choice(len(ids), len(ids), replace=False, p=_tree_sampling_probabilities(prob_m))     # (:232)
                branch = (state.slot, child.slot, ids[order], prob_m[order], rng)
                if literal:
                    finish(child, *dsw.sweep([branch])[0])
                else:
                    pending.append(branch)
                    children.append(child)
            if n_maps != 1:
                parents.append(state.slot)
        if not literal:
            for child, res in zip(children, dsw.sweep(pending)):
                finish(child, *res)
        for slot in parents:                                    # (forked into fresh slots: the parent's own is free again)
            dsw.release(slot)
    if results and all(r[1] is not None for r in results):
        results = sorted(results, key=lambda tup: tup[1], reverse=True)                             # (:180)
    return results, predict_cnt
