"""Layout producer and brick-layout files (/root/reference/util/data_util.py).

Same functions, same argument meaning, same return values (down to dtype and to the shape-(0,) arrays the reference
hands back for an empty edge list) as the reference's module; what changed is how the work is done:

  generate_brick_layout_data      :164-205  per-edge dict look-ups, a Python loop per tile
      -> one searchsorted over the graph's (u, v) keys + three fancy-index gathers (GraphArrays, tile_graph.py).
  recover_features_from_reindex   :144-162  `edge[0] in tiles_super_set and ...` over ALL edges with a LIST on the right
      (O(E * N); 132 ms for the full 1 254-tile labyrinth graph here) -> a boolean membership mask, O(E + N), 2.3 ms.
  layout_on_device                (new)     the same super-set cut carried out on the GPU: the complete graph is uploaded
      once (`CompleteGraphOnDevice`), a layout is its `alive` mask run through `tgnn_sublayout_compact`
      (csrc/graph_prep.hip) -- the arrays `to_torch_tensor` (:110-117) would have produced, without a host copy.
  tiles_in_regions                (new)     the tile-in-region predicate of tile_factory.py:39 (`contain`, util/algo_util.py:
      143-144) for K target regions at once (csrc/region.hip); the tile geometry is uploaded on first use.
  write_brick_layout_data / load_brick_layout_data / write_bricklayout / load_bricklayout   :18-78
      the same pickle schema; read through the schema-restricted unpickler of tile_graph.py.
"""
from __future__ import annotations

import math
import os
import pickle
from collections import defaultdict

import numpy as np

from ..tiling.tile_graph import TileGraph, load_schema_pickle, _reference_names

optional_variables_names = ['node_features', 'collide_edge_index', 'collide_edge_features', 'align_edge_index',
                            'align_edge_features', 'predict', 'predict_order', 'target_shape', 'predict_probs']


# ------------------------------------------------------------------------------------------ files
def write_brick_layout_data(save_path, re_index, node_features=None, collide_edge_index=None,
                            collide_edge_features=None, align_edge_index=None, align_edge_features=None, prefix=None,
                            predict=None, predict_order=None, target_shape=None, predict_probs=None):
    """data_util.py:18-33."""
    if not os.path.exists(prefix):
        os.mkdir(prefix)
    given = locals()
    dic = {"re_index": re_index}
    for name in optional_variables_names:
        if given[name] is not None:
            dic[name] = given[name]
    with _reference_names():
        data = pickle.dumps(dic)
    with open(os.path.join(prefix, save_path), "wb") as f:
        f.write(data)


def load_brick_layout_data(save_path):
    """data_util.py:38-56."""
    f = load_schema_pickle(save_path)
    assert 're_index' in f.keys()
    return (f['re_index'],) + tuple(f.get(name) for name in optional_variables_names)


def load_bricklayout(file_path, complete_graph):
    """data_util.py:58-78."""
    from ..tiling.brick_layout import BrickLayout
    re_index, node_features, collide_edge_index, collide_edge_features, align_edge_index, align_edge_features, \
        predict, predict_order, target_polygon, predict_probs = load_brick_layout_data(file_path)
    if node_features is None or collide_edge_index is None or collide_edge_features is None or \
            align_edge_index is None or align_edge_features is None:
        node_features, collide_edge_index, collide_edge_features, align_edge_index, align_edge_features = \
            recover_features_from_reindex(re_index, complete_graph)
    layout = BrickLayout(complete_graph, node_features, collide_edge_index, collide_edge_features, align_edge_index,
                         align_edge_features, re_index)
    if predict is not None:
        layout.predict = predict
    if predict_order is not None:
        layout.predict_order = predict_order
    if target_polygon is not None:
        layout.target_polygon = target_polygon
    if predict_probs is not None:
        layout.predict_probs = predict_probs
    return layout


def write_bricklayout(folder_path, file_name, brick_layout, with_features=True):
    """data_util.py:80-108."""
    feats = dict(node_features=brick_layout.node_feature, collide_edge_index=brick_layout.collide_edge_index,
                 collide_edge_features=brick_layout.collide_edge_features,
                 align_edge_index=brick_layout.align_edge_index,
                 align_edge_features=brick_layout.align_edge_features) if with_features else {}
    write_brick_layout_data(save_path=file_name, re_index=brick_layout.re_index, prefix=folder_path,
                            predict=brick_layout.predict, predict_order=brick_layout.predict_order,
                            target_shape=brick_layout.target_polygon, predict_probs=brick_layout.predict_probs, **feats)


def to_torch_tensor(device, node_feature, align_edge_index, align_edge_features, collide_edge_index,
                    collide_edge_features):
    """data_util.py:110-117."""
    import torch
    return (torch.from_numpy(node_feature).float().to(device), torch.from_numpy(align_edge_index).long().to(device),
            torch.from_numpy(align_edge_features).float().to(device),
            torch.from_numpy(collide_edge_index).long().to(device),
            torch.from_numpy(collide_edge_features).float().to(device))


# ------------------------------------------------------------------------------------------ producer, host
def generate_brick_layout_data(graph: TileGraph, super_tiles: list, collide_edges, adj_edges):
    """data_util.py:164-205.  `collide_edges` / `adj_edges`: lists of (u, v) complete-graph pairs as in the reference.
    Returns node_feature [n, types + 1] f64, collide index [2, Ec] (or shape (0,)), collide features [Ec, F] f64,
    adjacency index, adjacency features (column 1 / max_align_length), re_index."""
    a = graph.arrays
    col = np.asarray(collide_edges, dtype=np.int64).reshape(-1, 2).T
    adj = np.asarray(adj_edges, dtype=np.int64).reshape(-1, 2).T
    super_arr = np.asarray(super_tiles, dtype=np.int64).reshape(-1)
    return _produce(a, super_arr, col, a.edge_rows(0, col), adj, a.edge_rows(1, adj), super_tiles)


def _produce(a, super_arr, col, col_rows, adj, adj_rows, super_tiles):
    n = super_arr.shape[0]
    re_index = defaultdict(int)                                   # :178-180
    for i, t in enumerate(super_tiles):
        re_index[t] = i
    lookup = np.zeros(a.n_tiles, dtype=np.int64)                   # defaultdict(int): unknown tile -> 0
    lookup[super_arr] = np.arange(n)
    node_feature = np.zeros((n, a.tile_type_count + 1))            # :183-187
    node_feature[np.arange(n), a.tile_ids[super_arr]] = 1
    node_feature[:, -1] = a.tile_areas[super_arr] / a.max_area
    colf = a.colli_features[col_rows]
    adjf = a.adj_features[adj_rows]
    if adjf.shape[0] > 0:
        adjf[:, 1] = adjf[:, 1] / a.max_align_length               # :168-169
    empty = np.array([])                                          # np.array([]).T of an empty list: shape (0,), float64
    return (node_feature,
            lookup[col] if col.shape[1] else empty.copy(), colf if col.shape[1] else empty.copy(),
            lookup[adj] if adj.shape[1] else empty.copy(), adjf if adj.shape[1] else empty.copy(), re_index)


def filter_edges(graph: TileGraph, tiles_super_set):
    """The two comprehensions of tile_factory.py:42-45 / data_util.py:148-151 as a membership mask: rows (into the
    graph's edge arrays) of the edges with both ends in the super set, in file order."""
    a = graph.arrays
    member = np.zeros(a.n_tiles, dtype=bool)
    member[np.asarray(tiles_super_set, dtype=np.int64).reshape(-1)] = True
    col_rows = np.flatnonzero(member[a.colli_edges[0]] & member[a.colli_edges[1]])
    adj_rows = np.flatnonzero(member[a.adj_edges[0]] & member[a.adj_edges[1]])
    return col_rows, adj_rows


def recover_features_from_reindex(re_index, complete_graph: TileGraph):
    """data_util.py:144-162."""
    tiles_super_set = list(re_index.keys())
    a = complete_graph.arrays
    col_rows, adj_rows = filter_edges(complete_graph, tiles_super_set)
    out = _produce(a, np.asarray(tiles_super_set, dtype=np.int64).reshape(-1), a.colli_edges[:, col_rows], col_rows,
                   a.adj_edges[:, adj_rows], adj_rows, tiles_super_set)
    for key, item in out[5].items():
        assert re_index[key] == item                               # :158-159
    return out[:5]


def create_brick_layout_from_super_set(graph: TileGraph, tiles_super_set):
    """tile_factory.py:49-58 after the polygon test: the six producer outputs for a given list of tiles.  (Which tiles
    lie inside a target polygon, tile_factory.py:39, is answered on the GPU: CompleteGraphOnDevice.tiles_in_regions.)"""
    a = graph.arrays
    col_rows, adj_rows = filter_edges(graph, tiles_super_set)
    return _produce(a, np.asarray(tiles_super_set, dtype=np.int64).reshape(-1), a.colli_edges[:, col_rows], col_rows,
                    a.adj_edges[:, adj_rows], adj_rows, list(tiles_super_set))


# ------------------------------------------------------------------------------------------ producer, device
def _union_api():
    """(torch, _lib, check, lib, ptr, UNION_TOL): what the union calls of CompleteGraphOnDevice need, imported on first use (this
    module imports without torch and without the library)."""
    import torch
    from .. import _lib
    from .._lib import check, lib, ptr
    from ..tiling.region import UNION_TOL
    return torch, _lib, check, lib, ptr, UNION_TOL


# the bits of the device error words (include/tgnn.h: TGNN_UNION_ERR_*, TGNN_TOPO_ERR_*, TGNN_CONTOUR_ERR_*)
_AREA_ERROR_BITS = {1: "collision index out of range",
                    2: "a tile side is covered in more separate stretches than the kernel's interval list holds"}
_TOPOLOGY_ERROR_BITS = {1: "collision or contact index out of range",            # (tgnn_union_hole_delta's too)
                        2: "more tiles meet in one point than the kernel's wedge list holds"}
_CONTOUR_ERROR_BITS = {1: "a collision or contact index out of range",
                       2: "more boundary pieces leave one point than the kernel's wedge list holds",
                       4: "more foreign vertices inside one tile side than the kernel's split list holds",
                       8: "an output or the workspace is too small",
                       16: "the boundary of a mask does not close: its tiles overlap"}


def _raise_device_error(name, code, bits, only_set=False):
    """TgnnError for the non-zero device error word `code` of entry point `name`, with the table of its bits (only_set: only
    the bits that are set)."""
    from .._lib import TgnnError
    listed = [f"{b}: {t}" for b, t in bits.items() if code & b or not only_set]
    raise TgnnError(f"{name}: device error word {code} (" + ("; " if only_set else ", ").join(listed) + ")")


class CompleteGraphOnDevice:
    """The complete graph resident in HBM: node features of ALL tiles, both edge lists, the normalised adjacency
    features, each converted exactly as `to_torch_tensor` converts a layout (float64 -> .float(), int -> .long()).
    Edge subsetting commutes with that conversion, so a layout cut out of these arrays on the device is bit-identical
    to the reference's host-side producer followed by the upload."""

    def __init__(self, graph: TileGraph, device):
        import torch
        from .algorithms import DeviceLayout, SubLayoutBuilder
        a = graph.arrays
        self.device = torch.device(device)
        self.n_tiles = a.n_tiles
        t = lambda arr, dt: torch.from_numpy(np.ascontiguousarray(arr)).to(dt).to(self.device)
        self.full = DeviceLayout(t(a.node_features(), torch.float32), t(a.adj_edges, torch.int64),
                                 t(a.adj_features_normalised(), torch.float32), t(a.colli_edges, torch.int64))
        self.adj_type = t(a.adj_type, torch.int32)
        self._builder = SubLayoutBuilder(self.full)
        self._alive = torch.zeros(self.n_tiles, dtype=torch.int32, device=self.device)
        self._graph = graph
        self._geometry = None
        self._union = self._rings_host = None
        self._topology = None

    def layout(self, tiles_super_set):
        """DeviceLayout of the given tiles (ASCENDING complete-graph ids: the order get_all_placement_in_polygon,
        tile_factory.py:39, and compute_sub_layout, brick_layout.py:250-252, both produce).  `inverse_index` maps layout
        node -> complete-graph tile (BrickLayout.inverse_index, brick_layout.py:42-44).  The result aliases this object's
        buffers: valid until the next call."""
        import torch
        s = np.asarray(tiles_super_set, dtype=np.int64).reshape(-1)
        if s.size and (np.any(np.diff(s) <= 0) or s[0] < 0 or s[-1] >= self.n_tiles):
            raise ValueError("the device producer takes strictly ascending tile ids; use "
                             "create_brick_layout_from_super_set for an arbitrary order")
        self._alive.zero_()
        if s.size:
            self._alive[torch.from_numpy(s).to(self.device)] = 1
        return self._builder.build(self._alive)


    # -------------------------------------------------------------------------- the tile-in-region predicate
    def _tile_geometry(self):
        """Tile triangles, triangle ranges, boxes, areas (the GEOS ring areas the reference compares against) and inside
        points, uploaded on first use."""
        if self._geometry is None:
            import torch
            from ..tiling.region import tile_geometry
            g = self._graph
            rings = [t.tile_poly.exterior for t in g.tiles]
            tri, tri_ptr, bbox, area, point = tile_geometry(rings, g.arrays.tile_areas)
            t = lambda arr: torch.from_numpy(np.ascontiguousarray(arr)).to(self.device)
            self._geometry = (t(tri), t(tri_ptr), t(bbox), t(area), t(point))
        return self._geometry

    def tiles_in_regions(self, regions, with_area=False):
        """alive [K, n_tiles] int32 on the device: 1 where |area(R_k n T_i) - area(T_i)| < 1e-6 (the reference's `contain`).
        `regions`: tiling.region.Region objects.  with_area: also area(R_k n T_i) [K, n_tiles] float64.  No host sync."""
        import torch
        from .. import _lib
        from .._lib import check, lib, ptr
        from ..tiling.region import pack_regions
        regions = list(regions)
        k = len(regions)
        alive = torch.empty(k, self.n_tiles, dtype=torch.int32, device=self.device)
        area = torch.empty(k, self.n_tiles, dtype=torch.float64, device=self.device) if with_area else None
        if k:
            tri, tri_ptr, bbox, t_area, point = self._tile_geometry()
            ring_xy, ring_ptr, region_ring_ptr, region_bbox, max_edges = pack_regions(regions)
            up = lambda arr: torch.from_numpy(np.ascontiguousarray(arr)).to(self.device, non_blocking=False)
            ring_xy_d = up(ring_xy if ring_xy.shape[0] else np.zeros((1, 2)))
            bufs = (ring_xy_d, up(ring_ptr), up(region_ring_ptr), up(region_bbox))
            check(lib.tgnn_tiles_in_region(ptr(tri), ptr(tri_ptr), ptr(bbox), ptr(t_area), ptr(point), self.n_tiles,
                                           *(ptr(b) for b in bufs), k, max_edges, ptr(alive), ptr(area),
                                           _lib.current_stream(self.device)))
        return (alive, area) if with_area else alive

    def region_edge_counts(self, alive):
        """[K, 2] int64 on the device: collision and adjacency edges of the complete graph with both ends alive."""
        import torch
        from .. import _lib
        from .._lib import check, lib, ptr
        k = int(alive.shape[0])
        counts = torch.empty(k, 2, dtype=torch.int64, device=self.device)
        err = torch.zeros(1, dtype=torch.int32, device=self.device)
        col, adj = self.full.collide_edge_index, self.full.align_edge_index
        if k:
            check(lib.tgnn_region_edge_counts(ptr(alive.contiguous()), k, self.n_tiles, ptr(col) if col.shape[1] else None,
                                              int(col.shape[1]), ptr(adj) if adj.shape[1] else None, int(adj.shape[1]),
                                              ptr(counts), ptr(err), _lib.current_stream(self.device)))
        return counts

    # -------------------------------------------------------------------------- the area of a union of tiles
    def _union_geometry(self):
        """Tile rings (open, counter-clockwise) and the collision edges as CSR, uploaded on first use; the graph is checked
        once for features the union's tolerance could not tell from noise (region.check_tolerance_gap)."""
        if self._union is None:
            import torch
            from ..tiling.region import check_tolerance_gap, union_geometry
            g = self._graph
            geo = union_geometry([t.tile_poly.exterior for t in g.tiles], g.arrays.colli_edges, self.n_tiles)
            check_tolerance_gap(*geo)
            self._rings_host = geo[:2]                           # (kept for _topology_geometry)
            self._union = tuple(torch.from_numpy(a if a.size else np.zeros(1, dtype=a.dtype)).to(self.device) for a in geo)
        return self._union

    def _as_masks(self, alive):
        """`alive` ([K, n_tiles] or [n_tiles], any integer or bool tensor) as a contiguous [K, n_tiles] int32 tensor on this
        device."""
        import torch
        alive = torch.as_tensor(alive, device=self.device)
        if alive.dim() == 1:
            alive = alive[None, :]
        if alive.dim() != 2 or alive.shape[1] != self.n_tiles:
            raise ValueError(f"alive must be [K, {self.n_tiles}], got {tuple(alive.shape)}")
        return (alive != 0).to(torch.int32).contiguous() if alive.dtype != torch.int32 else alive.contiguous()

    def union_areas(self, alive):
        """[K] float64 on the device: the area of the union of the tiles with alive[k, i] != 0 (`alive` [K, n_tiles] or
        [n_tiles], any integer or bool tensor on this device; what `tiles_in_regions` returns, or a solver's selection) -- the
        reference's `get_super_contour_poly().area` of that tile set.  csrc/union_area.hip; one device-to-host copy of the
        error word."""
        torch, _lib, check, lib, ptr, UNION_TOL = _union_api()
        alive = self._as_masks(alive)
        k = int(alive.shape[0])
        area =torch.empty(k, dtype=torch.float64, device=self.device)
        if k:
            ring_xy, ring_ptr, col_ptr, col_idx = self._union_geometry()
            err = torch.zeros(1, dtype=torch.int32, device=self.device)
            ws_bytes = int(lib.tgnn_union_area_workspace_bytes(k, self.n_tiles))
            ws = torch.empty(ws_bytes // 8, dtype=torch.float64, device=self.device)
            check(lib.tgnn_union_area(ptr(ring_xy), ptr(ring_ptr), self.n_tiles, ptr(col_ptr), ptr(col_idx), ptr(alive), k,
                                      UNION_TOL, ptr(area), ptr(err), ptr(ws), ws_bytes, _lib.current_stream(self.device)))
            code = int(err.item())
            if code:
                _raise_device_error("tgnn_union_area", code, _AREA_ERROR_BITS)
        return area

    # -------------------------------------------------------------------------- the topology of a union of tiles
    def _topology_geometry(self):
        """The contact relation as CSR and the sweep direction of tgnn_union_topology (region.contact_geometry,
        region.sweep_direction), made from the packed rings `_union_geometry` built on the host and uploaded on first use."""
        if self._topology is None:
            import torch
            from ..tiling.region import contact_geometry, sweep_direction
            self._union_geometry()
            ring_xy, ring_ptr = self._rings_host
            theta = sweep_direction(ring_xy, ring_ptr)
            touch = contact_geometry(ring_xy, ring_ptr)
            self._topology = tuple(torch.from_numpy(a if a.size else np.zeros(1, dtype=a.dtype)).to(self.device)
                                   for a in touch) + (math.cos(theta), math.sin(theta))
        return self._topology

    def union_topology(self, alive):
        """[K, 3] int32 on the device: {components, holes, status} of the union of the tiles with alive[k, i] != 0 (`alive`
        [K, n_tiles] or [n_tiles], any integer or bool tensor on this device) -- the connected components of the closed union
        (tiles sharing a single point are connected) and the bounded components of its complement, what the reference's
        `detect_holes` looks for.  For selections that do not overlap: a mask with two colliding alive tiles gets
        {-1, -1, 1}.  csrc/union_topology.hip; one device-to-host copy of the error word."""
        torch, _lib, check, lib, ptr, UNION_TOL = _union_api()
        alive = self._as_masks(alive)
        k = int(alive.shape[0])
        out = torch.empty(k, 3, dtype=torch.int32, device=self.device)
        if k:
            ring_xy, ring_ptr, col_ptr, col_idx = self._union_geometry()
            touch_ptr, touch_idx, dir_x, dir_y = self._topology_geometry()
            err = torch.zeros(1, dtype=torch.int32, device=self.device)
            ws_bytes = int(lib.tgnn_union_topology_workspace_bytes(k, self.n_tiles))
            ws = torch.empty(ws_bytes // 4, dtype=torch.int32, device=self.device)
            check(lib.tgnn_union_topology(ptr(ring_xy), ptr(ring_ptr), self.n_tiles, ptr(col_ptr), ptr(col_idx), ptr(touch_ptr),
                                          ptr(touch_idx), ptr(alive), k, UNION_TOL, dir_x, dir_y, ptr(out), ptr(err), ptr(ws),
                                          ws_bytes, _lib.current_stream(self.device)))
            code = int(err.item())
            if code:
                _raise_device_error("tgnn_union_topology", code, _TOPOLOGY_ERROR_BITS)
        return out

    def hole_deltas(self, alive):
        """(delta [K, n_tiles, 2] int32, state [K, n_tiles] int32) on the device: for every tile t of every mask (`alive` as for
        `union_topology`) what adding t would do -- delta[k, t] = {d components, d holes} = union_topology(mask k + {t}) -
        union_topology(mask k) -- where state[k, t] is 0 (a candidate); state 1: t is alive, 2: t collides with an alive tile,
        3: two alive tiles of the mask collide (the whole row); the delta is {0, 0} there.  What the reference's hole veto asks
        per tile (util/algorithms.py:150-152), for all tiles at once.  csrc/union_hole_delta.hip; one device-to-host copy of
        the error word."""
        import torch
        alive = self._as_masks(alive)
        k = int(alive.shape[0])
        delta = torch.empty(k, self.n_tiles, 2, dtype=torch.int32, device=self.device)
        state = torch.empty(k, self.n_tiles, dtype=torch.int32, device=self.device)
        if k and self.n_tiles:
            err = torch.zeros(1, dtype=torch.int32, device=self.device)
            self.hole_deltas_into(alive, delta, state, err)
            code = int(err.item())
            if code:
                _raise_device_error("tgnn_union_hole_delta", code, _TOPOLOGY_ERROR_BITS)
        return delta, state

    def hole_deltas_into(self, alive, delta, state, err):
        """The call of `hole_deltas` alone, queued on the current stream with nothing read back: `alive` [K, n_tiles] int32
        contiguous, `delta` / `state` / `err` int32 device buffers of 2 K n_tiles / K n_tiles / 1 words, `err` zeroed by the
        caller (util.algorithms.HoleGuard keeps the three in one buffer and reads it back in one copy)."""
        torch, _lib, check, lib, ptr, UNION_TOL = _union_api()
        k = int(alive.shape[0])
        ring_xy, ring_ptr, col_ptr, col_idx = self._union_geometry()
        touch_ptr, touch_idx, dir_x, dir_y = self._topology_geometry()
        ws_bytes = int(lib.tgnn_union_hole_delta_workspace_bytes(k, self.n_tiles))
        ws = torch.empty(ws_bytes // 4, dtype=torch.int32, device=self.device)
        check(lib.tgnn_union_hole_delta(ptr(ring_xy), ptr(ring_ptr), self.n_tiles, ptr(col_ptr), ptr(col_idx), ptr(touch_ptr),
                                        ptr(touch_idx), ptr(alive), k, UNION_TOL, dir_x, dir_y, ptr(delta), ptr(state),
                                        ptr(err), ptr(ws), ws_bytes, _lib.current_stream(self.device)))

    def _sweep_geometry(self):
        """The eight leading arguments of `tgnn_hole_sweep_many` and `tgnn_tree_sweep_many`: the rings, the contact rows, the
        tolerance and the sweep direction."""
        _, _, _, _, ptr, UNION_TOL = _union_api()
        ring_xy, ring_ptr, _, _ = self._union_geometry()
        touch_ptr, touch_idx, dir_x, dir_y = self._topology_geometry()
        return ptr(ring_xy), ptr(ring_ptr), self.n_tiles, ptr(touch_ptr), ptr(touch_idx), UNION_TOL, dir_x, dir_y

    def hole_sweep_into(self, k, node_ptr, n_nodes, tile_of_node, nbr_ptr, nbr_idx, n_nbr, unlabelled, tile_alive, label, chi_cache,
                        active, visit_ptr, visit_node, thr, u, n_visit, stats, accepted, killed, trace, err, ws=None):
        """One round of the hole-free greedy sweep of K layouts of this graph, queued on the current stream with nothing read
        back: the raw call of `tgnn_hole_sweep_many` (include/tgnn.h has the argument contract; csrc/hole_sweep.hip).  Every
        argument but the counts is a contiguous tensor on this device: int32, `thr` / `u` float64; `ws` int32 of at least K
        words (made here when None).  `util.algorithms.DeviceHoleSweep` keeps the state, the staging buffers and the RNG."""
        torch, _lib, check, lib, ptr, _ = _union_api()
        ws_bytes = int(lib.tgnn_hole_sweep_workspace_bytes(k))
        if ws is None:
            ws = torch.empty(max(ws_bytes // 4, 1), dtype=torch.int32, device=self.device)
        with torch.cuda.device(self.device):
            check(lib.tgnn_hole_sweep_many(*self._sweep_geometry(), k, ptr(node_ptr), n_nodes, ptr(tile_of_node), ptr(nbr_ptr),
                                           ptr(nbr_idx), n_nbr, ptr(unlabelled), ptr(tile_alive), ptr(label), ptr(chi_cache), ptr(active), ptr(visit_ptr),
                                           ptr(visit_node), ptr(thr), ptr(u), n_visit, ptr(stats), ptr(accepted), ptr(killed),
                                           ptr(trace), ptr(err), ptr(ws), 4 * int(ws.numel()),
                                           _lib.current_stream(self.device)))

    def tree_sweep_into(self, n_nodes, tile_of_node, nbr_ptr, nbr_idx, n_nbr, n_slots, unlabelled, tile_alive, label, chi_cache, k,
                        parent_slot, slot, visit_ptr, visit_node, p, u, n_visit, check_holes, stats, accepted, killed, trace, err,
                        ws=None, geometry=True):
        """One step of the tree search -- the sweeps of K branches of one layout of this graph, each on its own slot of the
        caller's state pool -- queued on the current stream with nothing read back: the raw call of `tgnn_tree_sweep_many`
        (include/tgnn.h has the argument contract and the slot contract; csrc/tree_sweep.hip).  Every argument but the counts is
        a contiguous tensor on this device: int32, `p` / `u` float64; `ws` int32 of at least K words (made here when None).
        geometry=False (check_holes == 0 only): the graph's rings and contact rows are not handed over and no tile state is
        kept -- `tile_of_node` and the three tile rows may be None.  `util.algorithms.DeviceTreeSweep` keeps the pool, the
        staging buffers and the RNGs."""
        tree_sweep_call(self.device, self._sweep_geometry() if geometry else None, n_nodes, tile_of_node, nbr_ptr, nbr_idx, n_nbr,
                        n_slots, unlabelled, tile_alive, label, chi_cache, k, parent_slot, slot, visit_ptr, visit_node, p, u, n_visit, check_holes, stats, accepted, killed,
                        trace, err, ws)

    # -------------------------------------------------------------------------- the outline of a union of tiles
    def union_contours(self, alive):
        """`UnionContours` of the K masks `alive` ([K, n_tiles] or [n_tiles], any integer or bool tensor on this device): the
        boundary rings of the closed union of the tiles with alive[k, i] != 0, one counter-clockwise ring per component (tiles
        sharing a single point are connected) and one clockwise ring per hole -- the reference's
        `get_selected_tiles_union_polygon` of that selection.  For selections that do not overlap: a mask with two colliding
        alive tiles gets status 1 and no rings.  csrc/union_contour.hip; the outputs are sized by the bound of 2 points per
        vertex of an alive tile (one device reduction), one device-to-host copy brings back the error word and the totals."""
        torch, _lib, check, lib, ptr, UNION_TOL = _union_api()
        alive = self._as_masks(alive)
        k = int(alive.shape[0])
        ring_xy, ring_ptr, col_ptr, col_idx = self._union_geometry()
        i32 = lambda *shape: torch.empty(*shape, dtype=torch.int32, device=self.device)
        f64 = lambda *shape: torch.empty(*shape, dtype=torch.float64, device=self.device)
        if k == 0:
            return UnionContours(ring_xy, ring_ptr, i32(0, 4), i32(0, 4), f64(0), f64(0, 2), i32(0))
        touch_ptr, touch_idx, _, _ = self._topology_geometry()
        verts = (ring_ptr[1:] - ring_ptr[:-1]).to(torch.float64)             # (exact in fp64: the counts are far below 2^53)
        bound = 2 * int(((alive != 0).to(torch.float64) @ verts).sum().item())
        if bound >= 2 ** 31:
            raise ValueError("too many tile vertices for one call; split the masks")
        cap_rings = bound // 3 + 1                               # (a ring has at least three points)
        mask_out, ring_out, ring_area = i32(k, 4), i32(cap_rings, 4), f64(cap_rings)
        pts_xy, pts_src = f64(max(bound, 1), 2), i32(max(bound, 1))
        word = torch.zeros(3, dtype=torch.int64, device=self.device)          # the error word (int32) and total_out [2]
        ws_bytes = int(lib.tgnn_union_contour_workspace_bytes(k, self.n_tiles, bound))
        ws = torch.empty(ws_bytes // 8 + 1, dtype=torch.int64, device=self.device)
        check(lib.tgnn_union_contour(ptr(ring_xy), ptr(ring_ptr), self.n_tiles, ptr(col_ptr), ptr(col_idx), ptr(touch_ptr),
                                     ptr(touch_idx), ptr(alive), k, UNION_TOL, cap_rings, bound, ptr(mask_out), ptr(ring_out),
                                     ptr(ring_area), ptr(pts_xy), ptr(pts_src), ptr(word[1:]), ptr(word), ptr(ws), ws_bytes,
                                     _lib.current_stream(self.device)))
        code, rings, points = (int(v) for v in word.cpu().tolist())
        code &= 0xFFFFFFFF
        if code:
            _raise_device_error("tgnn_union_contour", code, _CONTOUR_ERROR_BITS, only_set=True)
        return UnionContours(ring_xy, ring_ptr, mask_out, ring_out[:rings], ring_area[:rings], pts_xy[:points], pts_src[:points])

    def layouts_in_regions(self, regions, with_area=False):
        """One DeviceLayout per region: the tiles inside it cut out of the complete graph (what `layout` gives for that
        tile set).  Each layout owns its buffers.  with_area: every layout also carries `super_contour_area`, the area of
        the union of its tiles as a Python float (one kernel call and one copy for all regions)."""
        from .algorithms import DeviceLayout
        alive = self.tiles_in_regions(regions)
        areas = self.union_areas(alive).cpu().tolist() if with_area else None
        out = []
        for k in range(alive.shape[0]):
            sub = self._builder.build(alive[k])
            out.append(DeviceLayout(sub.node_feature.clone(), sub.align_edge_index.clone(), sub.align_edge_features.clone(),
                                    sub.collide_edge_index.clone(), sub.inverse_index.clone()))
            if with_area:
                out[-1].super_contour_area = areas[k]
        return out


class UnionContours:
    """What `CompleteGraphOnDevice.union_contours` returns: the five device tensors of tgnn_union_contour, cut to the call's
    totals.  mask [K, 4] int32 = {rings, first ring, points, status}; ring [R, 4] int32 = {first point, points, component,
    +1 exterior / -1 hole}; ring_area [R] float64, signed; pts_xy [P, 2] float64; pts_src [P] int32, the index of each point into
    the graph's ring_xy (`pts_xy` holds exactly those coordinates).  `polygons(k)` reads all of them back once."""

    def __init__(self, ring_xy, ring_ptr, mask, ring, ring_area, pts_xy, pts_src):
        self.ring_xy, self.ring_ptr = ring_xy, ring_ptr
        self.mask, self.ring, self.ring_area, self.pts_xy, self.pts_src = mask, ring, ring_area, pts_xy, pts_src
        self._host = None

    def __len__(self):
        return int(self.mask.shape[0])

    def host(self):
        """(mask, ring, ring_area, pts_xy, pts_src) as numpy arrays, read back on first use."""
        if self._host is None:
            self._host = tuple(t.cpu().numpy() for t in (self.mask, self.ring, self.ring_area, self.pts_xy, self.pts_src))
        return self._host

    def polygons(self, k):
        """The union of mask k as a list of `tiling.region.Region(exterior, holes, validate=False)`, one per connected
        component in ascending component label (the lowest tile of the component), holes in ring order.  A ring that passes a
        pinch point touches itself there, which is why the regions are not validated.  ValueError when the mask's tiles
        collide."""
        from ..tiling.region import Region
        mask, ring, _, pts_xy, _ = self.host()
        rings, first, _, status = (int(v) for v in mask[k])
        if status != 0:
            raise ValueError(f"mask {k}: two alive tiles collide (the union polygon is defined for a solution, whose tiles do "
                             "not overlap)")
        rows = ring[first:first + rings]
        cut = lambda r: pts_xy[r[0]:r[0] + r[1]].copy()
        out = []
        for label in sorted({int(r[2]) for r in rows if r[3] > 0}):
            (ext,) = [r for r in rows if r[2] == label and r[3] > 0]
            out.append(Region(cut(ext), [cut(r) for r in rows if r[2] == label and r[3] < 0], validate=False))
        return out


def graph_on_device(graph: TileGraph, device=None) -> CompleteGraphOnDevice:
    """The CompleteGraphOnDevice of `graph` on `device` (default: the current CUDA device), made once and kept on the graph."""
    import torch
    dev = torch.device(device if device is not None else "cuda")
    if dev.type == "cuda" and dev.index is None:
        dev = torch.device("cuda", torch.cuda.current_device())
    cache = graph.__dict__.setdefault("_on_device", {})
    if dev not in cache:
        cache[dev] = CompleteGraphOnDevice(graph, dev)
    return cache[dev]


def layout_on_device(graph_on_device: CompleteGraphOnDevice, tiles_super_set):
    return graph_on_device.layout(tiles_super_set)


def tree_sweep_call(device, geo, n_nodes, tile_of_node, nbr_ptr, nbr_idx, n_nbr, n_slots, unlabelled, tile_alive, label, chi_cache, k,
                    parent_slot, slot, visit_ptr, visit_node, p, u, n_visit, check_holes, stats, accepted, killed, trace, err, ws=None):
    """`tgnn_tree_sweep_many` on `device`'s current stream.  geo: the eight leading arguments (a graph's rings and contact rows:
    `CompleteGraphOnDevice.tree_sweep_into`), or None for a layout that carries no complete graph -- check_holes == 0 only, no
    tile state."""
    torch, _lib, check, lib, ptr, UNION_TOL = _union_api()
    opt = lambda t: None if t is None else ptr(t)
    if geo is None:
        geo = (None, None, 0, None, None, UNION_TOL, 1.0, 0.0)
    ws_bytes = int(lib.tgnn_tree_sweep_workspace_bytes(k))
    if ws is None:
        ws = torch.empty(max(ws_bytes // 4, 1), dtype=torch.int32, device=device)
    with torch.cuda.device(device):
        check(lib.tgnn_tree_sweep_many(*geo, n_nodes, opt(tile_of_node), ptr(nbr_ptr), ptr(nbr_idx), n_nbr, n_slots, ptr(unlabelled),
                                       opt(tile_alive), opt(label), opt(chi_cache), k, ptr(parent_slot), ptr(slot), ptr(visit_ptr),
                                       ptr(visit_node), ptr(p), ptr(u), n_visit, int(bool(check_holes)), ptr(stats), ptr(accepted),
                                       ptr(killed), ptr(trace), ptr(err), ptr(ws), 4 * int(ws.numel()), _lib.current_stream(device)))
