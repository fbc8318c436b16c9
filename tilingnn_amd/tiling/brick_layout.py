"""`BrickLayout` -- the data side (/root/reference/tiling/brick_layout.py:22-56, :242-286).

A layout is five numpy arrays + the index maps to the complete graph.  The reference's class also draws, unions and
measures polygons through shapely (`show_*`, `get_super_contour_poly`, ...): geometry is outside this package and those
methods are not mirrored -- hand the arrays of this object to the reference's class when they are needed (same constructor
arguments).  Three facts of that geometry are here.  The AREA of the union of the layout's tiles, because every score divides by
it: `compute_super_contour_area` (on the GPU, csrc/union_area.hip) -> `super_contour_area`; there is deliberately no method
called `get_super_contour_poly`.  And whether a solution leaves an enclosed gap, the validity bit the reference asks every
solved layout for: `detect_holes` (:229-240), with `count_holes` and the many-layout `detect_holes_many` (on the GPU,
csrc/union_topology.hip).  And the outline of a solution: `get_selected_tiles_union_polygon` (:223-227) and the many-layout
`union_polygons_many` (on the GPU, csrc/union_contour.hip), as `tiling.region.Region`s instead of a shapely polygon.  And what
adding each further tile would do to the holes of a selection, the question behind the reference's `check_holes` veto
(util/algorithms.py:150-152): `hole_deltas` (on the GPU, csrc/union_hole_delta.hip).  What
`ML_Solver.predict` and the greedy loop read is here:
`get_data_as_torch_tensor` (:242-246) and `compute_sub_layout` (:248-286, vectorised: one membership mask instead of
four comprehensions over every edge).
"""
import copy
from collections import defaultdict

import numpy as np


class BrickLayout:
    def __init__(self, complete_graph, node_feature, collide_edge_index, collide_edge_features, align_edge_index,
                 align_edge_features, re_index, target_polygon=None):
        self.complete_graph = complete_graph
        self.node_feature = node_feature
        self.collide_edge_index = collide_edge_index
        self.collide_edge_features = collide_edge_features
        self.align_edge_index = align_edge_index
        self.align_edge_features = align_edge_features
        self.re_index = re_index                                   # complete-graph tile -> layout node (:37-38)
        self.inverse_index = defaultdict(int)                      # layout node -> complete-graph tile (:40-43)
        for k, v in self.re_index.items():
            self.inverse_index[v] = k
        self.predict = np.zeros(len(self.node_feature))
        self.predict_probs = []
        self.predict_order = []
        self.target_polygon = target_polygon
        self.super_contour_poly = None
        self.super_contour_area = None                             # compute_super_contour_area, or the crop path's coverage=True

    def __deepcopy__(self, memo):                                  # :57-73: arrays shared, predictions copied
        new = type(self).__new__(self.__class__)
        new.__dict__.update(self.__dict__)
        new.predict = copy.deepcopy(self.predict)
        new.predict_probs = copy.deepcopy(self.predict_probs)
        return new

    def is_solved(self):                                           # :75-76
        return len(self.predict) != 0

    def get_data_as_torch_tensor(self, device):
        """:242-246."""
        from ..util.data_util import to_torch_tensor
        return to_torch_tensor(device, self.node_feature, self.align_edge_index, self.align_edge_features,
                               self.collide_edge_index, self.collide_edge_features)

    def compute_super_contour_area(self, device=None):
        """The area of the union of this layout's tiles -- the reference's `get_super_contour_poly().area` (:180-188) --
        computed on the GPU from the complete graph's rings and `re_index` (csrc/union_area.hip), stored in
        `self.super_contour_area` (what `Losses.solution_score` divides by) and returned.  There is no host fallback."""
        import torch
        if not torch.cuda.is_available():
            raise RuntimeError("compute_super_contour_area runs on the GPU (csrc/union_area.hip) and no GPU is available; "
                               "there is no host fallback")
        from ..util.data_util import graph_on_device
        on_device = graph_on_device(self.complete_graph, device)
        tiles = np.fromiter(self.re_index.keys(), dtype=np.int64, count=len(self.re_index))
        if tiles.size and (tiles.min() < 0 or tiles.max() >= on_device.n_tiles):
            raise ValueError(f"re_index names a tile outside [0, {on_device.n_tiles})")
        alive = np.zeros(on_device.n_tiles, dtype=np.int32)
        alive[tiles] = 1
        self.super_contour_area = float(on_device.union_areas(torch.from_numpy(alive).to(on_device.device)).item())
        return self.super_contour_area

    def selected_tiles(self):
        """Complete-graph ids (int64) of the tiles with `predict == 1`, through `inverse_index`."""
        nodes = np.flatnonzero(np.asarray(self.predict) == 1)
        return np.fromiter((self.inverse_index[int(i)] for i in nodes), dtype=np.int64, count=nodes.shape[0])

    def count_holes(self, device=None):
        """(components, holes) of the union of the selected tiles (`predict == 1`): its connected components, tiles that touch
        in a single corner being connected as under the reference's 1e-7 buffer, and the enclosed gaps it leaves.  Computed on
        the GPU (csrc/union_topology.hip); ValueError when two selected tiles collide (a solution never does).  There is no host
        fallback."""
        return detect_holes_many([self], device)[0]

    def detect_holes(self, device=None):
        """True when the selected tiles enclose a gap -- the reference's `detect_holes` (:229-240)."""
        return self.count_holes(device)[1] > 0

    def hole_deltas(self, selection=None, device=None):
        """(dcomponents, dholes, state), int32 arrays with one entry per node of this layout: what adding the node's tile to
        `selection` (one 0/1 entry per node; default `predict`) would do to `count_holes()` of it, where state is 0 (the tile
        may be added); state 1: the node is selected, 2: its tile collides with a selected one -- both deltas 0 there.  The
        reference's hole veto (util/algorithms.py:150-152) refuses the nodes with dholes > 0; the ones with dholes < 0 plug
        a gap.  Tiles of the complete graph outside the layout are not reported.  Computed on the GPU
        (csrc/union_hole_delta.hip); ValueError when two selected tiles collide.  There is no host fallback."""
        import torch
        if not torch.cuda.is_available():
            raise RuntimeError("hole_deltas runs on the GPU (csrc/union_hole_delta.hip) and no GPU is available; "
                               "there is no host fallback")
        from ..util.data_util import graph_on_device
        on_device = graph_on_device(self.complete_graph, device)
        n = len(self.node_feature)
        chosen = np.asarray(self.predict if selection is None else selection).reshape(-1)
        if chosen.shape[0] != n:
            raise ValueError(f"selection must have one entry per node ({n}), got {chosen.shape[0]}")
        tiles = np.fromiter((self.inverse_index[i] for i in range(n)), dtype=np.int64, count=n)
        if n and (tiles.min() < 0 or tiles.max() >= on_device.n_tiles):
            raise ValueError(f"inverse_index names a tile outside [0, {on_device.n_tiles})")
        alive = np.zeros(on_device.n_tiles, dtype=np.int32)
        alive[tiles[chosen == 1]] = 1
        delta, state = on_device.hole_deltas(torch.from_numpy(alive).to(on_device.device))
        both = torch.cat([delta[0], state[0][:, None]], dim=1).cpu().numpy()[tiles]       # one read-back
        if n and (both[:, 2] == 3).any():
            raise ValueError("two selected tiles collide (hole_deltas is defined for a selection whose tiles do not overlap)")
        return both[:, 0].copy(), both[:, 1].copy(), both[:, 2].copy()

    def get_selected_tiles_union_polygon(self, device=None):
        """The outline of the union of the selected tiles (`predict == 1`) -- the reference's method of this name (:223-227) --
        as a list of `tiling.region.Region`, one per connected component (tiles that touch in a single corner are connected,
        where shapely's unbuffered union would return them apart), exterior counter-clockwise, holes clockwise, every point a
        vertex of a selected tile.  Computed on the GPU (csrc/union_contour.hip); ValueError when two selected tiles collide.
        There is no host fallback."""
        return union_polygons_many([self], device)[0]

    def compute_sub_layout(self, predict):
        """:248-286.  `predict`: a SelectionSolution-like object with dicts `labelled_nodes` / `unlabelled_nodes`."""
        assert len(self.node_feature) == len(predict.labelled_nodes) + len(predict.unlabelled_nodes)
        sorted_items = sorted(predict.unlabelled_nodes.items(), key=lambda kv: kv[0])         # :250-252
        predict.unlabelled_nodes.clear()
        predict.unlabelled_nodes.update(sorted_items)
        keep = np.fromiter(predict.unlabelled_nodes.keys(), dtype=np.int64, count=len(sorted_items))
        n = len(self.node_feature)
        new_id = np.full(n, -1, dtype=np.int64)
        new_id[keep] = np.arange(keep.shape[0])

        def cut(index, feats):
            index, feats = np.asarray(index), np.asarray(feats)
            if index.shape[0] == 0:                                # the reference's `else np.array([])` branches
                return np.array([]), np.array([])
            a, b = new_id[index[0]], new_id[index[1]]
            alive = (a >= 0) & (b >= 0)
            if not alive.any():
                return np.array([]), np.array([])                 # np.array([]).T / np.array([]) of empty lists
            return np.stack([a[alive], b[alive]]), feats[alive]

        col, colf = cut(self.collide_edge_index, self.collide_edge_features)
        adj, adjf = cut(self.align_edge_index, self.align_edge_features)
        node_inverse_index = {i: int(k) for i, k in enumerate(keep)}                          # :276-278
        fixed_re_index = {self.inverse_index[int(k)]: i for i, k in enumerate(keep)}         # :280-282
        return BrickLayout(self.complete_graph, self.node_feature[keep], col, colf, adj, adjf, fixed_re_index,
                           target_polygon=self.target_polygon), node_inverse_index

    @staticmethod
    def assert_equal_layout(a, b):                                 # :288-300
        for name in ("node_feature", "collide_edge_index", "collide_edge_features", "align_edge_index",
                     "align_edge_features"):
            assert np.array_equal(getattr(a, name), getattr(b, name)), name
        assert dict(a.re_index) == dict(b.re_index)


def _selection_masks(layouts, what, device):
    """(on_device, alive [K, n_tiles] int32 on the host) of K solved layouts of ONE complete graph: the mask construction
    `detect_holes_many` and `union_polygons_many` share."""
    graph = layouts[0].complete_graph
    if any(l.complete_graph is not graph for l in layouts):
        raise ValueError(f"{what} takes layouts of one complete graph")
    from ..util.data_util import graph_on_device
    on_device = graph_on_device(graph, device)
    alive = np.zeros((len(layouts), on_device.n_tiles), dtype=np.int32)
    for k, layout in enumerate(layouts):
        tiles = layout.selected_tiles()
        if tiles.size and (tiles.min() < 0 or tiles.max() >= on_device.n_tiles):
            raise ValueError(f"layout {k}: inverse_index names a tile outside [0, {on_device.n_tiles})")
        alive[k, tiles] = 1
    return on_device, alive


def union_polygons_many(layouts, device=None):
    """[`BrickLayout.get_selected_tiles_union_polygon` of each] for K solved layouts of ONE complete graph, with one kernel call
    and one read-back of the rings for all of them (csrc/union_contour.hip).  ValueError when a layout's selected tiles
    collide; RuntimeError without a GPU: there is no host fallback."""
    import torch
    if not torch.cuda.is_available():
        raise RuntimeError("get_selected_tiles_union_polygon runs on the GPU (csrc/union_contour.hip) and no GPU is available; "
                           "there is no host fallback")
    layouts = list(layouts)
    if not layouts:
        return []
    on_device, alive = _selection_masks(layouts, "union_polygons_many", device)
    contours = on_device.union_contours(torch.from_numpy(alive).to(on_device.device))
    bad = np.flatnonzero(contours.host()[0][:, 3] != 0)
    if bad.size:
        raise ValueError(f"layout {int(bad[0])}: two selected tiles collide (the union polygon is defined for a solution, whose "
                         f"tiles do not overlap); {bad.size} of {len(layouts)} layouts do")
    return [contours.polygons(k) for k in range(len(layouts))]


def detect_holes_many(layouts, device=None):
    """[(components, holes)] of K solved layouts of ONE complete graph -- `BrickLayout.count_holes` of each -- with one kernel
    call and one read-back for all of them (csrc/union_topology.hip).  ValueError when a layout's selected tiles collide;
    RuntimeError without a GPU: there is no host fallback."""
    import torch
    if not torch.cuda.is_available():
        raise RuntimeError("detect_holes runs on the GPU (csrc/union_topology.hip) and no GPU is available; "
                           "there is no host fallback")
    layouts = list(layouts)
    if not layouts:
        return []
    on_device, alive = _selection_masks(layouts, "detect_holes_many", device)
    out = on_device.union_topology(torch.from_numpy(alive).to(on_device.device)).cpu().numpy()
    bad = np.flatnonzero(out[:, 2] != 0)
    if bad.size:
        raise ValueError(f"layout {int(bad[0])}: two selected tiles collide (detect_holes is defined for a solution, whose "
                         f"tiles do not overlap); {bad.size} of {len(layouts)} layouts do")
    return [(int(c), int(h)) for c, h, _ in out]
