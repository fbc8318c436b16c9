"""Target shapes -> layouts (the reference's tiling/tile_factory.py), with the tile-in-region predicate on the GPU.

Same function names and argument meanings as the reference's module.  What changed is where the predicate runs: the
reference asks shapely, one intersection per (region, tile) pair (`contain`, util/algo_util.py:143-144); here every
call goes to `CompleteGraphOnDevice.tiles_in_regions` (csrc/region.hip), all regions of a call in one launch.  The target
polygon is a `Region` (tiling/region.py).  There is no host fallback: without a GPU these functions raise.

Random shapes.  `generatePolygon` and `generate_random_inputs` draw from a `random.Random` instance (default: the global
`random` module) in the reference's order -- uniform(low, high), random(), random(), randint(3, max_vertices), then n x
uniform, uniform(0, 2 pi), n x gauss -- with the same arithmetic, so the same stream state gives the same vertices.
A star whose clipped radii reach 0 at two non-adjacent vertices touches itself at its centre.  Such a ring is not a valid
GEOS polygon, and the reference's intersection may raise on it, in which case its `try` draws again; here the winding
number still defines the set the reference means and the candidate is kept.  The test suite counts how often this happens.

The coverage score of `crop_multiple_layouts_from_contour` (the area of the union of the cropped tiles over the target's) is
opt-in, `coverage=True` (csrc/union_area.hip); by default None is returned in its place.
Not mirrored: `compute_super_graph` (the union polygon itself), plotting, SVG input.
"""
from __future__ import annotations

import itertools
import math
import random as _random

import numpy as np

from .region import Region

EPS = 1e-5


def _device_graph(graph, device=None):
    from ..util.data_util import graph_on_device
    return graph_on_device(graph, device)


def get_graph_bound(graph):
    """(x_min, x_max, y_min, y_max) over every vertex of every tile."""
    pts = np.concatenate([np.asarray(t.tile_poly.exterior) for t in graph.tiles])
    return float(np.min(pts[:, 0])), float(np.max(pts[:, 0])), float(np.min(pts[:, 1])), float(np.max(pts[:, 1]))


def clip(x, min, max):
    """x limited to [min, max]; unchanged when the interval is empty."""
    if min > max:
        return x
    if x < min:
        return min
    if x > max:
        return max
    return x


def generatePolygon(ctrX, ctrY, aveRadius, irregularity, spikeyness, numVerts, rng=None):
    """A random star around (ctrX, ctrY): numVerts vertices, counter-clockwise, as a list of (x, y).  The angular steps
    vary by up to irregularity * 2 pi / numVerts and are rescaled to sum to 2 pi; the radii are normal around aveRadius
    with deviation spikeyness * aveRadius, limited to [0, 2 aveRadius]."""
    rng = _random if rng is None else rng
    two_pi = 2 * math.pi
    irregularity = clip(irregularity, 0, 1) * two_pi / numVerts
    spikeyness = clip(spikeyness, 0, 1) * aveRadius
    step = two_pi / numVerts
    steps = [rng.uniform(step - irregularity, step + irregularity) for _ in range(numVerts)]
    total = 0
    for s in steps:
        total = total + s
    scale = total / two_pi
    steps = [s / scale for s in steps]
    angle = rng.uniform(0, two_pi)
    points = []
    for s in steps:
        radius = clip(rng.gauss(aveRadius, spikeyness), 0, 2 * aveRadius)
        points.append((ctrX + radius * math.cos(angle), ctrY + radius * math.sin(angle)))
        angle = angle + s
    return points


def draw_random_polygon(bound, max_vertices=10, low=0.2, high=0.7, rng=None):
    """The draw of one attempt of `generate_random_inputs` for a graph with bound (x_min, x_max, y_min, y_max)."""
    rng = _random if rng is None else rng
    x_min, x_max, y_min, y_max = bound
    base_radius = min(x_max - x_min, y_max - y_min) / 2
    radius_ratio = rng.uniform(low, high)
    irregularity = rng.random()
    spikeyness = rng.random()
    n = rng.randint(3, max_vertices)
    return generatePolygon((x_max + x_min) / 2, (y_max + y_min) / 2, base_radius * radius_ratio, irregularity, spikeyness, n,
                           rng=rng)


def get_all_placement_in_polygon(graph, polygon: Region, device=None):
    """(tiles inside the polygon in ascending order, collision edges, adjacency edges among them) -- the edges as lists of
    (u, v) pairs in the graph's edge order."""
    alive = _device_graph(graph, device).tiles_in_regions([polygon])[0].cpu().numpy()
    tiles_super_set = np.flatnonzero(alive).tolist()
    from ..util.data_util import filter_edges
    a = graph.arrays
    col_rows, adj_rows = filter_edges(graph, tiles_super_set)
    return (tiles_super_set, [tuple(int(v) for v in e) for e in a.colli_edges[:, col_rows].T],
            [tuple(int(v) for v in e) for e in a.adj_edges[:, adj_rows].T])


def create_brick_layout_from_polygon(graph, polygon: Region, device=None):
    """node_feature, collide_edge_index, collide_edge_features, align_edge_index, align_edge_features, re_index of the tiles
    inside `polygon`."""
    from ..util.data_util import create_brick_layout_from_super_set
    alive = _device_graph(graph, device).tiles_in_regions([polygon])[0].cpu().numpy()
    return create_brick_layout_from_super_set(graph, np.flatnonzero(alive).tolist())


def generate_random_inputs(graph, max_vertices: float = 10, low=0.2, high=0.7, plotter=None, debugger=None, plot_shape=False,
                           rng=None, device=None):
    """A layout cut out of the graph by a random star; attempts whose crop has no collision or no adjacency edge are
    drawn again from the stream."""
    rng = _random if rng is None else rng
    bound = get_graph_bound(graph)
    while True:
        vertices = draw_random_polygon(bound, max_vertices, low, high, rng)
        out = create_brick_layout_from_polygon(graph, Region(vertices, validate=False), device)
        if len(out[1]) == 0 or len(out[3]) == 0:
            continue
        return out


def get_tile_movement_delta(complete_graph, movement_delta_ratio):
    """The offsets: ratios times the smaller side of the first tile's box."""
    ring = np.asarray(complete_graph.tiles[0].tile_poly.exterior)
    w = ring[:, 0].max() - ring[:, 0].min()
    h = ring[:, 1].max() - ring[:, 1].min()
    return np.array(movement_delta_ratio) * min(w, h)


def shape_transform(complete_graph, exterior_contour, interior_contours, margin_padding_ratio, rotate_angle, x_delta, y_delta):
    """(base diameter of the graph, the silhouette scaled so that its longer box side is margin_padding_ratio times the
    graph's shorter side, rotated by rotate_angle degrees about its centroid, its centroid placed at the graph centre plus
    (x_delta, y_delta)).  The reference's final buffer(0) is not applied (see tiling/region.py)."""
    b = Region(exterior_contour, interior_contours, validate=False).bounds
    max_axis = max(b[2] - b[0], b[3] - b[1])
    x_min, x_max, y_min, y_max = get_graph_bound(complete_graph)
    graph_center = (x_max + x_min) / 2, (y_max + y_min) / 2
    base_diameter = min(x_max - x_min, y_max - y_min)
    factor = base_diameter * margin_padding_ratio
    ext = np.asarray(exterior_contour) / max_axis * factor
    holes = [np.asarray(h) / max_axis * factor for h in interior_contours]
    region = Region(ext, holes, validate=False)
    cx, cy = region.centroid
    region = region.translate(-cx, -cy).rotate(rotate_angle, origin="centroid")
    return base_diameter, region.translate(graph_center[0] + x_delta, graph_center[1] + y_delta)


def crop_variants(exterior_contour, interior_contours, complete_graph, start_angle=0.0, end_angle=60.0, num_of_angle=1,
                  movement_delta_ratio=(0,), margin_padding_ratios=(0.2,)):
    """The target regions of crop_multiple_layouts_from_contour, in its loop order (margin, angle, x offset, y offset)."""
    deltas = get_tile_movement_delta(complete_graph, list(movement_delta_ratio))
    out = []
    for margin in margin_padding_ratios:
        for angle in np.linspace(start_angle, end_angle, num_of_angle):
            for dx, dy in itertools.product(deltas, deltas):
                out.append(shape_transform(complete_graph, exterior_contour, interior_contours, margin, angle, dx, dy)[1])
    return out


def crop_multiple_layouts_from_contour(exterior_contour, interior_contours, complete_graph, start_angle=0.0, end_angle=60.0,
                                       num_of_angle=1, movement_delta_ratio=[0], margin_padding_ratios=[0.2], device=None,
                                       coverage=False):
    """[(BrickLayout, coverage)] for every margin x angle x offset variant whose crop holds a tile; every variant is
    evaluated in one kernel launch.  coverage=True: the second member is the reference's (tile_factory.py:197), the area of
    the union of the cropped tiles over the target's area (csrc/union_area.hip, all variants in one call), and the layout's
    `super_contour_area` is set, so that `ML_Solver.solve` scores it.  The default leaves both None."""
    from .brick_layout import BrickLayout
    from ..util.data_util import create_brick_layout_from_super_set
    regions = crop_variants(exterior_contour, interior_contours, complete_graph, start_angle, end_angle, num_of_angle,
                            movement_delta_ratio, margin_padding_ratios)
    on_device = _device_graph(complete_graph, device)
    alive_dev = on_device.tiles_in_regions(regions)
    areas = on_device.union_areas(alive_dev).cpu().tolist() if coverage else [None] * len(regions)
    alive = alive_dev.cpu().numpy()
    result = []
    for region, row, area in zip(regions, alive, areas):
        tiles = np.flatnonzero(row).tolist()
        if not tiles:
            continue
        node_feature, col, colf, adj, adjf, re_index = create_brick_layout_from_super_set(complete_graph, tiles)
        layout = BrickLayout(complete_graph, node_feature, col, colf, adj, adjf, re_index, target_polygon=region)
        layout.predict_probs = [0.5 for _ in range(node_feature.shape[0])]
        if coverage:
            layout.super_contour_area = area
        result.append((layout, area / region.area if coverage else None))
    return result
