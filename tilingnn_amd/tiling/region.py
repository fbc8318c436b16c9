"""`Region` -- a shapely-free stand-in for the target `Polygon` the reference crops layouts with
(tiling/tile_factory.py: shape_transform, generate_random_inputs; util/algo_util.py:143-144 `contain`).

A region is one exterior ring and any number of holes, float64 [n, 2] arrays.  It answers what the reference asks of its
target polygon on the cropping path: `area`, `bounds`, `centroid` (the area-weighted one of a polygon with holes, which
`shape_transform` centres on), translation and rotation about a point, and it packs itself into the ring buffers the
device predicate takes (csrc/region.hip: `tgnn_tiles_in_region`), with the orientation normalised there: exterior
counter-clockwise, holes clockwise, so input in either orientation gives the same answer.

Not mirrored: shapely's `buffer(0)` repair, which `shape_transform` applies to its result.  A loaded ring that intersects
itself raises ValueError here instead of being repaired (`validate=False` skips the check; the random stars of
`generatePolygon` are built that way, see tile_factory.py).  Which tiles lie inside follows the winding number, which for a
valid polygon is the polygon itself.
"""
from __future__ import annotations

import math

import numpy as np


def _open_ring(ring) -> np.ndarray:
    r = np.array(ring, dtype=np.float64).reshape(-1, 2)
    if r.shape[0] > 1 and r[0, 0] == r[-1, 0] and r[0, 1] == r[-1, 1]:
        r = r[:-1]
    return r


def signed_area(ring: np.ndarray) -> float:
    """Shoelace area of an open ring, > 0 when counter-clockwise."""
    if ring.shape[0] < 3:
        return 0.0
    x, y = ring[:, 0], ring[:, 1]
    x0 = x[0]
    return float(np.sum((x - x0) * (np.roll(y, -1) - np.roll(y, 1)))) / 2.0


def _ring_moments(ring: np.ndarray):
    """(signed area, integral of x, integral of y) of an open ring, relative to its first vertex."""
    if ring.shape[0] < 3:
        return 0.0, 0.0, 0.0
    b = ring[0]
    p = ring - b
    q = np.roll(p, -1, axis=0)
    c = p[:, 0] * q[:, 1] - q[:, 0] * p[:, 1]
    a = float(np.sum(c)) / 2.0
    mx = float(np.sum((p[:, 0] + q[:, 0]) * c)) / 6.0 + a * b[0]
    my = float(np.sum((p[:, 1] + q[:, 1]) * c)) / 6.0 + a * b[1]
    return a, mx, my


def ring_self_intersects(ring: np.ndarray) -> bool:
    """True when two edges of the open ring meet anywhere but at the vertex two consecutive edges share."""
    n = ring.shape[0]
    if n < 4:
        return False
    p, q = ring, np.roll(ring, -1, axis=0)

    def orient(a, b, c):
        return np.sign((b[..., 0] - a[..., 0]) * (c[..., 1] - a[..., 1]) - (b[..., 1] - a[..., 1]) * (c[..., 0] - a[..., 0]))

    def on_seg(a, b, c):      # c collinear with a-b: within its box
        return (np.minimum(a[..., 0], b[..., 0]) <= c[..., 0]) & (c[..., 0] <= np.maximum(a[..., 0], b[..., 0])) & \
               (np.minimum(a[..., 1], b[..., 1]) <= c[..., 1]) & (c[..., 1] <= np.maximum(a[..., 1], b[..., 1]))

    for i in range(n):
        j = np.arange(i + 2, n)
        if i == 0:
            j = j[j != n - 1]                # edge n-1 shares vertex 0 with edge 0
        if j.size == 0:
            continue
        a, b = p[i][None, :], q[i][None, :]
        c, d = p[j], q[j]
        o1, o2, o3, o4 = orient(a, b, c), orient(a, b, d), orient(c, d, a), orient(c, d, b)
        hit = (o1 != o2) & (o3 != o4) & (o1 != 0) & (o2 != 0) & (o3 != 0) & (o4 != 0)
        hit |= (o1 == 0) & on_seg(a, b, c)
        hit |= (o2 == 0) & on_seg(a, b, d)
        hit |= (o3 == 0) & on_seg(c, d, a)
        hit |= (o4 == 0) & on_seg(c, d, b)
        if hit.any():
            return True
    return False


class Region:
    """exterior: [n, 2]; interiors: list of [m, 2] (closed or open rings, either orientation)."""

    def __init__(self, exterior, interiors=(), validate: bool = True):
        self.exterior = _open_ring(exterior)
        self.interiors = [_open_ring(h) for h in interiors]
        if validate:
            for k, r in enumerate([self.exterior] + self.interiors):
                if ring_self_intersects(r):
                    raise ValueError(f"ring {k} of the region intersects itself (shapely's buffer(0) repair is not mirrored)")

    # ------------------------------------------------------------------ what the reference asks of its Polygon
    @property
    def area(self) -> float:
        return abs(signed_area(self.exterior)) - sum(abs(signed_area(h)) for h in self.interiors)

    @property
    def bounds(self):
        """(minx, miny, maxx, maxy) -- of the exterior, as shapely's."""
        if self.exterior.shape[0] == 0:
            return (math.nan,) * 4
        lo, hi = self.exterior.min(axis=0), self.exterior.max(axis=0)
        return float(lo[0]), float(lo[1]), float(hi[0]), float(hi[1])

    @property
    def centroid(self):
        """Area-weighted centroid (x, y): the exterior's moments minus the holes'."""
        a, mx, my = 0.0, 0.0, 0.0
        for k, r in enumerate([self.exterior] + self.interiors):
            ra, rx, ry = _ring_moments(r)
            s = 1.0 if (k == 0) == (ra >= 0) else -1.0          # exterior counts positive, holes negative
            a, mx, my = a + s * ra, mx + s * rx, my + s * ry
        if a == 0.0:
            c = self.exterior.mean(axis=0)
            return float(c[0]), float(c[1])
        return mx / a, my / a

    def translate(self, xoff=0.0, yoff=0.0) -> "Region":
        d = np.array([xoff, yoff], dtype=np.float64)
        return self._new(self.exterior + d, [h + d for h in self.interiors])

    def rotate(self, angle, origin="centroid", use_radians=False) -> "Region":
        """Counter-clockwise by `angle` (degrees unless use_radians) about `origin` ("centroid", "center" = box centre, or (x, y))."""
        if isinstance(origin, str):
            if origin == "centroid":
                origin = self.centroid
            elif origin == "center":
                b = self.bounds
                origin = ((b[0] + b[2]) / 2.0, (b[1] + b[3]) / 2.0)
            else:
                raise ValueError(f"origin {origin!r}")
        t = angle if use_radians else angle * math.pi / 180.0
        c, s = math.cos(t), math.sin(t)
        x0, y0 = float(origin[0]), float(origin[1])

        def rot(r):
            x, y = r[:, 0] - x0, r[:, 1] - y0
            return np.stack([x0 + c * x - s * y, y0 + s * x + c * y], axis=1)
        return self._new(rot(self.exterior), [rot(h) for h in self.interiors])

    def _new(self, ext, holes) -> "Region":
        out = Region.__new__(Region)
        out.exterior, out.interiors = ext, holes
        return out

    # ------------------------------------------------------------------ device buffers
    def rings(self):
        """The rings with the orientation normalised: exterior counter-clockwise, holes clockwise."""
        ext = self.exterior if signed_area(self.exterior) >= 0 else self.exterior[::-1]
        holes = [h if signed_area(h) <= 0 else h[::-1] for h in self.interiors]
        return [np.ascontiguousarray(ext)] + [np.ascontiguousarray(h) for h in holes]


def pack_regions(regions):
    """Flattened ring buffers of tgnn_tiles_in_region: ring_xy [P, 2] f64, ring_ptr [R + 1] i32, region_ring_ptr [K + 1] i32,
    region_bbox [K, 4] f64 (over all rings), and the largest vertex count of a region."""
    rings, region_ring_ptr, bbox, max_edges = [], [0], [], 0
    for reg in regions:
        rs = reg.rings()
        rings.extend(rs)
        region_ring_ptr.append(len(rings))
        pts = np.concatenate(rs) if sum(r.shape[0] for r in rs) else np.zeros((0, 2))
        if pts.shape[0]:
            lo, hi = pts.min(axis=0), pts.max(axis=0)
            bbox.append([lo[0], lo[1], hi[0], hi[1]])
        else:                                   # an empty region: a box no tile meets
            bbox.append([math.inf, math.inf, -math.inf, -math.inf])
        max_edges = max(max_edges, int(pts.shape[0]))
    sizes = np.array([r.shape[0] for r in rings], dtype=np.int64)
    ring_ptr = np.zeros(len(rings) + 1, dtype=np.int64)
    ring_ptr[1:] = np.cumsum(sizes)
    if ring_ptr[-1] >= 2 ** 31 or len(rings) >= 2 ** 31:
        raise ValueError("too many region vertices for one call")
    ring_xy = np.concatenate(rings) if ring_ptr[-1] else np.zeros((0, 2))
    return (np.ascontiguousarray(ring_xy, dtype=np.float64), ring_ptr.astype(np.int32),
            np.asarray(region_ring_ptr, dtype=np.int32), np.asarray(bbox, dtype=np.float64).reshape(-1, 4), max_edges)


# ---------------------------------------------------------------------------------------------- tiles
def _is_convex_vertex(a, b, c) -> bool:
    return (b[0] - a[0]) * (c[1] - a[1]) - (b[1] - a[1]) * (c[0] - a[0]) > 0.0


def _in_triangle(p, a, b, c) -> bool:
    d1 = (b[0] - a[0]) * (p[1] - a[1]) - (b[1] - a[1]) * (p[0] - a[0])
    d2 = (c[0] - b[0]) * (p[1] - b[1]) - (c[1] - b[1]) * (p[0] - b[0])
    d3 = (a[0] - c[0]) * (p[1] - c[1]) - (a[1] - c[1]) * (p[0] - c[0])
    return d1 >= 0 and d2 >= 0 and d3 >= 0


def ear_clip(ring) -> np.ndarray:
    """Counter-clockwise triangles [t, 3, 2] of a simple ring (either orientation; closed or open), by ear clipping."""
    r = _open_ring(ring)
    if signed_area(r) < 0:
        r = r[::-1]
    idx = list(range(r.shape[0]))
    tris = []
    while len(idx) > 3:
        m = len(idx)
        for k in range(m):
            i0, i1, i2 = idx[k - 1], idx[k], idx[(k + 1) % m]
            a, b, c = r[i0], r[i1], r[i2]
            if not _is_convex_vertex(a, b, c):
                continue
            if any(_in_triangle(r[j], a, b, c) for j in idx if j not in (i0, i1, i2)):
                continue
            tris.append((a, b, c))
            del idx[k]
            break
        else:
            raise ValueError("ear clipping found no ear: the ring is not simple")
    if len(idx) == 3:
        tris.append((r[idx[0]], r[idx[1]], r[idx[2]]))
    return np.asarray(tris, dtype=np.float64).reshape(-1, 3, 2)


def tile_geometry(rings, areas):
    """Device-side tile description of tgnn_tiles_in_region from tile rings and their areas: tri_xy [T, 3, 2],
    tile_tri_ptr [n + 1] i32, tile_bbox [n, 4], tile_area [n], tile_point [n, 2] (the centroid of the tile's first triangle)."""
    tris, ptr, bbox, point = [], [0], [], []
    for r in rings:
        t = ear_clip(r)
        if t.shape[0] == 0:
            raise ValueError("a tile ring with fewer than three vertices")
        tris.append(t)
        ptr.append(ptr[-1] + t.shape[0])
        rr = _open_ring(r)
        lo, hi = rr.min(axis=0), rr.max(axis=0)
        bbox.append([lo[0], lo[1], hi[0], hi[1]])
        point.append(t[0].mean(axis=0))
    return (np.ascontiguousarray(np.concatenate(tris)), np.asarray(ptr, dtype=np.int32), np.asarray(bbox, dtype=np.float64),
            np.ascontiguousarray(areas, dtype=np.float64), np.asarray(point, dtype=np.float64))


# ---------------------------------------------------------------------------------------------- union of tiles
UNION_TOL = 1e-6          # the radius the reference buffers every tile by before its union (brick_layout.py:185)


def union_geometry(rings, colli_edges, n_tiles=None):
    """Device-side description of tgnn_union_area (csrc/union_area.hip): ring_xy [P, 2] f64 with every ring open and
    counter-clockwise (the graphs store them clockwise), ring_ptr [n + 1] i32, and the collision edges [2, E] (either or
    both directions) as a symmetric CSR without self loops or duplicates: col_ptr [n + 1] i32, col_idx i32."""
    out = []
    for r in rings:
        r = _open_ring(r)
        if r.shape[0] < 3:
            raise ValueError("a tile ring with fewer than three vertices")
        out.append(np.ascontiguousarray(r if signed_area(r) >= 0 else r[::-1]))
    n = len(out) if n_tiles is None else int(n_tiles)
    if n != len(out):
        raise ValueError(f"{len(out)} rings for {n} tiles")
    ring_ptr = np.zeros(n + 1, dtype=np.int64)
    ring_ptr[1:] = np.cumsum([r.shape[0] for r in out])
    col = np.asarray(colli_edges, dtype=np.int64).reshape(2, -1)
    if col.size and (col.min() < 0 or col.max() >= n):
        raise ValueError(f"collision edge end outside [0, {n})")
    both = np.concatenate([col, col[::-1]], axis=1)
    both = both[:, both[0] != both[1]]
    keys = np.unique(both[0] * n + both[1])
    col_ptr = np.searchsorted(keys // max(n, 1), np.arange(n + 1))
    if ring_ptr[-1] >= 2 ** 31 or keys.size >= 2 ** 31:
        raise ValueError("too many tile vertices or collision edges for one call")
    return (np.ascontiguousarray(np.concatenate(out) if out else np.zeros((0, 2)), dtype=np.float64), ring_ptr.astype(np.int32),
            col_ptr.astype(np.int32), (keys % max(n, 1)).astype(np.int32))


def _point_segment_distances(pts, a, b):
    """[..., V, S] distances of the points pts [..., V, 2] to the segments a -> b [..., S, 2]."""
    d = b - a
    rel = pts[..., :, None, :] - a[..., None, :, :]
    dd = np.maximum(np.sum(d * d, axis=-1), 1e-300)[..., None, :]
    t = np.clip(np.sum(rel * d[..., None, :, :], axis=-1) / dd, 0.0, 1.0)
    gap = rel - t[..., None] * d[..., None, :, :]
    return np.hypot(gap[..., 0], gap[..., 1])


def vertex_side_distances(ring_xy, ring_ptr, pairs):
    """Every distance from a vertex of tile v to a side of tile u, for the pairs [2, E] = (u, v); one flat array.  Pairs are
    grouped by the two rings' vertex counts, so the work is a few array operations whatever the tile shapes are."""
    pairs = np.asarray(pairs, dtype=np.int64).reshape(2, -1)
    if pairs.shape[1] == 0:
        return np.zeros(0)
    size = np.diff(ring_ptr).astype(np.int64)
    out = []
    shape_key = size[pairs[0]] * (int(size.max()) + 1) + size[pairs[1]]
    for key in np.unique(shape_key):
        u, v = pairs[:, shape_key == key]
        nu, nv = int(size[u[0]]), int(size[v[0]])
        a = ring_xy[ring_ptr[u][:, None] + np.arange(nu)[None, :]]
        b = ring_xy[ring_ptr[u][:, None] + (np.arange(nu)[None, :] + 1) % nu]
        p = ring_xy[ring_ptr[v][:, None] + np.arange(nv)[None, :]]
        out.append(_point_segment_distances(p, a, b).reshape(-1))
    return np.concatenate(out)


def _pair_gaps(ring_xy, ring_ptr, u, v):
    """Per pair (u[k], v[k]): the smallest distance from a vertex of tile v[k] to a side of tile u[k]."""
    out = np.full(u.shape[0], np.inf)
    if u.shape[0] == 0:
        return out
    size = np.diff(ring_ptr).astype(np.int64)
    shape_key = size[u] * (int(size.max()) + 1) + size[v]
    for key in np.unique(shape_key):
        sel = np.flatnonzero(shape_key == key)
        uu, vv = u[sel], v[sel]
        nu, nv = int(size[uu[0]]), int(size[vv[0]])
        for s in range(0, sel.shape[0], 1 << 16):               # bounded temporaries whatever the graph's size
            us, vs = uu[s:s + (1 << 16)], vv[s:s + (1 << 16)]
            a = ring_xy[ring_ptr[us][:, None] + np.arange(nu)[None, :]]
            b = ring_xy[ring_ptr[us][:, None] + (np.arange(nu)[None, :] + 1) % nu]
            p = ring_xy[ring_ptr[vs][:, None] + np.arange(nv)[None, :]]
            out[sel[s:s + (1 << 16)]] = _point_segment_distances(p, a, b).reshape(us.shape[0], -1).min(axis=1)
    return out


def contact_geometry(ring_xy, ring_ptr, tol=UNION_TOL):
    """The contact relation of tgnn_union_topology (csrc/union_topology.hip) as a CSR: touch_ptr [n + 1] i32, touch_idx i32, row
    i = the tiles j != i with a vertex of one within `tol` of the closed ring of the other; symmetric, rows sorted.  For tiles
    that do not overlap this is every pair that shares a point: an isolated shared point is a vertex of one of the two, and a
    shared stretch ends in vertices.  It is NOT the union of the graph's two edge lists (on ring 9 most of its pairs, the
    corner-to-corner contacts, are in neither).  `ring_xy`, `ring_ptr`: what `union_geometry` returns.  Pairs whose boxes,
    grown by tol, do not meet are never measured."""
    ring_xy = np.asarray(ring_xy, dtype=np.float64).reshape(-1, 2)
    ring_ptr = np.asarray(ring_ptr, dtype=np.int64)
    n = ring_ptr.shape[0] - 1
    if n <= 0:
        return np.zeros(max(n, 0) + 1, dtype=np.int32), np.zeros(0, dtype=np.int32)
    if np.any(np.diff(ring_ptr) < 3):
        raise ValueError("a tile ring with fewer than three vertices")
    starts = ring_ptr[:-1]
    lo = np.stack([np.minimum.reduceat(ring_xy[:, 0], starts), np.minimum.reduceat(ring_xy[:, 1], starts)], axis=1) - tol
    hi = np.stack([np.maximum.reduceat(ring_xy[:, 0], starts), np.maximum.reduceat(ring_xy[:, 1], starts)], axis=1) + tol
    us, vs = [], []
    for s in range(0, n, 1024):                                     # box prefilter, a block of rows at a time
        e = min(s + 1024, n)
        near = ((lo[s:e, None, 0] <= hi[None, :, 0]) & (hi[s:e, None, 0] >= lo[None, :, 0]) &
                (lo[s:e, None, 1] <= hi[None, :, 1]) & (hi[s:e, None, 1] >= lo[None, :, 1]))
        i, j = np.nonzero(near)
        i = i + s
        keep = i < j
        us.append(i[keep])
        vs.append(j[keep])
    u, v = np.concatenate(us).astype(np.int64), np.concatenate(vs).astype(np.int64)
    gap = np.minimum(_pair_gaps(ring_xy, ring_ptr, u, v), _pair_gaps(ring_xy, ring_ptr, v, u))
    u, v = u[gap <= tol], v[gap <= tol]
    keys = np.unique(np.concatenate([u * n + v, v * n + u]))
    if keys.size >= 2 ** 31:
        raise ValueError("too many contact pairs for one call")
    touch_ptr = np.searchsorted(keys // n, np.arange(n + 1))
    return touch_ptr.astype(np.int32), (keys % n).astype(np.int32)


CONTOUR_MAX_SPLITS = 8    # foreign vertex positions tgnn_union_contour keeps inside one tile side (union_contour_piece.h: kMaxSplits)
CONTOUR_LDS_PIECES = 3072  # boundary pieces of one mask up to which its trace works in LDS (csrc/union_contour.hip: kLdsPieces)

SWEEP_CANDIDATES = (0.1234, 0.5678, 0.9876, 1.4142, 1.7321, 2.2361, 2.7183)     # radians; the first that qualifies is used
SWEEP_ANGLE_TOL = 1e-5    # side directions closer than this are one direction (the kernel merges arcs that meet within it)
SWEEP_MIN_GAP = 1e-3      # every side direction keeps this distance (mod pi) from the level lines, and 100 tolerances from each other


def side_directions(ring_xy, ring_ptr):
    """The distinct directions (radians in [0, pi), ascending) of the sides of the rings, sides within SWEEP_ANGLE_TOL of each
    other counted once.  Raises ValueError when two distinct directions are closer than 100 x SWEEP_ANGLE_TOL: the kernel's
    angular tolerance could then not tell a shared side from a thin gap."""
    ring_xy = np.asarray(ring_xy, dtype=np.float64).reshape(-1, 2)
    ring_ptr = np.asarray(ring_ptr, dtype=np.int64)
    if ring_xy.shape[0] == 0:
        return np.zeros(0)
    nxt = np.arange(ring_xy.shape[0]) + 1
    nxt[ring_ptr[1:] - 1] = ring_ptr[:-1]                           # the last vertex of a ring goes back to its first
    d = ring_xy[nxt] - ring_xy
    d = d[(d[:, 0] != 0.0) | (d[:, 1] != 0.0)]
    ang = np.sort(np.mod(np.arctan2(d[:, 1], d[:, 0]), math.pi))
    if ang.size == 0:
        return ang
    first = np.concatenate([[True], np.diff(ang) > SWEEP_ANGLE_TOL])
    dirs = ang[first]
    if dirs.size > 1 and dirs[0] + math.pi - ang[-1] <= SWEEP_ANGLE_TOL:        # the group that wraps around pi
        dirs = dirs[1:]
    if dirs.size > 1:
        gaps = np.diff(np.concatenate([dirs, [dirs[0] + math.pi]]))
        if gaps.min() < 100.0 * SWEEP_ANGLE_TOL:
            raise ValueError(f"two side directions of the graph are {float(gaps.min()):.3g} rad apart, less than "
                             f"{100.0 * SWEEP_ANGLE_TOL:g}: the union topology's angular tolerance cannot tell them apart safely")
    return dirs


def sweep_direction(ring_xy, ring_ptr, candidates=SWEEP_CANDIDATES):
    """The angle theta of the level lines tgnn_union_topology sweeps with: the first of `candidates` that every side direction of
    the rings keeps at least SWEEP_MIN_GAP rad away from (mod pi), so that no side lies along a level line.  ValueError when
    none qualifies."""
    dirs = side_directions(ring_xy, ring_ptr)
    for theta in candidates:
        off = np.mod(dirs - theta, math.pi)
        if dirs.size == 0 or float(np.minimum(off, math.pi - off).min()) >= SWEEP_MIN_GAP:
            return float(theta)
    raise ValueError(f"every candidate sweep direction {tuple(candidates)} lies within {SWEEP_MIN_GAP:g} rad of a side of the graph")


def check_tolerance_gap(ring_xy, ring_ptr, col_ptr, col_idx, tol=UNION_TOL):
    """tgnn_union_area snaps what lies within `tol` of a side onto it, which is only sound when nothing real is that small:
    raises ValueError when a vertex of a tile lies between tol and 100 tol from a side of a tile it collides with."""
    n = ring_ptr.shape[0] - 1
    u = np.repeat(np.arange(n, dtype=np.int64), np.diff(col_ptr))
    d = vertex_side_distances(ring_xy, ring_ptr, np.stack([u, col_idx.astype(np.int64)]))
    bad = (d >= tol) & (d <= 100.0 * tol)
    if bad.any():
        raise ValueError(f"{int(bad.sum())} vertex-to-side distances between colliding tiles lie in [{tol:g}, {100 * tol:g}] "
                         f"(the smallest: {float(d[bad].min()):.3g}): the union's tolerance cannot tell noise from geometry here")
