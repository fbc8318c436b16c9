"""Host oracle of area(R n T) for the tile-in-region predicate (tilingnn_amd/csrc/region.hip), by a DIFFERENT algorithm
from the kernel's signed triangle fan: the boundary integral  area = 1/2 * sum cross(a, b)  over the boundary pieces of
R n T -- the pieces of R's edges inside T plus the pieces of T's edges inside R.  Every edge is split at its intersection
parameters with the other polygon's edges and every piece is classified by its midpoint: inside T by a point-in-polygon
test, inside R by the winding number (!= 0).  A piece lying on the other polygon's boundary counts once: from R's side when
both edges run the same way, never from T's side.  fp64; the rings are oriented here (exterior counter-clockwise, holes
clockwise) independently of the package.
"""
import numpy as np

ON_TOL = 1e-14          # coincident edges only: the complete graphs place shared vertices ~1e-12 apart, real geometry


def _open(r):
    r = np.asarray(r, dtype=np.float64).reshape(-1, 2)
    if r.shape[0] > 1 and np.array_equal(r[0], r[-1]):
        r = r[:-1]
    return r


def _sarea(r):
    x, y = r[:, 0], r[:, 1]
    return 0.5 * float(np.sum(x * np.roll(y, -1) - np.roll(x, -1) * y))


def oriented_rings(exterior, holes=()):
    ext = _open(exterior)
    rings = [ext if _sarea(ext) >= 0 else ext[::-1]]
    for h in holes:
        h = _open(h)
        rings.append(h if _sarea(h) <= 0 else h[::-1])
    return rings


def edges_of(rings):
    p = np.concatenate([r for r in rings])
    q = np.concatenate([np.roll(r, -1, axis=0) for r in rings])
    return p, q


def winding(pts, p, q):
    """Winding number of every point of pts [M, 2] about the closed edges p -> q [E, 2]."""
    px, py = pts[:, 0:1], pts[:, 1:2]
    ax, ay, bx, by = p[None, :, 0], p[None, :, 1], q[None, :, 0], q[None, :, 1]
    side = (bx - ax) * (py - ay) - (px - ax) * (by - ay)
    up = (ay <= py) & (by > py) & (side > 0)
    down = (ay > py) & (by <= py) & (side < 0)
    return up.sum(axis=1) - down.sum(axis=1)


def _on_edges(m, p, q):
    """[M, E] bool: point m within ON_TOL of edge p -> q (zero-length edges: never)."""
    d = q - p
    ln = np.hypot(d[:, 0], d[:, 1])
    rel = m[:, None, :] - p[None, :, :]
    cr = d[None, :, 0] * rel[..., 1] - d[None, :, 1] * rel[..., 0]
    t = (d[None, :, 0] * rel[..., 0] + d[None, :, 1] * rel[..., 1]) / np.maximum(ln * ln, 1e-300)[None, :]
    return (np.abs(cr) <= ON_TOL * np.maximum(ln, 1.0)[None, :]) & (t >= -1e-12) & (t <= 1 + 1e-12) & (ln > 0)[None, :]


def _split_params(a, b, p, q):
    """Intersection parameters in (0, 1) of segment a -> b with the segments p -> q (collinear overlaps: their ends)."""
    d = b - a
    e = q - p
    den = d[0] * e[:, 1] - d[1] * e[:, 0]
    ap = p - a
    s_out = [0.0, 1.0]
    nz = den != 0
    s = (ap[nz, 0] * e[nz, 1] - ap[nz, 1] * e[nz, 0]) / den[nz]
    u = (ap[nz, 0] * d[1] - ap[nz, 1] * d[0]) / den[nz]
    ok = (s > 0) & (s < 1) & (u >= -1e-15) & (u <= 1 + 1e-15)
    s_out.extend(s[ok].tolist())
    dd = float(d @ d)
    if dd > 0:
        col = ~nz & (np.abs(ap[:, 0] * d[1] - ap[:, 1] * d[0]) <= ON_TOL * max(np.sqrt(dd), 1.0))
        for pt in (p[col], q[col]):
            t = ((pt - a) @ d) / dd
            s_out.extend(t[(t > 0) & (t < 1)].tolist())
    return np.unique(np.asarray(s_out))


def _pieces(a, b, params):
    pa = a[None, :] + params[:-1, None] * (b - a)[None, :]
    pb = a[None, :] + params[1:, None] * (b - a)[None, :]
    return pa, pb


def intersection_area(rings, tile):
    """area(R n T): rings = oriented region rings, tile = an open simple ring (either orientation)."""
    t = _open(tile)
    if _sarea(t) < 0:
        t = t[::-1]
    tp, tq = t, np.roll(t, -1, axis=0)
    rp, rq = edges_of(rings)
    lo, hi = t.min(axis=0), t.max(axis=0)
    total = 0.0
    # pieces of R's edges inside T
    near = ~((np.maximum(rp[:, 0], rq[:, 0]) < lo[0]) | (np.minimum(rp[:, 0], rq[:, 0]) > hi[0]) |
             (np.maximum(rp[:, 1], rq[:, 1]) < lo[1]) | (np.minimum(rp[:, 1], rq[:, 1]) > hi[1]))
    for a, b in zip(rp[near], rq[near]):
        pa, pb = _pieces(a, b, _split_params(a, b, tp, tq))
        m = 0.5 * (pa + pb)
        on = _on_edges(m, tp, tq)
        same = ((tq - tp) @ (b - a)) > 0
        keep = np.where(on.any(axis=1), (on & same[None, :]).any(axis=1), winding(m, tp, tq) != 0)
        total += float(np.sum(pa[keep, 0] * pb[keep, 1] - pa[keep, 1] * pb[keep, 0]))
    # pieces of T's edges inside R
    for a, b in zip(tp, tq):
        pa, pb = _pieces(a, b, _split_params(a, b, rp, rq))
        m = 0.5 * (pa + pb)
        keep = ~_on_edges(m, rp, rq).any(axis=1) & (winding(m, rp, rq) != 0)
        total += float(np.sum(pa[keep, 0] * pb[keep, 1] - pa[keep, 1] * pb[keep, 0]))
    return 0.5 * total


def areas_for_region(rings, tile_rings, exact=False):
    """area(R n T_i) for every tile.  Tiles whose box meets no region edge's box have no split point: their integral is
    taken for all of them at once (every tile edge whole, kept when its midpoint winds).  exact: the other tiles in rational
    arithmetic (edges a few 1e-12 apart and nearly parallel make the fp64 split parameters ill-conditioned)."""
    rp, rq = edges_of(rings)
    out = np.zeros(len(tile_rings))
    tiles = [_open(t) for t in tile_rings]
    lo = np.array([t.min(axis=0) for t in tiles])
    hi = np.array([t.max(axis=0) for t in tiles])
    elo, ehi = np.minimum(rp, rq), np.maximum(rp, rq)
    touch = ~((ehi[None, :, 0] < lo[:, None, 0]) | (elo[None, :, 0] > hi[:, None, 0]) |
              (ehi[None, :, 1] < lo[:, None, 1]) | (elo[None, :, 1] > hi[:, None, 1]))
    busy = touch.any(axis=1)
    quiet = np.flatnonzero(~busy)
    if quiet.size:
        for i in quiet:
            t = tiles[i] if _sarea(tiles[i]) >= 0 else tiles[i][::-1]
            a, b = t, np.roll(t, -1, axis=0)
            keep = winding(0.5 * (a + b), rp, rq) != 0
            out[i] = 0.5 * float(np.sum(a[keep, 0] * b[keep, 1] - a[keep, 1] * b[keep, 0]))
    for i in np.flatnonzero(busy):
        out[i] = intersection_area_exact(rings, tiles[i]) if exact else intersection_area(rings, tiles[i])
    return out


def contained(areas, tile_areas):
    return np.abs(areas - tile_areas) < 1e-6


# ---------------------------------------------------------------------------------------------- exact, for the small cases
def _fr(v):
    from fractions import Fraction
    return Fraction(float(v))


def _winding_exact(m, edges):
    w = 0
    for (ax, ay), (bx, by) in edges:
        side = (bx - ax) * (m[1] - ay) - (m[0] - ax) * (by - ay)
        if ay <= m[1] < by and side > 0:
            w += 1
        elif by <= m[1] < ay and side < 0:
            w -= 1
    return w


def _on_exact(m, a, b):
    if a == b:
        return False
    cr = (b[0] - a[0]) * (m[1] - a[1]) - (b[1] - a[1]) * (m[0] - a[0])
    return cr == 0 and min(a[0], b[0]) <= m[0] <= max(a[0], b[0]) and min(a[1], b[1]) <= m[1] <= max(a[1], b[1])


def _split_exact(a, b, edges):
    ts = {0, 1}
    dx, dy = b[0] - a[0], b[1] - a[1]
    for p, q in edges:
        ex, ey = q[0] - p[0], q[1] - p[1]
        den = dx * ey - dy * ex
        apx, apy = p[0] - a[0], p[1] - a[1]
        if den != 0:
            s, u = (apx * ey - apy * ex) / den, (apx * dy - apy * dx) / den
            if 0 < s < 1 and 0 <= u <= 1:
                ts.add(s)
        elif apx * dy - apy * dx == 0 and (dx or dy):
            for pt in (p, q):
                t = ((pt[0] - a[0]) * dx + (pt[1] - a[1]) * dy) / (dx * dx + dy * dy)
                if 0 < t < 1:
                    ts.add(t)
    return sorted(ts)


def intersection_area_exact(rings, tile):
    """area(R n T) as intersection_area, in rational arithmetic on the exact values of the fp64 inputs; returned as float."""
    t = _open(tile)
    if _sarea(t) < 0:
        t = t[::-1]
    tv = [(_fr(x), _fr(y)) for x, y in t]
    t_edges = list(zip(tv, tv[1:] + tv[:1]))
    r_edges = []
    for r in rings:
        rv = [(_fr(x), _fr(y)) for x, y in r]
        r_edges += list(zip(rv, rv[1:] + rv[:1]))
    total = 0
    for own, other, from_region in ((r_edges, t_edges, True), (t_edges, r_edges, False)):
        for a, b in own:
            ts = _split_exact(a, b, other)
            for s0, s1 in zip(ts[:-1], ts[1:]):
                pa = (a[0] + s0 * (b[0] - a[0]), a[1] + s0 * (b[1] - a[1]))
                pb = (a[0] + s1 * (b[0] - a[0]), a[1] + s1 * (b[1] - a[1]))
                m = ((pa[0] + pb[0]) / 2, (pa[1] + pb[1]) / 2)
                on = [(p, q) for p, q in other if _on_exact(m, p, q)]
                if on:
                    keep = from_region and any((q[0] - p[0]) * (b[0] - a[0]) + (q[1] - p[1]) * (b[1] - a[1]) > 0 for p, q in on)
                else:
                    keep = _winding_exact(m, other) != 0
                if keep:
                    total += pa[0] * pb[1] - pa[1] * pb[0]
    return float(total / 2)
