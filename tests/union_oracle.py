"""Host oracle of the area of a union of polygons (tilingnn_amd/csrc/union_area.hip), by a DIFFERENT algorithm from the
kernel's boundary integral: a vertical slab sweep.  The abscissae of all vertices and of all pairwise edge crossings cut the
plane into slabs inside which no two edges cross; in a slab the union's area is the slab's width times the length of the 1-D
union of the polygons' even-odd cross-sections at the slab's middle (every edge is a straight line across the slab, so the
cross-section's length is linear in x and the midpoint rule is exact).  Coincident edges only make zero-height intervals, so
plain fp64 is enough; slabs narrower than 1e-13 are skipped.

Also here: the quantities the tests' gate is made of (perimeters, the largest coordinate, the largest vertex-to-side distance
below the tolerance), computed without the package.
"""
import numpy as np

MIN_SLAB = 1e-13
EPS = 2.0 ** -53


def _open(r):
    r = np.asarray(r, dtype=np.float64).reshape(-1, 2)
    if r.shape[0] > 1 and np.array_equal(r[0], r[-1]):
        r = r[:-1]
    return r


def _edges(rings):
    rings = [_open(r) for r in rings]
    p = np.concatenate(rings)
    q = np.concatenate([np.roll(r, -1, axis=0) for r in rings])
    owner = np.concatenate([np.full(r.shape[0], k) for k, r in enumerate(rings)])
    return p, q, owner


def _crossing_abscissae(p, q, block=512):
    """x of every proper or touching crossing of two edges (parallel pairs have none that matters: their ends are vertices)."""
    d = q - p
    lo, hi = np.minimum(p, q), np.maximum(p, q)
    out = []
    for s in range(0, p.shape[0], block):
        e = slice(s, s + block)
        near = ~((hi[e, None, 0] < lo[None, :, 0]) | (lo[e, None, 0] > hi[None, :, 0]) |
                 (hi[e, None, 1] < lo[None, :, 1]) | (lo[e, None, 1] > hi[None, :, 1]))
        i, j = np.nonzero(near)
        i = i + s
        keep = i < j
        i, j = i[keep], j[keep]
        den = d[i, 0] * d[j, 1] - d[i, 1] * d[j, 0]
        ok = den != 0
        i, j, den = i[ok], j[ok], den[ok]
        r = p[j] - p[i]
        t = (r[:, 0] * d[j, 1] - r[:, 1] * d[j, 0]) / den
        u = (r[:, 0] * d[i, 1] - r[:, 1] * d[i, 0]) / den
        hit = (t >= 0) & (t <= 1) & (u >= 0) & (u <= 1)
        out.append(p[i[hit], 0] + t[hit] * d[i[hit], 0])
    return np.concatenate(out) if out else np.zeros(0)


def union_area(rings):
    """Area of the union of simple polygons (open or closed rings, either orientation)."""
    rings = [r for r in (_open(r) for r in rings) if r.shape[0] >= 3]
    if not rings:
        return 0.0
    p, q, owner = _edges(rings)
    xs = np.unique(np.concatenate([p[:, 0], _crossing_abscissae(p, q)]))
    x0, x1 = xs[:-1], xs[1:]
    wide = (x1 - x0) > MIN_SLAB
    x0, x1 = x0[wide], x1[wide]
    exl, exh = np.minimum(p[:, 0], q[:, 0]), np.maximum(p[:, 0], q[:, 0])
    order = np.argsort(exl, kind="stable")
    begin_sorted = exl[order]
    total = 0.0
    start = 0
    active = np.zeros(0, dtype=np.int64)
    for a, b in zip(x0, x1):
        xm = 0.5 * (a + b)
        stop = np.searchsorted(begin_sorted, xm, side="left")          # edges that begin left of the middle
        if stop > start:
            active = np.concatenate([active, order[start:stop]])
            start = stop
        active = active[exh[active] > xm]
        if active.size == 0:
            continue
        e = active
        y = p[e, 1] + (q[e, 1] - p[e, 1]) * ((xm - p[e, 0]) / (q[e, 0] - p[e, 0]))
        by = np.lexsort((y, owner[e]))
        y, own = y[by], owner[e][by]
        assert y.size % 2 == 0 and np.array_equal(own[0::2], own[1::2]), "a ring is not closed or not simple"
        lo, hi = y[0::2], y[1::2]
        s = np.argsort(lo, kind="stable")
        lo, hi = lo[s], hi[s]
        reach = np.maximum.accumulate(hi)
        begins = np.concatenate([[True], lo[1:] > reach[:-1]])           # an interval that starts a new connected stretch
        ends = np.concatenate([begins[1:], [True]])
        total += (b - a) * float(np.sum(reach[ends] - lo[begins]))
    return total


def synthetic_tiles():
    """Eight tiles with what the lattice fixtures lack: 0 an L, 1 a U that interlocks it (given clockwise), 2 a square that holds
    both strictly inside, 3-5 rectangles sharing sides from the same side (with j < i and j > i), 6 a hook that touches the
    square 7 from outside along x = 10, y in [0, 1], and overlaps it in [10.5, 11.5] x [1, 2]."""
    box = lambda x0, y0, x1, y1: np.array([[x0, y0], [x1, y0], [x1, y1], [x0, y1]], dtype=float)
    ell = np.array([[0, 0], [3, 0], [3, 1], [1, 1], [1, 3], [0, 3]], dtype=float)
    u = np.array([[0.5, -1], [3.5, -1], [3.5, 2], [2.5, 2], [2.5, 0.5], [1.5, 0.5], [1.5, 2], [0.5, 2]], dtype=float)
    hook = np.array([[9, 0], [10, 0], [10, 1], [9.5, 1], [9.5, 2.5], [10.5, 2.5], [10.5, 1], [11.5, 1], [11.5, 3], [9, 3]], dtype=float)
    return [ell, u[::-1], box(-2, -2, 5, 5), box(6, 0, 8, 2), box(6, 0, 7, 3), box(6, 0, 9, 1), hook, box(10, 0, 12, 2)]


# ---------------------------------------------------------------------------------------------- what the gate is made of
def perimeter(ring):
    r = _open(ring)
    d = np.roll(r, -1, axis=0) - r
    return float(np.sum(np.hypot(d[:, 0], d[:, 1])))


def point_segment_distance(pt, a, b):
    d = b - a
    dd = float(d @ d)
    t = 0.0 if dd == 0.0 else min(1.0, max(0.0, float((pt - a) @ d) / dd))
    g = pt - (a + t * d)
    return float(np.hypot(g[0], g[1]))


def noise_width(rings, pairs, tol):
    """delta: the largest distance below `tol` from a vertex of one tile to a side of the other, over the given tile pairs
    [2, E] (both orders are looked at) -- how far apart sides that should coincide really are."""
    rings = [_open(r) for r in rings]
    pairs = np.asarray(pairs, dtype=np.int64).reshape(2, -1)
    keys = np.unique(np.minimum(pairs[0], pairs[1]) * len(rings) + np.maximum(pairs[0], pairs[1]))
    worst = 0.0
    for key in keys:
        i, j = int(key // len(rings)), int(key % len(rings))
        if i == j:
            continue
        for u, v in ((i, j), (j, i)):
            a, b = rings[u], np.roll(rings[u], -1, axis=0)
            rel = rings[v][:, None, :] - a[None, :, :]
            d = (b - a)[None, :, :]
            dd = np.maximum(np.sum(d * d, axis=-1), 1e-300)
            t = np.clip(np.sum(rel * d, axis=-1) / dd, 0.0, 1.0)
            g = rel - t[..., None] * d
            dist = np.hypot(g[..., 0], g[..., 1])
            small = dist[dist < tol]
            if small.size:
                worst = max(worst, float(small.max()))
    return worst


def gate(rings, delta):
    """delta * P + 64 eps R^2 n_edges for the given (alive) rings: two correct treatments of nearly coincident sides differ by
    slivers at most delta wide along the tile sides; the second term is the rounding of a sum of n_edges products of
    coordinates up to R."""
    rings = [_open(r) for r in rings]
    if not rings:
        return 0.0
    big = max(float(np.abs(r).max()) for r in rings)
    return delta * sum(perimeter(r) for r in rings) + 64.0 * EPS * big * big * sum(r.shape[0] for r in rings)
