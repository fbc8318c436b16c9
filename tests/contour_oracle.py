"""Host oracle of the outline of a union of polygons that do not overlap (tilingnn_amd/csrc/union_contour.hip): the loop walk of
tests/topology_oracle.py -- sides split at every vertex that lies on them, twins dropped, at each point the first outgoing edge
counter-clockwise from the reversed incoming one -- which RETURNS its loops instead of counting them, with the points a loop runs
straight through merged away.  Points are identified on the oracle's SNAP grid, where the kernel names them by canonical vertices:
another method, the same rings.

Also here: three hand-made sets beyond the twelve of topology_oracle.hand_sets(), and the rings of all of them written out by hand.
"""
import math

import numpy as np

from tests import topology_oracle as to

STRAIGHT = 1e-5           # rad: the kernel's kAngTol


class Ring:
    """xy [m, 2] float64 (open), area (signed: > 0 counter-clockwise, an exterior), leader: the (tile, side, position) of the
    lowest boundary piece of the ring, pieces: how many boundary pieces it is made of."""

    def __init__(self, xy, leader, pieces):
        self.xy = np.asarray(xy, dtype=np.float64).reshape(-1, 2)
        self.area = to._signed_area(self.xy) if self.xy.shape[0] >= 3 else 0.0
        self.leader = leader
        self.pieces = pieces


def contours(rings):
    """The rings of the boundary of the closed union of simple polygons that do not overlap (open or closed rings, either
    orientation; tile index = position in `rings`), in ascending leader order, each starting at the first surviving point at or
    after its leader's start.  ValueError when the polygons overlap."""
    rings = [to._open(r) for r in rings]
    assert all(r.shape[0] >= 3 for r in rings)
    rings = [r if to._signed_area(r) > 0 else r[::-1] for r in rings]
    if not rings:
        return []
    pts = to._Points()
    ids = [[pts.key(p) for p in r] for r in rings]
    allp = np.asarray(pts.xy)
    edges = {}                                                # (from id, to id) -> (tile, side, position)
    for t, (r, row) in enumerate(zip(rings, ids)):
        n = r.shape[0]
        for e in range(n):
            a, b = r[e], r[(e + 1) % n]
            ka, kb = row[e], row[(e + 1) % n]
            d = b - a
            length = float(np.hypot(d[0], d[1]))
            if ka == kb or length == 0.0:
                continue
            u = d / length
            rel = allp - a
            along = rel @ u
            off = np.abs(rel[:, 0] * u[1] - rel[:, 1] * u[0])
            on = np.flatnonzero((off <= to.SNAP) & (along > to.SNAP) & (along < length - to.SNAP))
            on = [int(k) for k in on if k != ka and k != kb]
            chain = [ka] + sorted(on, key=lambda k: along[k]) + [kb]
            for q, (s, e2) in enumerate(zip(chain[:-1], chain[1:])):
                if (s, e2) in edges:
                    raise ValueError("two polygons of the set overlap (the same directed boundary piece twice)")
                edges[(s, e2)] = (t, e, q)
    boundary = sorted(((s, e) for (s, e) in edges if (e, s) not in edges), key=edges.get)
    out_of = {}
    for s, e in boundary:
        out_of.setdefault(s, []).append(e)

    def angle(frm, to_):
        return math.atan2(pts.xy[to_][1] - pts.xy[frm][1], pts.xy[to_][0] - pts.xy[frm][0])

    nxt = {}
    for s, e in boundary:
        back = angle(e, s)
        best, best_turn = None, None
        for w in out_of.get(e, ()):
            turn = (angle(e, w) - back) % (2.0 * math.pi)
            if turn <= 1e-9:
                turn += 2.0 * math.pi
            if best is None or turn < best_turn:
                best, best_turn = w, turn
        if best is None:
            raise ValueError("a boundary edge with no continuation: the polygons are not simple or overlap")
        nxt[(s, e)] = (e, best)
    if len(set(nxt.values())) != len(nxt):
        raise ValueError("two boundary edges continue into the same one: the polygons overlap")
    out, seen = [], set()
    for start in boundary:                                    # ascending piece order: the first unseen piece of a loop leads it
        if start in seen:
            continue
        loop, cur = [], start
        while cur not in seen:
            seen.add(cur)
            loop.append(cur)
            cur = nxt[cur]
        assert cur == start, "a boundary walk that does not close"
        xy = []
        for q, (s, e) in enumerate(loop):
            ps, pe = loop[q - 1]
            turn = (angle(s, e) - angle(ps, pe) + math.pi) % (2.0 * math.pi) - math.pi
            if abs(turn) > STRAIGHT:
                xy.append(pts.xy[s])
        out.append(Ring(xy, edges[start], len(loop)))
    return out


def same_ring(a, b, tol=to.SNAP):
    """True when the open rings a and b [m, 2] list the same points in the same cyclic order (every point within tol)."""
    a, b = np.asarray(a, dtype=float).reshape(-1, 2), np.asarray(b, dtype=float).reshape(-1, 2)
    if a.shape != b.shape:
        return False
    if a.shape[0] == 0:
        return True
    for shift in np.flatnonzero(np.hypot(*(b - a[0]).T) <= tol):
        if (np.hypot(*(np.roll(b, -int(shift), axis=0) - a).T) <= tol).all():
            return True
    return False


# ---------------------------------------------------------------------------------------------- hand-made sets
def extra_sets(max_splits):
    """name -> (tiles, (components, holes)): the sets this feature adds to topology_oracle.hand_sets()."""
    box = to._box
    over = max_splits + 2
    return {
        "tip on a bar": ([box(0, 0, 4, 1), np.array([[2, 1], [3, 2], [1, 2]], dtype=float)], (1, 0)),
        "comb": ([box(0, 0, 8, 1)] + [box(x, 1, x + 1, 2) for x in range(8)], (1, 0)),
        "comb past the limit": ([box(0, 0, over, 1)] + [box(x, 1, x + 1, 2) for x in range(over)], (1, 0)),
    }


def hand_rings(max_splits):
    """name -> the rings of the whole set in the order and orientation the contract gives them, written out by hand (each may
    start anywhere: compare with same_ring)."""
    sq = lambda x, y: [(x, y), (x + 1, y), (x + 1, y + 1), (x, y + 1)]
    hole = lambda x0, y0, x1, y1: [(x0, y0), (x0, y1), (x1, y1), (x1, y0)]        # clockwise
    nine = [(0, 0), (9, 0), (9, 9), (0, 9)]
    over = max_splits + 2
    return {
        "one square": [sq(0, 0)],
        "3x3 without the centre": [[(0, 0), (3, 0), (3, 3), (0, 3)], hole(1, 1, 2, 2)],
        "3x3 without centre and a corner": [[(1, 0), (3, 0), (3, 3), (0, 3), (0, 1), (1, 1)], hole(1, 1, 2, 2)],
        "3x3 without centre and an edge square": [[(0, 0), (1, 0), (1, 2), (2, 2), (2, 0), (3, 0), (3, 3), (0, 3)]],
        "pinwheel": [[(0, 0), (3, 0), (3, 3), (0, 3)], hole(1, 1, 2, 2)],
        "two squares apart": [sq(0, 0), sq(3, 0)],
        "two squares corner to corner": [[(0, 0), (1, 0), (1, 1), (2, 1), (2, 2), (1, 2), (1, 1), (0, 1)]],
        "block ring, square inside the hole": [nine, hole(3, 3, 6, 6), sq(4, 4)],
        "block ring, square in the hole's corner": [nine, [(3, 4), (3, 6), (6, 6), (6, 3), (4, 3), (4, 4)]],
        "block ring, hexagon bridging the hole": [nine, [(4, 3), (6, 5), (6, 3)], [(3, 4), (3, 6), (5, 6)]],
        "U closed by a bar": [[(0, 0), (3, 0), (3, 3), (2, 3), (2, 4), (1, 4), (1, 3), (0, 3)], hole(1, 1, 2, 3)],
        "checkerboard": [[(0, 0), (1, 0), (1, 1), (2, 1), (2, 0), (3, 0), (3, 1), (4, 1), (4, 2), (3, 2), (3, 3), (4, 3), (4, 4),
                          (3, 4), (3, 3), (2, 3), (2, 4), (1, 4), (1, 3), (0, 3), (0, 2), (1, 2), (1, 1), (0, 1)],
                         hole(2, 1, 3, 2), hole(1, 2, 2, 3)],
        "tip on a bar": [[(0, 0), (4, 0), (4, 1), (2, 1), (3, 2), (1, 2), (2, 1), (0, 1)]],
        "comb": [[(0, 0), (8, 0), (8, 2), (0, 2)]],
        "comb past the limit": [[(0, 0), (over, 0), (over, 2), (0, 2)]],
    }


def all_sets(max_splits):
    sets = dict(to.hand_sets())
    sets.update(extra_sets(max_splits))
    return sets
