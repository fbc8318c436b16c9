"""Host oracle of the topology of a union of polygons that do not overlap (tilingnn_amd/csrc/union_topology.hip), by a
DIFFERENT method from the kernel's sum of local Euler terms: tracing the boundary loops.

  * every side is split at the vertices (of any polygon of the set) that lie on it;
  * points are identified when they lie within SNAP of each other (a grid of cells of width CELL finds the candidates);
  * a directed sub-edge whose reverse twin exists lies inside the union and is dropped (two polygons touching along it); the same
    directed sub-edge twice means two polygons overlap: ValueError;
  * at each point an incoming boundary edge continues with the first outgoing one COUNTER-CLOCKWISE from its reversed direction.
    The union lies to the left of its boundary, so that turn goes through the outside: where polygons meet in a single point the
    inside stays connected and the outside is pinched off -- the topology of the closed union;
  * every loop is walked; holes = the loops of negative signed area (each bounded component of the complement has exactly one
    outer boundary, run clockwise);
  * components: a union-find over the polygons that share a point or have a vertex on a side of the other.

Also here: the twelve hand-made sets with the counts worked out by hand, and the lattice mask recipes the tests share.
"""
import math

import numpy as np

SNAP = 1e-5           # points closer than this are one point (noise is ~3e-8, the smallest feature 0.25)
CELL = 1e-4


def _open(r):
    r = np.asarray(r, dtype=np.float64).reshape(-1, 2)
    if r.shape[0] > 1 and np.array_equal(r[0], r[-1]):
        r = r[:-1]
    return r


def _signed_area(r):
    x, y = r[:, 0], r[:, 1]
    return 0.5 * float(np.sum(x * np.roll(y, -1) - np.roll(x, -1) * y))


class _Points:
    """Point -> id, points within SNAP of a known one get its id."""

    def __init__(self):
        self.cells = {}
        self.xy = []

    def key(self, p):
        cx, cy = int(math.floor(p[0] / CELL)), int(math.floor(p[1] / CELL))
        for dx in (-1, 0, 1):
            for dy in (-1, 0, 1):
                for k in self.cells.get((cx + dx, cy + dy), ()):
                    q = self.xy[k]
                    if math.hypot(q[0] - p[0], q[1] - p[1]) <= SNAP:
                        return k
        self.xy.append((float(p[0]), float(p[1])))
        self.cells.setdefault((cx, cy), []).append(len(self.xy) - 1)
        return len(self.xy) - 1


def topology(rings):
    """(components, holes) of the closed union of simple polygons that do not overlap (open or closed rings, either orientation)."""
    rings = [r for r in (_open(r) for r in rings) if r.shape[0] >= 3]
    rings = [r if _signed_area(r) > 0 else r[::-1] for r in rings]
    if not rings:
        return 0, 0
    pts = _Points()
    ids = [[pts.key(p) for p in r] for r in rings]
    parent = list(range(len(rings)))

    def find(a):
        while parent[a] != a:
            parent[a] = parent[parent[a]]
            a = parent[a]
        return a

    owners = {}
    for t, row in enumerate(ids):
        for k in row:
            if k in owners:
                parent[find(t)] = find(owners[k])
            owners[k] = t
    # all vertices, for the split: a few box tests per side
    allp = np.asarray(pts.xy)
    point_tiles = {}
    for t, row in enumerate(ids):
        for k in row:
            point_tiles.setdefault(k, set()).add(t)
    edges = {}                                                # (from id, to id) -> 1
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
            on = np.flatnonzero((off <= SNAP) & (along > SNAP) & (along < length - SNAP))
            on = [int(k) for k in on if k != ka and k != kb]
            for k in on:                                      # a vertex of another polygon on this side: they touch
                for other in point_tiles[k]:
                    parent[find(t)] = find(other)
            chain = [ka] + sorted(on, key=lambda k: along[k]) + [kb]
            for s, e2 in zip(chain[:-1], chain[1:]):
                if (s, e2) in edges:
                    raise ValueError("two polygons of the set overlap (the same directed boundary piece twice)")
                edges[(s, e2)] = 1
    boundary = [(s, e) for (s, e) in edges if (e, s) not in edges]
    out_of = {}
    for s, e in boundary:
        out_of.setdefault(s, []).append(e)

    def angle(frm, to):
        return math.atan2(pts.xy[to][1] - pts.xy[frm][1], pts.xy[to][0] - pts.xy[frm][0])

    nxt = {}
    for s, e in boundary:                                     # the edge s -> e arrives at e
        back = angle(e, s)
        best, best_turn = None, None
        for w in out_of.get(e, ()):
            turn = (angle(e, w) - back) % (2.0 * math.pi)
            if turn <= 1e-9:                                  # (its own twin would be; twins are gone)
                turn += 2.0 * math.pi
            if best is None or turn < best_turn:
                best, best_turn = w, turn
        if best is None:
            raise ValueError("a boundary edge with no continuation: the polygons are not simple or overlap")
        nxt[(s, e)] = (e, best)
    if len(set(nxt.values())) != len(nxt):
        raise ValueError("two boundary edges continue into the same one: the polygons overlap")
    holes, seen = 0, set()
    for start in boundary:
        if start in seen:
            continue
        area2, cur = 0.0, start
        while cur not in seen:
            seen.add(cur)
            (x0, y0), (x1, y1) = pts.xy[cur[0]], pts.xy[cur[1]]
            area2 += x0 * y1 - x1 * y0
            cur = nxt[cur]
        assert cur == start, "a boundary walk that does not close"
        holes += 1 if area2 < 0 else 0
    return len({find(t) for t in range(len(rings))}), holes


# ---------------------------------------------------------------------------------------------- hand-made sets
def _box(x0, y0, x1, y1):
    return np.array([[x0, y0], [x1, y0], [x1, y1], [x0, y1]], dtype=float)


def _grid3(skip):
    return [_box(x, y, x + 1, y + 1) for y in range(3) for x in range(3) if (x, y) not in skip]


def _block_ring():
    """Eight 3 x 3 blocks around the hole [3, 6] x [3, 6]."""
    return [_box(3 * x, 3 * y, 3 * x + 3, 3 * y + 3) for y in range(3) for x in range(3) if (x, y) != (1, 1)]


def hand_sets():
    """name -> (tiles, (components, holes)), the counts worked out by hand."""
    hexagon = np.array([[3, 3], [4, 3], [6, 5], [6, 6], [5, 6], [3, 4]], dtype=float)
    u_shape = np.array([[0, 0], [3, 0], [3, 3], [2, 3], [2, 1], [1, 1], [1, 3], [0, 3]], dtype=float)
    return {
        "one square": ([_box(0, 0, 1, 1)], (1, 0)),
        "3x3 without the centre": (_grid3({(1, 1)}), (1, 1)),
        "3x3 without centre and a corner": (_grid3({(1, 1), (0, 0)}), (1, 1)),
        "3x3 without centre and an edge square": (_grid3({(1, 1), (1, 0)}), (1, 0)),
        "pinwheel": ([_box(0, 0, 2, 1), _box(2, 0, 3, 2), _box(1, 2, 3, 3), _box(0, 1, 1, 3)], (1, 1)),
        "two squares apart": ([_box(0, 0, 1, 1), _box(3, 0, 4, 1)], (2, 0)),
        "two squares corner to corner": ([_box(0, 0, 1, 1), _box(1, 1, 2, 2)], (1, 0)),
        "block ring, square inside the hole": (_block_ring() + [_box(4, 4, 5, 5)], (2, 1)),
        "block ring, square in the hole's corner": (_block_ring() + [_box(3, 3, 4, 4)], (1, 1)),
        "block ring, hexagon bridging the hole": (_block_ring() + [hexagon], (1, 2)),
        "U closed by a bar": ([u_shape, _box(1, 3, 2, 4)], (1, 1)),
        "checkerboard": ([_box(x, y, x + 1, y + 1) for y in range(4) for x in range(4) if (x + y) % 2 == 0], (1, 2)),
    }


ROTATIONS = (0.0, 0.3, 1.1)


def rotated(tiles, angle):
    c, s = math.cos(angle), math.sin(angle)
    return [np.asarray(t, dtype=float) @ np.array([[c, s], [-s, c]]) for t in tiles]


# ---------------------------------------------------------------------------------------------- lattice masks
def independent_set(n, colli_edges, seed):
    """A maximal collision-free selection (the recipe of tests/test_union_area_gpu.py::_independent_set)."""
    col = np.asarray(colli_edges)
    rng = np.random.default_rng(seed)
    blocked, mask = np.zeros(n, dtype=bool), np.zeros(n, dtype=bool)
    order = np.argsort(col[0], kind="stable")
    starts = np.searchsorted(col[0][order], np.arange(n + 1))
    for i in rng.permutation(n):
        if not blocked[i]:
            mask[i] = True
            blocked[i] = True
            blocked[col[1][order[starts[i]:starts[i + 1]]]] = True
    assert not (mask[col[0]] & mask[col[1]]).any() and blocked.all()
    return mask


def thinned_set(n, colli_edges, seed):
    mask = independent_set(n, colli_edges, seed)
    mask &= np.random.default_rng(100 + seed).random(n) > 0.3
    return mask


SEEDS = tuple(range(8))
# (holes, components) per seed as measured when the kernel was designed; the tests quote them as a cross-check of the recipe
QUOTED = {
    ("ring9", "independent"): ((0, 0, 1, 0, 0, 1, 0, 0), (1,) * 8),
    ("ring9", "thinned"): ((40, 37, 39, 38, 44, 44, 45, 44), (1, 1, 1, 1, 1, 1, 1, 2)),
    ("small", "independent"): ((0,) * 8, (1,) * 8),
    ("small", "thinned"): ((1, 2, 2, 4, 2, 3, 3, 3), (1, 2, 1, 1, 1, 1, 1, 1)),
}
