"""The hand-made sets and the expected values the hole-delta tests share (tests/test_union_hole_delta_host.py on the host,
tests/test_union_hole_delta_gpu.py on the device): the twelve sets of tests/topology_oracle.py and three more in which adding a
tile CLOSES a hole (the twelve alone never give d holes < 0), every subset of each as a mask, and for every (subset, tile outside
it) the change of (components, holes) by the loop-tracing oracle: want[m | 1 << t] - want[m].  Made once per set from the tiles
as given and shared by the rotations (a rotation changes no count), read-only."""
import numpy as np

from tests import topology_oracle as to

PLUS = np.array([(1, 0), (2, 0), (2, 1), (3, 1), (3, 2), (2, 2), (2, 3), (1, 3), (1, 2), (0, 2), (0, 1), (1, 1)], dtype=float)

# every (d components, d holes) the fifteen sets must show
PAIRS = {(-3, 0), (-2, 0), (-2, 1), (-1, 0), (-1, 1), (-1, 2), (0, -1), (0, 0), (0, 1), (0, 2), (0, 3), (1, 0)}


def box(x0, y0, x1, y1):
    return np.array([[x0, y0], [x1, y0], [x1, y1], [x0, y1]], dtype=float)


def sets():
    """name -> tiles: fifteen sets of at most 10 tiles."""
    out = {name: tiles for name, (tiles, _) in to.hand_sets().items()}
    assert len(out) == 12
    out["3x3 full"] = [box(x, y, x + 1, y + 1) for y in range(3) for x in range(3)]
    out["plus among four squares"] = [PLUS.copy(), box(1, -1, 2, 0), box(3, 1, 4, 2), box(1, 3, 2, 4), box(-1, 1, 0, 2)]
    out["frame with a plus inside"] = [box(-1, -1, 3, 0), box(3, -1, 4, 3), box(0, 3, 4, 4), box(-1, 0, 0, 4), PLUS.copy()]
    return out


def all_subsets(n):
    return ((np.arange(2 ** n)[:, None] >> np.arange(n)[None, :]) & 1).astype(np.int32)


_TABLES = {}


def subset_table(name, tiles):
    """(want [2^n, 2], delta [2^n, n, 2]): (components, holes) of every subset by the oracle, and for tile t outside subset m
    want[m | 1 << t] - want[m] (zeros where t is in m)."""
    if name not in _TABLES:
        n = len(tiles)
        masks = all_subsets(n)
        want = np.array([to.topology([tiles[i] for i in np.flatnonzero(m)]) for m in masks], dtype=np.int32)
        m_idx = np.arange(2 ** n)[:, None]
        with_t = m_idx | (1 << np.arange(n)[None, :])
        delta = (want[with_t] - want[m_idx]).astype(np.int32)
        delta[masks != 0] = 0
        want.setflags(write=False)
        delta.setflags(write=False)
        _TABLES[name] = (want, delta)
    return _TABLES[name]


def pair_counts(delta, masks):
    """{(dc, dh): count} over the (subset, outside tile) pairs of one table."""
    rows = delta[masks == 0]
    pairs, counts = np.unique(rows, axis=0, return_counts=True)
    return {(int(a), int(b)): int(c) for (a, b), c in zip(pairs, counts)}
