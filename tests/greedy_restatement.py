"""Host restatement of the device greedy loop (tilingnn_amd/csrc/greedy.hip, greedy_many.hip, tilingnn_amd.util.algorithms.
solve_by_device_greedy) -- TEST INFRASTRUCTURE ONLY.  Plain numpy, fp64 and uint64, no torch, no GPU, no library.

The device loop is a documented SUBSTITUTE of the reference's sequential sweep, so no golden file of the reference can pin it;
what pins it is its own rule, stated once more here from the header comment of csrc/greedy.hip and from the reference lines it
keeps (/root/reference/util/algorithms.py):

  mean    (:33-34)     p = (saved^(round - 1) * prob)^(1 / round), written back as the node's saved value
  order   (:41)        larger p first; on equal p the smaller sub-layout number first
  beaten               of the two ends of a collision edge the later one in that order -- whichever way the edge is stored
  accept  (:51)        a node that no edge beats is accepted when exp(p - 1) > u, u = uniform(seed, round, ORIGINAL node number)
  label   (:196-207)   an accepted u labels v for every stored edge (u, v): collision_edges[1][collision_edges[0] == u]

Everything is vectorised over nodes and edges; tests/test_greedy_restatement_host.py holds it against a scalar loop, against
the Python big-integer form of the draw and against oracle.greedy_oracle.compute_sub_layout.

MARGINS.  The device's pow need not equal libm's bit for bit, so `saved` is compared within 1e-14 (tests/test_greedy_ops.py).
A decision (accepted or not, which end of an edge comes first) can differ between the device and this file only inside that
error of p.  Every call therefore reports how far its decisions were from flipping:
  accept   min |exp(p - 1) - u| / u over the nodes that reached the test
  order    min |p_u - p_v| / p_u over the collision edges whose two ends do NOT have bit-identical inputs (saved, prob);
           identical inputs give identical p on either side -- a true tie, decided by the node number, nothing to flip
A call with a margin below GUARD = 1e-12 (100 x the tolerance of `saved`) is UNDECIDABLE and counted.  The host test asserts
that no case of any GPU test is; that is a condition on the tests' inputs, never a tolerance of a comparison.
(Round 1 ignores saved: saved^0 = 1, so there the input is prob alone.  Two nodes whose different inputs ROUND to one p show
up as an order margin of 0 and are counted.)
"""
from collections import namedtuple

import numpy as np

GUARD = 1e-12
FINISH_MAX_NODES = 4096                                     # tgnn_greedy_finish_max_nodes()

_GOLDEN = np.uint64(0x9E3779B97F4A7C15)
_ROUND = np.uint64(0xD1B54A32D192ED03)
_MIX1 = np.uint64(0xBF58476D1CE4E5B9)
_MIX2 = np.uint64(0x94D049BB133111EB)


def uniform(seed, rnd, node):
    """The counter-based draw in [0, 1): splitmix64 of seed + golden * (node + 1) + c * (round + 1), top 53 bits.  `node`: the
    ORIGINAL node number(s); seeds are taken mod 2^64; all arithmetic wraps in uint64."""
    node = np.atleast_1d(np.asarray(node)).astype(np.uint64)
    one = np.uint64(1)
    with np.errstate(over="ignore"):
        z = np.full(node.shape, int(seed) % (1 << 64), dtype=np.uint64)
        z = z + _GOLDEN * (node + one) + _ROUND * np.full(node.shape, int(rnd) + 1, dtype=np.uint64)
        z = (z ^ (z >> np.uint64(30))) * _MIX1
        z = (z ^ (z >> np.uint64(27))) * _MIX2
        z = z ^ (z >> np.uint64(31))
    return (z >> np.uint64(11)).astype(np.float64) * 2.0 ** -53


class Margins:
    """The smallest acceptance and order margins seen, and how many calls had one below GUARD."""

    def __init__(self, accept=np.inf, order=np.inf, undecidable=0, calls=0):
        self.accept, self.order, self.undecidable, self.calls = float(accept), float(order), int(undecidable), int(calls)

    def add(self, other):
        self.accept, self.order = min(self.accept, other.accept), min(self.order, other.order)
        self.undecidable += other.undecidable
        self.calls += other.calls
        return self

    def __repr__(self):
        return f"Margins(accept={self.accept:.3g}, order={self.order:.3g}, undecidable={self.undecidable} of {self.calls})"


Round = namedtuple("Round", "saved alive selected accepted err margins")
Finish = namedtuple("Finish", "rounds_run left saved alive selected accepted err margins")


class BudgetExhausted(RuntimeError):
    """`solve` ran out of max_rounds; .left = the nodes still unlabelled (what the device loop's RuntimeError names)."""

    def __init__(self, left, max_rounds):
        super().__init__(f"{left} nodes still unlabelled after {max_rounds} rounds")
        self.left = int(left)


def _edges(col):
    if col is None:
        return np.zeros(0, dtype=np.int64), np.zeros(0, dtype=np.int64)
    col = np.asarray(col, dtype=np.int64).reshape(2, -1)
    return col[0], col[1]


def round_step(prob, inverse, col, rnd, seed, saved, alive, selected, n_sub=None, live=None):
    """One round over a sub-layout of n_sub nodes.  prob [n_sub] (None = 1 everywhere), inverse [n_sub] = original numbers
    (None = the identity; then n_sub must be given unless prob is), col [2, E] in sub-layout numbers; saved / alive / selected
    are indexed by ORIGINAL numbers and are not modified: the new state comes back in a Round, with the accepted count, the
    error word (an edge end outside [0, n_sub): that edge takes no part) and the margins.  live [n_sub] bool (None = all): the
    nodes that take part; the others, and the edges at them, are skipped (what `finish` does with nodes that have left)."""
    if n_sub is None:
        n_sub = len(inverse) if inverse is not None else len(prob)
    n_sub, rnd = int(n_sub), int(rnd)
    o = np.arange(n_sub, dtype=np.int64) if inverse is None else np.asarray(inverse, dtype=np.int64).reshape(-1)[:n_sub]
    pr = np.ones(n_sub) if prob is None else np.asarray(prob).reshape(-1)[:n_sub].astype(np.float64)
    live = np.ones(n_sub, dtype=bool) if live is None else np.asarray(live, dtype=bool)
    saved, alive, selected = np.array(saved, dtype=np.float64), np.array(alive), np.array(selected)

    before = saved[o]
    with np.errstate(all="ignore"):
        p = np.power(np.power(before, float(rnd - 1)) * pr, 1.0 / rnd)
    saved[o[live]] = p[live]

    u, v = _edges(col)
    inside = (u >= 0) & (u < n_sub) & (v >= 0) & (v < n_sub)
    err = int(not inside.all())
    u, v = u[inside], v[inside]
    both = live[u] & live[v]
    u, v = u[both], v[both]
    pair = u != v
    a, b = u[pair], v[pair]
    a_first = (p[a] > p[b]) | ((p[a] == p[b]) & (a < b))
    beaten = np.zeros(n_sub, dtype=bool)
    beaten[np.where(a_first, b, a)] = True

    tested = live & ~beaten
    draw = uniform(seed, rnd, o)
    chance = np.exp(p - 1.0)
    accepted = tested & (chance > draw)
    alive[o[accepted]] = 0
    selected[o[accepted]] = rnd
    alive[o[v[accepted[u]]]] = 0                            # the stored direction only: (u, v) with u accepted labels v

    same_input = (pr[a] == pr[b]) & ((before[a] == before[b]) if rnd > 1 else True)
    with np.errstate(all="ignore"):
        m_acc = np.abs(chance[tested] - draw[tested]) / draw[tested]
        m_ord = (np.abs(p[a] - p[b]) / p[a])[~same_input]
    m_acc = float(np.nanmin(m_acc)) if m_acc.size else np.inf
    m_ord = float(np.nanmin(m_ord)) if m_ord.size else np.inf
    margins = Margins(m_acc, m_ord, int(m_acc < GUARD or m_ord < GUARD), 1)
    return Round(saved, alive, selected, int(accepted.sum()), err, margins)


def compact(alive, adj, attr, col, x):
    """compute_sub_layout on arrays: the alive nodes in ascending order, the edges with both ends alive in their stored order,
    renumbered.  adj / col [2, E]; attr [Ea, F] and x [N, F] may be None.  -> (x', adj', attr', col', inverse)."""
    alive = np.asarray(alive).reshape(-1) != 0
    inverse = np.flatnonzero(alive).astype(np.int64)
    number = np.cumsum(alive) - 1

    def cut(ei):
        s, d = _edges(ei)
        keep = alive[s] & alive[d]
        return np.stack([number[s[keep]], number[d[keep]]]).astype(np.int64), keep

    adj2, keep_adj = cut(adj)
    col2, _ = cut(col)
    return (None if x is None else np.asarray(x)[inverse], adj2, None if attr is None else np.asarray(attr)[keep_adj], col2, inverse)


def finish(inverse, col, first_round, max_rounds, seed, saved, alive, selected, n_sub=None):
    """The remaining rounds on ONE sub-layout, every probability 1: round_step for first_round, first_round + 1, ... on the nodes
    that are still there -- entry nodes whose alive word is 0, and whoever leaves on the way, are skipped with the edges at
    them instead of being compacted away.  Stops when nobody is left or after max_rounds rounds.  -> Finish(rounds_run, left,
    state...).  (After an exhausted budget the device has already folded the NEXT round's mean into saved; this has not.)"""
    if n_sub is None:
        n_sub = len(inverse)
    o = np.arange(n_sub, dtype=np.int64) if inverse is None else np.asarray(inverse, dtype=np.int64).reshape(-1)[:n_sub]
    saved, alive, selected = np.array(saved, dtype=np.float64), np.array(alive), np.array(selected)
    margins, rounds_run, accepted, err = Margins(), 0, 0, 0
    live = alive[o] != 0
    while live.any() and rounds_run < max_rounds:
        r = round_step(None, inverse, col, first_round + rounds_run, seed, saved, alive, selected, n_sub=n_sub, live=live)
        saved, alive, selected = r.saved, r.alive, r.selected
        accepted += r.accepted
        err |= r.err
        margins.add(r.margins)
        rounds_run += 1
        live = live & (alive[o] != 0)
    return Finish(rounds_run, int(live.sum()), saved, alive, selected, accepted, err, margins)


Solve = namedtuple("Solve", "selection order rounds margins")


def solve(n, adj, col, prob_of_round, seed, max_rounds=100000, finish=True):
    """The loop of solve_by_device_greedy on a layout of n nodes: compact the unlabelled nodes; stop when there are none; a
    sub-layout without adjacency edges or without collision edges gets probability 1 (ML_Solver.predict, ml_solver.py:31-32),
    any other prob_of_round(round, inverse) -> float32 [n_sub]; one round; again.  finish: once probability 1 is all that can
    follow and the sub-layout has at most FINISH_MAX_NODES nodes, the rest is `finish` on that sub-layout (the same result
    by construction -- the host test asserts it).  -> Solve(selection [n] 0/1 float64, order (by round, then node number),
    rounds, margins); BudgetExhausted when max_rounds do not label every node."""
    run_finish = globals()["finish"]
    saved, alive, selected = np.ones(n), np.ones(n, dtype=np.int32), np.zeros(n, dtype=np.int32)
    margins, rounds = Margins(), 0
    while True:
        _, adj2, _, col2, inverse = compact(alive, adj, None, col, None)
        if inverse.size == 0:
            break
        rounds += 1
        if rounds > max_rounds:
            raise BudgetExhausted(inverse.size, max_rounds)
        ones = adj2.shape[1] == 0 or col2.shape[1] == 0
        if finish and ones and inverse.size <= FINISH_MAX_NODES:
            f = run_finish(inverse, col2, rounds, max_rounds - rounds + 1, seed, saved, alive, selected)
            saved, alive, selected = f.saved, f.alive, f.selected
            margins.add(f.margins)
            rounds += f.rounds_run - 1
            if f.left:
                raise BudgetExhausted(f.left, max_rounds)
            break
        r = round_step(None if ones else prob_of_round(rounds, inverse), inverse, col2, rounds, seed, saved, alive, selected)
        saved, alive, selected = r.saved, r.alive, r.selected
        margins.add(r.margins)
    picked = np.flatnonzero(selected > 0)
    order = [int(i) for i in picked[np.lexsort((picked, selected[picked]))]]
    return Solve((selected > 0).astype(np.float64), order, rounds, margins)
