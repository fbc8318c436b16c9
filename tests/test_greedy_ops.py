"""The entries that turn probabilities into a tiling -- tgnn_greedy_round, tgnn_greedy_finish (csrc/greedy.hip), tgnn_greedy_round_many,
tgnn_greedy_finish_many, tgnn_sublayout_compact_many (csrc/greedy_many.hip) -- each held DIRECTLY against the host restatement of
their rule (tests/greedy_restatement.py), not against each other: the sizes at which the kernels change path (wavefront, block,
the 4096 x 256 grid cap, the word-packed LDS flags' tail, the 1024-item chunks and the 256-wide plan scan of the `_many` entries),
NULL and strided arguments, ties, self loops, duplicated, one-way and out-of-range edges.

COMPARISON RULE (here and in tests/test_greedy_solve_restated.py): alive, selected, n_selected, the error word and `out` are equal;
`saved` within rtol 1e-14 (the device's pow need not equal libm's bit for bit); entries of saved / alive / selected outside the
sub-layout hold sentinels and are untouched.  A decision can only differ inside the error of p, so the inputs are chosen such
that no decision is within 1e-12 of flipping: tests/test_greedy_restatement_host.py asserts that for every case table built
here (they are numpy only, so the host test can import them).
"""
import ctypes as C
import functools

import numpy as np
import pytest
import torch

from tests import greedy_restatement as gr

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda:0")
RTOL_SAVED = 1e-14
S_SAVED, S_ALIVE, S_SEL, S_OUT = -5.0, -7, -9, -77           # sentinels
PAD = 8                                                      # sentinel entries behind every state array

ROUND_SIZES = (1, 63, 64, 65, 255, 256, 257, 1025, 5000)
ROUNDS = (1, 2, 7, 40)
SEEDS = (0, 2 ** 63 + 5, 2 ** 64 - 1)
VARIANTS = ("both", "loops_dups", "none", "oneway", "oob")
FINISH_SIZES = (1, 3, 4, 5, 1023, 1024, 1025, 4095, 4096)
FIRST_ROUNDS = (1, 4, 9)
FINISH_VARIANTS = ("both", "loops_dups", "oneway", "none")


# ------------------------------------------------------------------------------------------------ inputs (numpy only)
def make_edges(rng, n, variant, tied, per_node=4):
    """[2, E] collision edges of a sub-layout of n nodes (None: no edges, a NULL pointer).  both: every pair stored both ways,
    as the reference stores them (tile_graph.py:206-207); loops_dups: plus self loops and repeated edges; oneway: every pair
    stored once; oob: both, with some ends outside [0, n).  `tied`: nodes with identical inputs -- some pairs are drawn among
    them, so that the node-number tie-break decides."""
    if variant == "none":
        return None
    if n == 1:
        pairs = np.zeros((2, 0), dtype=np.int64)
    else:
        m = per_node * n
        u = rng.integers(0, n, size=m)
        v = (u + rng.integers(1, min(n, 40), size=m)) % n
        if len(tied) >= 2:
            a = rng.choice(tied, size=2 * len(tied))
            b = rng.choice(tied, size=2 * len(tied))
            u, v = np.concatenate([u, a[a != b]]), np.concatenate([v, b[a != b]])
        pairs = np.stack([u, v]).astype(np.int64)
    if variant == "oneway":
        col = pairs
    else:
        col = np.concatenate([pairs, pairs[::-1]], axis=1)
    if variant == "loops_dups" or col.shape[1] == 0:
        loops = rng.integers(0, n, size=n // 10 + 1)
        col = np.concatenate([col, np.stack([loops, loops]), col[:, :col.shape[1] // 5]], axis=1)
    if variant == "oob":
        bad = np.array([[0, -1, n, n + 5, 2 ** 40], [n, 0, 0, -2, 0]], dtype=np.int64)
        col = np.concatenate([col, bad], axis=1)
        col = col[:, rng.permutation(col.shape[1])]
    return np.ascontiguousarray(col)


class Case:
    """The arguments of one call and the state before it; .want() = the restatement's answer (computed once)."""

    def __init__(self, name, **kw):
        self.name = name
        self.__dict__.update(kw)

    @functools.lru_cache(maxsize=None)
    def want(self):
        return self.restate()


def _state(rng, n, with_inverse, rnd, tie_frac=0.04):
    """saved / alive / selected over the ORIGINAL numbering with sentinels wherever the sub-layout does not reach, the inverse
    (None: the identity) and the block of tied nodes."""
    n_orig = 3 * n if with_inverse else n
    inverse = np.sort(rng.choice(n_orig, size=n, replace=False)).astype(np.int64) if with_inverse else None
    o = inverse if with_inverse else np.arange(n)
    saved = np.full(n_orig + PAD, S_SAVED)
    alive = np.full(n_orig + PAD, S_ALIVE, dtype=np.int32)
    selected = np.full(n_orig + PAD, S_SEL, dtype=np.int32)
    if rnd == 1:                                             # saved^0 = 1 must ignore whatever is there
        saved[o] = rng.choice([0.0, 0.3, 7.5, 1e300], size=n)
    else:
        saved[o] = rng.uniform(0.2, 1.0, size=n)
    alive[o], selected[o] = 1, 0
    n_tied = max(2, int(round(tie_frac * n))) if n >= 2 else 0
    t0 = int(rng.integers(0, n - n_tied + 1)) if n_tied else 0
    tied = np.arange(t0, t0 + n_tied)
    if rnd > 1:
        saved[o[tied]] = 0.7
    return inverse, o, saved, alive, selected, tied


def build_round_case(name, n, with_inverse, rnd, seed, ld, variant, n_sel0, rng_seed, n_edges=None):
    rng = np.random.default_rng(rng_seed)
    inverse, o, saved, alive, selected, tied = _state(rng, n, with_inverse, rnd)
    column = ld // 2
    prob = rng.uniform(0.05, 1.0, size=(n, ld)).astype(np.float32)
    prob[tied, column] = 0.5
    if n_edges is None:
        col = make_edges(rng, n, variant, tied)
    else:                                                    # (more edges than one sweep of the grid covers)
        u = rng.integers(0, n, size=n_edges)
        col = np.stack([u, (u + rng.integers(1, 40, size=n_edges)) % n]).astype(np.int64)

    def restate():
        return gr.round_step(prob[:, column], inverse, col, rnd, seed, saved, alive, selected, n_sub=n)
    return Case(name, n=n, inverse=inverse, rnd=rnd, seed=seed, ld=ld, column=column, variant=variant, n_sel0=n_sel0, prob=prob, col=col,
                saved=saved, alive=alive, selected=selected, restate=restate)


def _round_specs():
    """Every size x {no inverse, inverse} x every round; the seed, the stride, the edge variant and the starting count are dealt
    round-robin from a shuffled deck, so that every value meets every size (the host test checks the coverage)."""
    rng = np.random.default_rng(2024)
    specs, i = {}, 0
    for n in ROUND_SIZES:
        for with_inverse in (False, True):
            for rnd in rng.permutation(ROUNDS):
                seed, ld = SEEDS[i % 3], (1, 3)[(i // 3) % 2]
                variant = VARIANTS[(i + i // 5) % 5]
                n_sel0 = 17 if i % 4 == 1 else 0
                name = f"n{n}-{'inv' if with_inverse else 'id'}-r{rnd}-s{SEEDS.index(seed)}-ld{ld}-{variant}-c{n_sel0}"
                specs[name] = (n, with_inverse, int(rnd), seed, ld, variant, n_sel0, 1000 + i)
                i += 1
    # past one sweep of the 4096 x 256 grid: nodes, then edges (the kernels' grid-stride loops take a second turn)
    specs["n1048653-no-edges"] = (1048653, False, 2, SEEDS[1], 1, "none", 0, 5001)
    specs["n3000-e1048653"] = (3000, True, 7, SEEDS[2], 1, "oneway", 17, 5002, 1048653)
    return specs


ROUND_SPECS = _round_specs()


@functools.lru_cache(maxsize=None)
def round_case(name):
    return build_round_case(name, *ROUND_SPECS[name])


def build_finish_case(name, n, first_round, with_inverse, dead_frac, variant, seed, max_rounds, rng_seed, per_node=4):
    rng = np.random.default_rng(rng_seed)
    inverse, o, saved, alive, selected, tied = _state(rng, n, with_inverse, max(first_round, 2))
    if dead_frac:
        dead = rng.uniform(size=n) < dead_frac
        alive[o[dead]] = 0
        selected[o[dead]] = np.where(rng.uniform(size=int(dead.sum())) < 0.3, 1, 0)      # (left in an earlier round, some of them selected)
    col = make_edges(rng, n, variant, tied, per_node)

    def restate():
        return gr.finish(inverse, col, first_round, max_rounds, seed, saved, alive, selected, n_sub=n)
    return Case(name, n=n, inverse=inverse, first_round=first_round, seed=seed, max_rounds=max_rounds, variant=variant, col=col,
                dead_frac=dead_frac, saved=saved, alive=alive, selected=selected, restate=restate)


def _finish_specs():
    specs, i = {}, 0
    for n in FINISH_SIZES:
        for first_round in FIRST_ROUNDS:
            with_inverse, dead = i % 2 == 1, (0.0, 0.3)[(i // 2) % 2]
            variant, seed = FINISH_VARIANTS[(i + i // 4) % 4], SEEDS[i % 3]
            specs[f"n{n}-first{first_round}-{'inv' if with_inverse else 'id'}-dead{dead}-{variant}-s{SEEDS.index(seed)}"] = \
                (n, first_round, with_inverse, dead, variant, seed, 1000, 2000 + i)
            i += 1
    return specs


FINISH_SPECS = _finish_specs()
# the budget runs out: out = [max_rounds, left > 0] (dense collisions, so that one or two rounds cannot label everybody)
BUDGET_SPECS = {f"n{n}-budget{m}-first{f}": (n, f, True, 0.0, "both", SEEDS[m % 3], m, 3000 + n + m, 12)
                for n, f in ((1025, 4), (4096, 1)) for m in (1, 2)}


@functools.lru_cache(maxsize=None)
def finish_case(name):
    return build_finish_case(name, *(FINISH_SPECS.get(name) or BUDGET_SPECS[name]))


class ManyCase:
    """K sub-layouts packed as csrc/greedy_many.hip wants them.  layouts: dicts with full_n, full_ec (the slots of the packed
    arrays), inverse [n_sub] (ascending local original numbers), col [2, ec_sub] or None, prob [n_sub, ld] or None (a NULL
    table entry: probability 1), seed, active, n_sel0, and for the bad-inverse case `bad` = the sub-layout node whose inverse
    entry is out of range (an isolated node: the rest of its layout is then the restatement without it)."""

    def __init__(self, name, layouts, rnd, ld, column, first_round=None, max_rounds=1000):
        self.name, self.layouts, self.rnd, self.ld, self.column = name, layouts, rnd, ld, column
        self.first_round, self.max_rounds = first_round, max_rounds
        self.K = len(layouts)
        self.node_ptr = np.concatenate([[0], np.cumsum([l["full_n"] for l in layouts])]).astype(np.int64)
        self.col_ptr = np.concatenate([[0], np.cumsum([l["full_ec"] for l in layouts])]).astype(np.int64)
        self.counts = np.array([[len(l["inverse"]), 0, 0 if l["col"] is None else l["col"].shape[1]] for l in layouts], dtype=np.int64)

    def packed(self):
        n, ec = int(self.node_ptr[-1]), int(self.col_ptr[-1])
        inverse = np.full(n + PAD, S_OUT, dtype=np.int64)
        col = np.full(2 * ec + PAD, S_OUT, dtype=np.int64)
        saved, alive, selected = np.full(n + PAD, S_SAVED), np.full(n + PAD, S_ALIVE, dtype=np.int32), np.full(n + PAD, S_SEL, dtype=np.int32)
        for k, l in enumerate(self.layouts):
            n0, c0 = int(self.node_ptr[k]), int(self.col_ptr[k])
            inv = l["inverse"].copy()
            if l.get("bad") is not None:
                inv[l["bad"]] = l["bad_value"]
            inverse[n0:n0 + len(inv)] = inv
            if l["col"] is not None:
                e = l["col"].shape[1]
                col[2 * c0:2 * c0 + 2 * e] = l["col"].reshape(-1)
            saved[n0:n0 + l["full_n"]], alive[n0:n0 + l["full_n"]], selected[n0:n0 + l["full_n"]] = l["saved"], l["alive"], l["selected"]
        return inverse, col, saved, alive, selected

    @functools.lru_cache(maxsize=None)
    def want(self, entry):
        """Per layout: the restatement's Round (entry 'round') or Finish (entry 'finish'), None for a layout that sits out."""
        out = []
        for l in self.layouts:
            if not l["active"]:
                out.append(None)
                continue
            n_sub = len(l["inverse"])
            live = None
            if l.get("bad") is not None:
                live = np.ones(n_sub, dtype=bool)
                live[l["bad"]] = False
            if entry == "round":
                prob = None if l["prob"] is None else l["prob"][:, self.column]
                out.append(gr.round_step(prob, l["inverse"], l["col"], self.rnd, l["seed"], l["saved"], l["alive"], l["selected"],
                                         n_sub=n_sub, live=live))
            else:
                out.append(gr.finish(l["inverse"], l["col"], self.first_round, self.max_rounds, l["seed"], l["saved"], l["alive"],
                                     l["selected"], n_sub=n_sub))
        return out


def _many_layout(rng, n_sub, ec_sub, rnd, ld, seed, active=True, null_prob=False, n_sel0=0, slack=7, variant="both"):
    full_n = n_sub + slack
    inverse = np.sort(rng.choice(full_n, size=n_sub, replace=False)).astype(np.int64)
    saved, alive, selected = np.full(full_n, S_SAVED), np.full(full_n, S_ALIVE, dtype=np.int32), np.full(full_n, S_SEL, dtype=np.int32)
    saved[inverse] = rng.choice([0.0, 0.3, 7.5], size=n_sub) if rnd == 1 else rng.uniform(0.2, 1.0, size=n_sub)
    alive[inverse], selected[inverse] = 1, 0
    col = None
    if ec_sub and n_sub >= 2:
        half = ec_sub // 2
        u = rng.integers(0, n_sub, size=half)
        v = (u + rng.integers(1, min(n_sub, 40), size=half)) % n_sub
        col = np.concatenate([np.stack([u, v]), np.stack([v, u])], axis=1).astype(np.int64)
        if ec_sub % 2:                                       # (an odd count: one self loop on top)
            col = np.concatenate([col, np.array([[n_sub // 2], [n_sub // 2]])], axis=1)
        if variant == "oneway":
            col = np.stack([u, v]).astype(np.int64)
    prob = None if null_prob else rng.uniform(0.05, 1.0, size=(n_sub, ld)).astype(np.float32)
    return dict(full_n=full_n, full_ec=(0 if col is None else col.shape[1]) + 3, inverse=inverse, col=col, prob=prob, seed=seed,
                active=active, n_sel0=n_sel0, saved=saved, alive=alive, selected=selected)


MANY_SIZES = ((1, 0), (1023, 1024), (1024, 1025), (1025, 4000), (2300, 9000), (500, 300))     # (nodes, collision edges) of the sub-layouts


@functools.lru_cache(maxsize=None)
def many_chunk_case(rnd):
    """The chunk edges of the `_many` entries (1024 items per block): 1, 1023, 1024, 1025, 2300 nodes, 0 / 1024 / 1025 collision
    edges, one layout inactive (the last), one NULL probability entry, ld_prob = 2 read at column 1, a seed per layout."""
    rng = np.random.default_rng(700 + rnd)
    seeds = (11, 2 ** 63 + 5, 0, 2 ** 64 - 1, 12345, 7)
    layouts = [_many_layout(rng, n, ec, rnd, 2, seeds[k], active=k != 5, null_prob=k == 1, n_sel0=17 if k == 3 else 0)
               for k, (n, ec) in enumerate(MANY_SIZES)]
    return ManyCase(f"chunks-r{rnd}", layouts, rnd, 2, 1, first_round=rnd)


@functools.lru_cache(maxsize=None)
def many_300_case():
    """K = 300 layouts of 1 to 5 nodes, active and inactive on both sides of layout 256: the plan's scan takes its second
    256-wide pass (mode 0), the carry of the first must reach it."""
    rng = np.random.default_rng(300)
    layouts = []
    for k in range(300):
        n_sub = int(rng.integers(1, 6))
        layouts.append(_many_layout(rng, n_sub, 2 * int(rng.integers(0, 4)), 3, 1, 1000003 * k + 5, active=bool(rng.uniform() < 0.7),
                                    null_prob=k % 11 == 0, n_sel0=k % 3, slack=int(rng.integers(0, 3))))
    return ManyCase("k300", layouts, 3, 1, 0, first_round=3)


@functools.lru_cache(maxsize=None)
def many_bad_inverse_case():
    """Layout 1 of three has one inverse entry out of range, at an isolated node."""
    rng = np.random.default_rng(77)
    layouts = [_many_layout(rng, n, ec, 2, 1, 40 + k) for k, (n, ec) in enumerate(((300, 1200), (1100, 4400), (64, 200)))]
    l = layouts[1]
    bad = 1030                                               # (in the second chunk of its layout)
    if l["col"] is not None:
        keep = (l["col"][0] != bad) & (l["col"][1] != bad)
        l["col"] = np.ascontiguousarray(l["col"][:, keep])
    l["bad"], l["bad_value"] = bad, l["full_n"]              # one past the layout's last node
    l["saved"][l["inverse"][bad]], l["alive"][l["inverse"][bad]], l["selected"][l["inverse"][bad]] = S_SAVED, 0, S_SEL    # nobody's node now
    return ManyCase("bad-inverse", layouts, 2, 1, 0, first_round=2)


ALL_CASE_TABLES = {
    "tgnn_greedy_round": lambda: [round_case(k) for k in ROUND_SPECS],
    "tgnn_greedy_finish": lambda: [finish_case(k) for k in list(FINISH_SPECS) + list(BUDGET_SPECS)],
}
MANY_CASE_TABLES = {
    "many, chunk edges": lambda: [(many_chunk_case(r), e) for r in (1, 3) for e in ("round", "finish")],
    "many, K = 300": lambda: [(many_300_case(), e) for e in ("round", "finish")],
    "many, bad inverse": lambda: [(many_bad_inverse_case(), e) for e in ("round", "finish")],
}


# ------------------------------------------------------------------------------------------------ the device side
def _t(a, dt=None):
    t = torch.from_numpy(np.ascontiguousarray(a))
    return (t if dt is None else t.to(dt)).to(DEV)


SAVED_DEVIATION = [0.0]                                      # the largest relative deviation of `saved` seen in this run


def assert_state(saved_d, alive_d, sel_d, want, compare_saved=True, label=""):
    alive, sel, saved = alive_d.cpu().numpy(), sel_d.cpu().numpy(), saved_d.cpu().numpy()
    assert np.array_equal(alive, want.alive), f"{label}: alive differs at {np.flatnonzero(alive != want.alive)[:8]}"
    assert np.array_equal(sel, want.selected), f"{label}: selected differs at {np.flatnonzero(sel != want.selected)[:8]}"
    if compare_saved:
        nz = want.saved != 0
        dev = float(np.max(np.abs(saved[nz] - want.saved[nz]) / np.abs(want.saved[nz]))) if nz.any() else 0.0
        SAVED_DEVIATION[0] = max(SAVED_DEVIATION[0], dev)
        print(f"{label}: largest relative deviation of saved {dev:.3g} (gate {RTOL_SAVED:g}; this run so far {SAVED_DEVIATION[0]:.3g})")
        np.testing.assert_allclose(saved, want.saved, rtol=RTOL_SAVED, atol=0.0)


@pytest.mark.parametrize("name", list(ROUND_SPECS))
def test_greedy_round_is_the_restated_round(name):
    from tilingnn_amd import _lib
    from tilingnn_amd._lib import check, lib, ptr
    c = round_case(name)
    want = c.want()
    assert want.margins.undecidable == 0, want.margins         # (a condition on the inputs, asserted without a GPU as well)
    prob_d, saved_d, alive_d, sel_d = _t(c.prob), _t(c.saved), _t(c.alive), _t(c.selected)
    inv_d = None if c.inverse is None else _t(c.inverse)
    col_d = None if c.col is None else _t(c.col)
    ec = 0 if c.col is None else int(c.col.shape[1])
    tail = _t(np.array([c.n_sel0, 0], dtype=np.int64))
    wsb = int(lib.tgnn_greedy_round_workspace_bytes(c.n))
    ws = torch.empty(wsb, dtype=torch.uint8, device=DEV)
    check(lib.tgnn_greedy_round(C.c_void_p(prob_d.data_ptr() + 4 * c.column), c.ld, ptr(inv_d), c.n, ptr(col_d), ec, c.rnd, c.seed,
                                ptr(saved_d), ptr(alive_d), ptr(sel_d), ptr(tail[:1]), ptr(tail[1:].view(torch.int32)[:1]), ptr(ws), wsb,
                                _lib.current_stream(DEV)))
    torch.cuda.synchronize()
    assert int(tail[0]) == c.n_sel0 + want.accepted
    assert int(tail[1:].view(torch.int32)[0]) == want.err == int(c.variant == "oob")
    assert_state(saved_d, alive_d, sel_d, want, label=name)
    if c.variant == "oneway":                                  # stored one way only, the two ends are still kept apart within the round
        o = c.inverse if c.inverse is not None else np.arange(c.n)
        acc = sel_d.cpu().numpy()[o] == c.rnd
        u, v = c.col
        assert not np.any(acc[u] & acc[v] & (u != v))


def _run_finish(c, n_sub=None):
    from tilingnn_amd import _lib
    from tilingnn_amd._lib import lib, ptr
    saved_d, alive_d, sel_d = _t(c.saved), _t(c.alive), _t(c.selected)
    inv_d = None if c.inverse is None else _t(c.inverse)
    col_d = None if c.col is None else _t(c.col)
    ec = 0 if c.col is None else int(c.col.shape[1])
    tail = _t(np.array([17, 0], dtype=np.int64))
    out = torch.full((2,), S_OUT, dtype=torch.int32, device=DEV)
    rc = lib.tgnn_greedy_finish(ptr(inv_d), c.n if n_sub is None else n_sub, ptr(col_d), ec, c.first_round, c.max_rounds, c.seed, ptr(saved_d),
                                ptr(alive_d), ptr(sel_d), ptr(tail[:1]), ptr(tail[1:].view(torch.int32)[:1]), ptr(out),
                                _lib.current_stream(DEV))
    torch.cuda.synchronize()
    return rc, saved_d, alive_d, sel_d, tail, out


@pytest.mark.parametrize("name", list(FINISH_SPECS))
def test_greedy_finish_is_the_restated_rounds(name):
    c = finish_case(name)
    want = c.want()
    assert want.margins.undecidable == 0, want.margins
    assert want.left == 0
    rc, saved_d, alive_d, sel_d, tail, out = _run_finish(c)
    assert rc == 0
    assert out.cpu().tolist() == [want.rounds_run, want.left]
    assert int(tail[0]) == 17 + want.accepted and int(tail[1:].view(torch.int32)[0]) == want.err == 0
    assert_state(saved_d, alive_d, sel_d, want, label=name)
    print(f"{name}: {want.rounds_run} rounds from round {c.first_round}, {want.accepted} accepted")


@pytest.mark.parametrize("name", list(BUDGET_SPECS))
def test_greedy_finish_out_of_budget_reports_the_nodes_left(name):
    """out = [max_rounds, left > 0].  `saved` is NOT compared here: the kernel folds the next round's mean before it notices
    that the budget is spent (the caller raises); everything else is the restatement's."""
    c = finish_case(name)
    want = c.want()
    assert want.margins.undecidable == 0, want.margins
    assert want.left > 0 and want.rounds_run == c.max_rounds
    rc, saved_d, alive_d, sel_d, tail, out = _run_finish(c)
    assert rc == 0
    assert out.cpu().tolist() == [c.max_rounds, want.left]
    assert int(tail[0]) == 17 + want.accepted and int(tail[1:].view(torch.int32)[0]) == 0
    assert_state(saved_d, alive_d, sel_d, want, compare_saved=False, label=name)
    untouched = c.saved == S_SAVED                              # (the sentinels of saved are still held to)
    assert np.array_equal(saved_d.cpu().numpy()[untouched], c.saved[untouched])


def test_greedy_finish_refuses_more_nodes_than_one_block_holds():
    from tilingnn_amd._lib import lib
    assert int(lib.tgnn_greedy_finish_max_nodes()) == gr.FINISH_MAX_NODES
    c = build_finish_case("n4097", 4097, 2, False, 0.0, "both", 5, 1000, 4097)
    rc, saved_d, alive_d, sel_d, tail, out = _run_finish(c)
    assert rc == -1 and b"shape" in lib.tgnn_last_error()
    assert out.cpu().tolist() == [S_OUT, S_OUT] and tail.cpu().tolist() == [17, 0]
    assert np.array_equal(saved_d.cpu().numpy(), c.saved) and np.array_equal(alive_d.cpu().numpy(), c.alive)
    assert np.array_equal(sel_d.cpu().numpy(), c.selected)


# ------------------------------------------------------------------------------------------------ the `_many` entries
class ManyDevice:
    def __init__(self, case):
        self.c = c = case
        inverse, col, saved, alive, selected = c.packed()
        self.inverse, self.col, self.saved, self.alive, self.selected = _t(inverse), _t(col), _t(saved), _t(alive), _t(selected)
        self.node_ptr, self.col_ptr, self.counts = _t(c.node_ptr), _t(c.col_ptr), _t(c.counts)
        self.n, self.ec = int(c.node_ptr[-1]), int(c.col_ptr[-1])
        self.seeds = _t(np.array([l["seed"] for l in c.layouts], dtype=np.uint64).view(np.int64))
        self.active = _t(np.array([int(l["active"]) for l in c.layouts], dtype=np.int32))
        self.n_sel = _t(np.array([l["n_sel0"] for l in c.layouts], dtype=np.int64))
        self.err = torch.zeros(c.K, dtype=torch.int32, device=DEV)
        self.probs = [None if l["prob"] is None else _t(l["prob"]) for l in c.layouts]
        self.table = _t(np.array([0 if p is None else p.data_ptr() + 4 * c.column for p in self.probs], dtype=np.int64))

    def round(self):
        from tilingnn_amd import _lib
        from tilingnn_amd._lib import check, lib, ptr
        c = self.c
        wsb = int(lib.tgnn_greedy_round_many_workspace_bytes(c.K, self.n))
        ws = torch.empty(wsb, dtype=torch.uint8, device=DEV)
        check(lib.tgnn_greedy_round_many(c.K, ptr(self.active), ptr(self.table), c.ld, ptr(self.node_ptr), ptr(self.col_ptr), self.n, self.ec,
                                         ptr(self.counts), ptr(self.inverse), ptr(self.col), c.rnd, ptr(self.seeds), ptr(self.saved),
                                         ptr(self.alive), ptr(self.selected), ptr(self.n_sel), ptr(self.err), ptr(ws), wsb,
                                         _lib.current_stream(DEV)))
        torch.cuda.synchronize()

    def finish(self):
        from tilingnn_amd import _lib
        from tilingnn_amd._lib import check, lib, ptr
        c = self.c
        self.out = torch.full((c.K, 2), S_OUT, dtype=torch.int32, device=DEV)
        check(lib.tgnn_greedy_finish_many(c.K, ptr(self.active), ptr(self.node_ptr), ptr(self.col_ptr), self.n, self.ec, ptr(self.counts),
                                          ptr(self.inverse), ptr(self.col), c.first_round, c.max_rounds, ptr(self.seeds), ptr(self.saved),
                                          ptr(self.alive), ptr(self.selected), ptr(self.n_sel), ptr(self.err), ptr(self.out),
                                          _lib.current_stream(DEV)))
        torch.cuda.synchronize()

    def compare(self, entry):
        """Layout by layout against the restatement; a layout that sits out keeps every word it had."""
        c = self.c
        wants = c.want(entry)
        saved, alive, selected = self.saved.cpu().numpy(), self.alive.cpu().numpy(), self.selected.cpu().numpy()
        n_sel, err = self.n_sel.cpu().tolist(), self.err.cpu().tolist()
        out = self.out.cpu().tolist() if entry == "finish" else None
        State = gr.Round
        worst = 0.0
        for k, (l, w) in enumerate(zip(c.layouts, wants)):
            sl = slice(int(c.node_ptr[k]), int(c.node_ptr[k + 1]))
            if w is None:
                w = State(l["saved"], l["alive"], l["selected"], 0, 0, None)
                if out is not None:
                    assert out[k] == [S_OUT, S_OUT], k
            else:
                assert w.margins.undecidable == 0, (k, w.margins)
                if out is not None:
                    assert out[k] == [w.rounds_run, w.left], k
            assert np.array_equal(alive[sl], w.alive), f"{c.name}: layout {k}: alive"
            assert np.array_equal(selected[sl], w.selected), f"{c.name}: layout {k}: selected"
            assert n_sel[k] == l["n_sel0"] + w.accepted, f"{c.name}: layout {k}: n_selected"
            assert err[k] == int(l.get("bad") is not None and l["active"]), f"{c.name}: layout {k}: error word"
            nz = w.saved != 0
            if nz.any():
                worst = max(worst, float(np.max(np.abs(saved[sl][nz] - w.saved[nz]) / np.abs(w.saved[nz]))))
            np.testing.assert_allclose(saved[sl], w.saved, rtol=RTOL_SAVED, atol=0.0, err_msg=f"{c.name}: layout {k}: saved")
        for arr, s in ((saved, S_SAVED), (alive, S_ALIVE), (selected, S_SEL)):
            assert (arr[self.n:] == s).all()
        SAVED_DEVIATION[0] = max(SAVED_DEVIATION[0], worst)
        print(f"{c.name} {entry}: largest relative deviation of saved {worst:.3g} (gate {RTOL_SAVED:g}; this run so far {SAVED_DEVIATION[0]:.3g})")


@pytest.mark.parametrize("rnd", [1, 3])
def test_round_many_at_the_chunk_edges_is_the_restated_round_per_layout(rnd):
    st = ManyDevice(many_chunk_case(rnd))
    st.round()
    st.compare("round")
    assert st.c.want("round")[5] is None and sum(w.accepted for w in st.c.want("round")[:5]) > 100


@pytest.mark.parametrize("rnd", [1, 3])
def test_finish_many_at_the_chunk_edges_is_the_restated_finish_per_layout(rnd):
    st = ManyDevice(many_chunk_case(rnd))
    st.finish()
    st.compare("finish")
    assert all(w.left == 0 for w in st.c.want("finish")[:5])


@pytest.mark.parametrize("entry", ["round", "finish"])
def test_three_hundred_small_layouts_pass_the_plans_second_scan(entry):
    st = ManyDevice(many_300_case())
    getattr(st, entry)()
    st.compare(entry)
    active = [l["active"] for l in st.c.layouts]
    assert any(active[:256]) and not all(active[:256]) and any(active[256:]) and not all(active[256:])


@pytest.mark.parametrize("entry", ["round", "finish"])
def test_an_inverse_entry_out_of_range_sets_the_layouts_error_word_and_is_never_accepted(entry):
    """The node's original number is unusable: the entry reports it (error word of ITS layout), never accepts the node and
    writes nothing through it; the node is isolated here, so the rest of its layout -- and the other layouts -- are the
    restatement without it."""
    c = many_bad_inverse_case()
    st = ManyDevice(c)
    getattr(st, entry)()
    st.compare(entry)                                          # (error words [0, 1, 0]; the accepted counts leave the node out)
    assert st.err.cpu().tolist() == [0, 1, 0]


def test_a_finish_word_on_a_layout_too_large_for_one_block_is_an_error_word():
    rng = np.random.default_rng(4097)
    layouts = [_many_layout(rng, 40, 100, 2, 1, 3), _many_layout(rng, 4097, 8000, 2, 1, 4), _many_layout(rng, 1, 0, 2, 1, 5)]
    c = ManyCase("finish-4097", layouts, 2, 1, 0, first_round=2)
    st = ManyDevice(c)
    st.finish()
    assert st.err.cpu().tolist() == [0, 1, 0]
    assert st.out.cpu().tolist()[1] == [0, 4097]
    sl = slice(int(c.node_ptr[1]), int(c.node_ptr[2]))
    assert np.array_equal(st.saved.cpu().numpy()[sl], layouts[1]["saved"]) and np.array_equal(st.alive.cpu().numpy()[sl], layouts[1]["alive"])
    assert np.array_equal(st.selected.cpu().numpy()[sl], layouts[1]["selected"]) and int(st.n_sel[1]) == 0
    for k in (0, 2):                                           # the others finish as restated
        w = gr.finish(layouts[k]["inverse"], layouts[k]["col"], 2, 1000, layouts[k]["seed"], layouts[k]["saved"], layouts[k]["alive"],
                      layouts[k]["selected"])
        assert w.margins.undecidable == 0
        s = slice(int(c.node_ptr[k]), int(c.node_ptr[k + 1]))
        assert st.out.cpu().tolist()[k] == [w.rounds_run, 0] and np.array_equal(st.selected.cpu().numpy()[s], w.selected)
        assert np.array_equal(st.alive.cpu().numpy()[s], w.alive)
        np.testing.assert_allclose(st.saved.cpu().numpy()[s], w.saved, rtol=RTOL_SAVED, atol=0.0)


# ------------------------------------------------------------------------------------------------ compaction of K layouts
def compact_layouts(which):
    """Layouts with every array compaction touches (numpy): '300' = the K = 300 small ones, 'chunks' = node and edge counts at
    the 1024-item chunk edges."""
    rng = np.random.default_rng(911)
    if which == "300":
        sizes = [(int(rng.integers(1, 6)), 2 * int(rng.integers(0, 5)), 2 * int(rng.integers(0, 5))) for _ in range(300)]
    else:
        sizes = [(1023, 1024, 1025), (1024, 1025, 0), (1025, 0, 1024), (2300, 2048, 2049), (1, 0, 0), (700, 1023, 3000)]
    layouts = []
    for k, (n, ea, ec) in enumerate(sizes):
        def edges(e):
            if n < 2 or e == 0:
                return np.zeros((2, 0), dtype=np.int64)
            u = rng.integers(0, n, size=e)
            return np.stack([u, (u + rng.integers(1, n, size=e)) % n]).astype(np.int64)
        adj, col = edges(ea), edges(ec)
        alive = (rng.uniform(size=n) < 0.6).astype(np.int32)
        if k % 7 == 3:
            alive[:] = 0
        if k % 7 == 5:
            alive[:] = 1
        layouts.append(dict(x=rng.uniform(size=(n, 3)).astype(np.float32), adj=adj, attr=rng.uniform(size=(adj.shape[1], 2)).astype(np.float32),
                            col=col, alive=alive * (1 + k % 3), active=bool(rng.uniform() < 0.7) if which == "300" else k != 5))
    return layouts


@pytest.mark.parametrize("which", ["300", "chunks"])
def test_compact_many_is_the_restated_compaction_per_layout(which):
    from tilingnn_amd import _lib
    from tilingnn_amd._lib import check, lib, ptr
    layouts = compact_layouts(which)
    K = len(layouts)
    ptr_of = lambda sizes: np.concatenate([[0], np.cumsum(sizes)]).astype(np.int64)
    node_ptr, adj_ptr, col_ptr = (ptr_of([l["x"].shape[0] for l in layouts]), ptr_of([l["adj"].shape[1] for l in layouts]),
                                  ptr_of([l["col"].shape[1] for l in layouts]))
    n, ea, ec = int(node_ptr[-1]), int(adj_ptr[-1]), int(col_ptr[-1])
    x = _t(np.concatenate([l["x"] for l in layouts]))
    attr = _t(np.concatenate([l["attr"] for l in layouts]))
    adj = _t(np.concatenate([l["adj"].reshape(-1) for l in layouts]))
    col = _t(np.concatenate([l["col"].reshape(-1) for l in layouts]))
    alive = _t(np.concatenate([l["alive"] for l in layouts]).astype(np.int32))
    active = _t(np.array([int(l["active"]) for l in layouts], dtype=np.int32))
    x_out = torch.full((n + PAD, 3), float(S_OUT), device=DEV)
    inverse = torch.full((n + PAD,), S_OUT, dtype=torch.int64, device=DEV)
    adj_out = torch.full((2 * ea + PAD,), S_OUT, dtype=torch.int64, device=DEV)
    attr_out = torch.full((ea + PAD, 2), float(S_OUT), device=DEV)
    col_out = torch.full((2 * ec + PAD,), S_OUT, dtype=torch.int64, device=DEV)
    counts = torch.full((K, 3), S_OUT, dtype=torch.int64, device=DEV)
    err = torch.zeros(K, dtype=torch.int32, device=DEV)
    wsb = int(lib.tgnn_sublayout_compact_many_workspace_bytes(K, n, ea, ec))
    ws = torch.empty(wsb, dtype=torch.uint8, device=DEV)
    node_ptr_d, adj_ptr_d, col_ptr_d = _t(node_ptr), _t(adj_ptr), _t(col_ptr)
    check(lib.tgnn_sublayout_compact_many(K, ptr(active), ptr(node_ptr_d), ptr(adj_ptr_d), ptr(col_ptr_d), n, ea, ec, ptr(alive), ptr(x), 3,
                                          ptr(adj), ptr(attr), 2, ptr(col), ptr(x_out), ptr(inverse), ptr(adj_out), ptr(attr_out),
                                          ptr(col_out), ptr(counts), ptr(err), ptr(ws), wsb, _lib.current_stream(DEV)))
    torch.cuda.synchronize()
    assert err.cpu().tolist() == [0] * K
    x_o, inv_o, adj_o, attr_o, col_o, cnt = (t.cpu().numpy() for t in (x_out, inverse, adj_out, attr_out, col_out, counts))
    seen = set()
    for k, l in enumerate(layouts):
        n0, a0, c0 = int(node_ptr[k]), int(adj_ptr[k]), int(col_ptr[k])
        n1, a1, c1 = int(node_ptr[k + 1]), int(adj_ptr[k + 1]), int(col_ptr[k + 1])
        if not l["active"]:                                    # sits out: nothing of it is written
            n2 = e2 = f2 = 0
            assert cnt[k].tolist() == [S_OUT] * 3, k
        else:
            x2, adj2, attr2, col2, inv2 = gr.compact(l["alive"], l["adj"], l["attr"], l["col"], l["x"])
            n2, e2, f2 = len(inv2), adj2.shape[1], col2.shape[1]
            assert cnt[k].tolist() == [n2, e2, f2], k
            assert np.array_equal(inv_o[n0:n0 + n2], inv2) and np.array_equal(x_o[n0:n0 + n2], x2), k
            assert np.array_equal(adj_o[2 * a0:2 * a0 + 2 * e2].reshape(2, e2), adj2) and np.array_equal(attr_o[a0:a0 + e2], attr2), k
            assert np.array_equal(col_o[2 * c0:2 * c0 + 2 * f2].reshape(2, f2), col2), k
            seen.add((n2 > 0, e2 > 0, f2 > 0))
        assert (inv_o[n0 + n2:n1] == S_OUT).all() and (x_o[n0 + n2:n1] == S_OUT).all(), k
        assert (adj_o[2 * a0 + 2 * e2:2 * a1] == S_OUT).all() and (attr_o[a0 + e2:a1] == S_OUT).all(), k
        assert (col_o[2 * c0 + 2 * f2:2 * c1] == S_OUT).all(), k
    assert (inv_o[n:] == S_OUT).all() and (adj_o[2 * ea:] == S_OUT).all() and (col_o[2 * ec:] == S_OUT).all()
    assert (True, True, True) in seen and (False, False, False) in seen
