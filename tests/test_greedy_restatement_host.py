"""The host restatement of the device greedy loop (tests/greedy_restatement.py) checked WITHOUT the library: the draw against
the Python big-integer formula, the vectorised round against a scalar loop, the structural facts the rule promises, the
compaction against oracle.greedy_oracle.compute_sub_layout (itself pinned to the reference's code by a golden file) -- and the
condition the GPU tests rest on: no case of their tables puts a decision within 1e-12 of flipping (see the module docstring of
the restatement).  The real-network replay of tests/test_greedy_solve_restated.py is the one case that cannot be checked here."""
import math

import numpy as np
import pytest

from tests import greedy_restatement as gr

M64 = (1 << 64) - 1


def big_int_uniform(seed, rnd, node):
    z = (seed + 0x9E3779B97F4A7C15 * (node + 1) + 0xD1B54A32D192ED03 * (rnd + 1)) & M64
    z = ((z ^ (z >> 30)) * 0xBF58476D1CE4E5B9) & M64
    z = ((z ^ (z >> 27)) * 0x94D049BB133111EB) & M64
    z ^= z >> 31
    return (z >> 11) / 9007199254740992.0


@pytest.mark.parametrize("seed", [0, 12345, 2 ** 63 + 5, 2 ** 64 - 1])
def test_uniform_is_the_big_integer_formula(seed):
    nodes = np.unique(np.concatenate([np.arange(300), 2 ** np.arange(21), 2 ** np.arange(1, 21) - 1,
                                      np.random.default_rng(1).integers(0, 2 ** 20 + 1, size=500)]))
    for rnd in (1, 2, 7, 40):
        got = gr.uniform(seed, rnd, nodes)
        want = np.array([big_int_uniform(seed, rnd, int(v)) for v in nodes])
        assert got.dtype == np.float64 and np.array_equal(got, want)
        assert (got >= 0).all() and (got < 1).all()
    assert np.array_equal(gr.uniform(seed - 2 ** 64, 3, nodes), gr.uniform(seed, 3, nodes))      # seeds are taken mod 2^64
    assert gr.uniform(seed, 3, 5).shape == (1,)
    assert 0.45 < gr.uniform(seed, 1, np.arange(1 << 16)).mean() < 0.55


def scalar_round(prob, inverse, col, rnd, seed, saved, alive, selected, n_sub):
    """round_step node by node and edge by edge, in Python floats and ints."""
    saved, alive, selected = list(saved), list(alive), list(selected)
    o = [int(inverse[i]) if inverse is not None else i for i in range(n_sub)]
    p = []
    for i in range(n_sub):
        pr = 1.0 if prob is None else float(prob[i])
        v = (saved[o[i]] ** (rnd - 1) * pr) ** (1.0 / rnd)
        saved[o[i]] = v
        p.append(v)
    edges = [] if col is None else [(int(col[0][e]), int(col[1][e])) for e in range(col.shape[1])]
    err = 0
    beaten = [False] * n_sub
    for u, v in edges:
        if not (0 <= u < n_sub and 0 <= v < n_sub):
            err = 1
            continue
        if u == v:
            continue
        if p[u] > p[v] or (p[u] == p[v] and u < v):
            beaten[v] = True
        else:
            beaten[u] = True
    accepted = [not beaten[i] and math.exp(p[i] - 1.0) > big_int_uniform(seed % (1 << 64), rnd, o[i]) for i in range(n_sub)]
    for i in range(n_sub):
        if accepted[i]:
            alive[o[i]] = 0
            selected[o[i]] = rnd
    for u, v in edges:
        if 0 <= u < n_sub and 0 <= v < n_sub and accepted[u]:
            alive[o[v]] = 0
    return saved, alive, selected, sum(accepted), err


def _small_case(seed):
    rng = np.random.default_rng(seed)
    n, n_orig = 40 + 13 * seed, 150
    inverse = np.sort(rng.choice(n_orig, size=n, replace=False)) if seed % 2 else None
    size = n_orig if inverse is not None else n
    saved = rng.uniform(0.2, 1.0, size=size)
    prob = rng.uniform(0.05, 1.0, size=n).astype(np.float32)
    prob[:6], saved[(inverse if inverse is not None else np.arange(n))[:6]] = 0.5, 0.7          # ties
    u = rng.integers(0, n, size=3 * n)
    v = rng.integers(0, n, size=3 * n)                        # (self loops among them)
    col = np.stack([np.concatenate([u, v, u[:9]]), np.concatenate([v, u, v[:9]])])
    col[:, rng.integers(0, col.shape[1], size=3)] = np.array([[-1, n, 2], [0, 1, n + 7]])
    return prob, inverse, col, saved, np.ones(size, dtype=np.int32), np.zeros(size, dtype=np.int32), n


@pytest.mark.parametrize("seed", [1, 2, 3])
def test_the_vectorised_round_is_the_scalar_loop(seed):
    prob, inverse, col, saved, alive, selected, n = _small_case(seed)
    for rnd, s in ((1, 0), (3, 12345), (7, 2 ** 64 - 1)):
        got = gr.round_step(prob, inverse, col, rnd, s, saved, alive, selected, n_sub=n)
        w_saved, w_alive, w_sel, w_acc, w_err = scalar_round(prob, inverse, col, rnd, s, saved, alive, selected, n)
        assert got.err == w_err == 1 and got.accepted == w_acc and 0 < w_acc < n
        assert np.array_equal(got.alive, w_alive) and np.array_equal(got.selected, w_sel)
        np.testing.assert_allclose(got.saved, w_saved, rtol=4e-16)         # (numpy's pow against Python's: an ulp)
        assert got.margins.undecidable == 0 and got.margins.calls == 1
    # probability 1 for every node, and the state passed in is not modified
    got = gr.round_step(None, inverse, col, 2, 5, saved, alive, selected, n_sub=n)
    w = scalar_round(None, inverse, col, 2, 5, saved, alive, selected, n)
    assert np.array_equal(got.alive, w[1]) and np.array_equal(got.selected, w[2]) and (alive == 1).all() and (selected == 0).all()


def _graph(n, seed, drop=None):
    from tilingnn_amd.synth import make_super_graph
    sg = make_super_graph(n, 8 * n, 10 * n, tile_count=2, n_edge_types=13, seed=seed)
    adj, col = sg.align_edge_index.astype(np.int64), sg.collide_edge_index.astype(np.int64)
    return sg, (adj[:, :0] if drop == "adj" else adj), (col[:, :0] if drop == "col" else col)


def test_structural_facts_of_a_round_and_of_a_solve():
    rng = np.random.default_rng(9)
    n = 900
    _, adj, col = _graph(n, 3)
    prob = rng.uniform(0.05, 1.0, size=n).astype(np.float32)
    prob[100:140] = 0.5
    r = gr.round_step(prob, None, col, 1, 4, np.ones(n), np.ones(n, dtype=np.int32), np.zeros(n, dtype=np.int32))
    acc = r.selected == 1
    u, v = col
    assert acc.sum() > 20 and not np.any(acc[u] & acc[v])                  # both-way storage: no two accepted nodes collide
    p = r.saved
    first = (p[u] > p[v]) | ((p[u] == p[v]) & (u < v))
    assert first[acc[u]].all()                                              # every accepted node precedes all its neighbours
    assert np.array_equal(r.alive == 0, acc | np.isin(np.arange(n), v[acc[u]]))
    table = rng.uniform(0.05, 1.0, size=(3, n)).astype(np.float32)
    for finish in (True, False):
        s = gr.solve(n, adj, col, lambda rnd, inv: table[rnd % 3][inv], 11, finish=finish)
        sel = s.selection > 0
        assert not np.any(sel[u] & sel[v])
        covered = sel.copy()
        covered[v[sel[u]]] = True
        assert covered.all()                                                # maximal
        assert sorted(s.order) == list(np.flatnonzero(sel)) and s.margins.undecidable == 0
    # one-way storage: within a round the two ends of a stored pair are still kept apart
    half = col[:, col[0] < col[1]]
    r = gr.round_step(prob, None, half, 1, 4, np.ones(n), np.ones(n, dtype=np.int32), np.zeros(n, dtype=np.int32))
    acc = r.selected == 1
    assert not np.any(acc[half[0]] & acc[half[1]])


@pytest.mark.parametrize("drop", [None, "adj", "col"])
def test_finishing_in_one_call_is_the_round_by_round_solve(drop):
    """The hand-over of the round number to `finish` and back (rounds += ran - 1) against the plain loop, which has none."""
    n = 1500
    _, adj, col = _graph(n, 5, drop)
    table = np.random.default_rng(2).uniform(0.05, 1.0, size=(3, n)).astype(np.float32)
    for seed in (0, -1, 2 ** 63 + 5):
        a = gr.solve(n, adj, col, lambda rnd, inv: table[rnd % 3][inv], seed, finish=True)
        b = gr.solve(n, adj, col, lambda rnd, inv: table[rnd % 3][inv], seed, finish=False)
        assert np.array_equal(a.selection, b.selection) and a.order == b.order and a.rounds == b.rounds
        assert a.rounds >= (1 if drop == "col" else 3)
    if drop == "col":                                         # (no collision: p = 1 in round 1, everybody is accepted at once)
        return
    for budget in (1, 2):                                     # a spent budget leaves the same nodes either way
        left = []
        for finish in (True, False):
            with pytest.raises(gr.BudgetExhausted) as exc:
                gr.solve(n, adj, col, lambda rnd, inv: table[rnd % 3][inv], 3, max_rounds=budget, finish=finish)
            left.append(exc.value.left)
        assert left[0] == left[1] > 0


def test_a_finish_skips_the_nodes_that_have_left():
    """Dead entry nodes and the edges at them take no part: the finish on the sub-layout WITH them equals the finish on the
    compacted sub-layout, node for node."""
    rng = np.random.default_rng(6)
    n = 700
    _, _, col = _graph(n, 8)
    alive = (rng.uniform(size=n) < 0.7).astype(np.int32)
    saved, selected = rng.uniform(0.2, 1.0, size=n), np.zeros(n, dtype=np.int32)
    a = gr.finish(None, col, 4, 1000, 9, saved, alive, selected, n_sub=n)
    _, _, _, col2, inverse = gr.compact(alive, None, None, col, None)
    b = gr.finish(inverse, col2, 4, 1000, 9, saved, alive, selected)
    assert a.rounds_run == b.rounds_run > 1 and a.left == b.left == 0 and a.accepted == b.accepted
    assert np.array_equal(a.alive, b.alive) and np.array_equal(a.selected, b.selected) and np.array_equal(a.saved, b.saved)
    assert np.array_equal(a.saved[alive == 0], saved[alive == 0])
    short = gr.finish(None, col, 4, 1, 9, saved, alive, selected, n_sub=n)
    assert short.rounds_run == 1 and short.left > 0


def test_compact_is_the_oracles_compute_sub_layout():
    from oracle import greedy_oracle as go
    rng = np.random.default_rng(4)
    sg, adj, col = _graph(500, 6)
    x, attr = sg.node_feature, sg.align_edge_features
    for frac in (0.0, 0.4, 1.0):
        alive = (rng.uniform(size=500) < frac).astype(np.int32) * 3
        x2, adj2, attr2, col2, inverse = gr.compact(alive, adj, attr, col, x)
        want = go.compute_sub_layout(x, adj, attr, col, np.zeros((col.shape[1], 1)), np.flatnonzero(alive))
        assert np.array_equal(x2, want[0]) and np.array_equal(adj2, want[1]) and np.array_equal(attr2, want[2])
        assert np.array_equal(col2, want[3]) and np.array_equal(inverse, want[5])
    assert gr.compact(np.ones(3), None, None, None, None)[1].shape == (2, 0)


# ------------------------------------------------------------------------------------------------ the GPU tests' inputs
def test_no_case_of_the_op_tests_is_undecidable_and_every_value_is_covered():
    from tests import test_greedy_ops as ops
    total = gr.Margins()
    for table, cases in ops.ALL_CASE_TABLES.items():
        m = gr.Margins()
        for c in cases():
            assert c.want().margins.undecidable == 0, (table, c.name, c.want().margins)
            m.add(c.want().margins)
        print(f"{table}: {m}")
        total.add(m)
    for table, cases in ops.MANY_CASE_TABLES.items():
        m = gr.Margins()
        for case, entry in cases():
            for k, w in enumerate(case.want(entry)):
                if w is not None:
                    assert w.margins.undecidable == 0, (table, case.name, entry, k, w.margins)
                    m.add(w.margins)
        print(f"{table}: {m}")
        total.add(m)
    assert total.undecidable == 0 and total.calls > 500
    # every value the issue lists meets the entry it is listed for
    rounds = [ops.round_case(k) for k in ops.ROUND_SPECS]
    assert {c.n for c in rounds} >= set(ops.ROUND_SIZES) | {1048653, 3000}
    for n in ops.ROUND_SIZES:
        mine = [c for c in rounds if c.n == n]
        assert {c.rnd for c in mine} == set(ops.ROUNDS) and {c.inverse is None for c in mine} == {True, False}
    for attr, values in (("seed", ops.SEEDS), ("ld", (1, 3)), ("variant", ops.VARIANTS), ("n_sel0", (0, 17))):
        assert {getattr(c, attr) for c in rounds} == set(values), attr
    assert max(c.col.shape[1] for c in rounds if c.col is not None) == 1048653
    assert any(c.variant == "oob" and c.want().err == 1 for c in rounds)
    finishes = [ops.finish_case(k) for k in ops.FINISH_SPECS]
    assert {(c.n, c.first_round) for c in finishes} == {(n, f) for n in ops.FINISH_SIZES for f in ops.FIRST_ROUNDS}
    assert {c.variant for c in finishes} == set(ops.FINISH_VARIANTS) and {c.dead_frac > 0 for c in finishes} == {True, False}
    assert all(c.want().left == 0 for c in finishes) and max(c.want().rounds_run for c in finishes) >= 5
    for k in ops.BUDGET_SPECS:
        c = ops.finish_case(k)
        assert c.want().left > 0 and c.want().rounds_run == c.max_rounds
    chunk = ops.many_chunk_case(3)
    assert [len(l["inverse"]) for l in chunk.layouts][:5] == [1, 1023, 1024, 1025, 2300]
    assert {0, 1024, 1025} <= {int(c) for c in chunk.counts[:, 2]}
    k300 = ops.many_300_case()
    active = [l["active"] for l in k300.layouts]
    assert k300.K == 300 and any(active[:256]) and not all(active[:256]) and any(active[256:]) and not all(active[256:])


def test_no_case_of_the_solve_tests_is_undecidable():
    from tests import test_greedy_solve_restated as sr
    total = gr.Margins()
    for name in sr.SOLVE_LAYOUTS:
        for seed in sr.SOLVE_SEEDS:
            a, b = sr.restated(name, seed, True), sr.restated(name, seed, False)
            assert a.margins.undecidable == 0 and b.margins.undecidable == 0, (name, seed, a.margins, b.margins)
            assert np.array_equal(a.selection, b.selection) and a.order == b.order and a.rounds == b.rounds
            total.add(a.margins).add(b.margins)
    assert sr.restated("n5000-no-adj", 0).rounds > sr.restated("n2000-no-adj", 0).rounds >= 3
    assert sr.restated("n2000-no-col", 0).rounds == 1 and sr.restated("n2000-no-col", 0).selection.all()
    for k, name in enumerate(sr.MANY_LAYOUTS):
        s = sr.restated(name, sr.MANY_SEEDS[k])
        assert s.margins.undecidable == 0, (name, s.margins)
        total.add(s.margins)
    for name, budget in sr.BUDGET_CASES:
        assert sr.restated(name, 7, True, budget).left > 0
    print(f"solves: {total}")
    assert total.undecidable == 0
