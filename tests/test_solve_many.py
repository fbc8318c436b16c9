"""K greedy solves in one loop (csrc/greedy_many.hip, tilingnn_amd.util.algorithms.solve_many_by_device_greedy,
ML_Solver.solve_many).  The batched loop is THE SAME COMPUTATION as K single-layout solves, so every comparison here is
equality (array_equal, ==), never a tolerance: the four `_many` entries against K calls of their single-layout
counterparts, the loop against `solve_by_device_greedy`, the scores against `ML_Solver.solve`."""
import ctypes as C
import os

import numpy as np
import pytest
import torch

from tests.test_device_greedy import _check_selection
from tests.test_hip_parity import make_net
from tests.test_union_area_gpu import CROP_KW, SIL, ring9  # noqa: F401  (ring9: the module-scoped fixture of the crop tests)

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda:0")
SENTINEL = -77


def _t(a, dt):
    return torch.from_numpy(np.ascontiguousarray(a)).to(dt).to(DEV)


def _synth(n, seed, adj=8, col=10):
    from tilingnn_amd.synth import make_super_graph
    from tilingnn_amd.util.algorithms import DeviceLayout
    sg = make_super_graph(n, adj * n, col * n, tile_count=2, n_edge_types=13, seed=seed)
    x, a, attr, c, _ = sg.to_torch(DEV)
    return DeviceLayout(x, a, attr, c)


def _five_layouts():
    """K = 5 of different sizes: ordinary, no collision edges, one node, ordinary (every node dead in the mask below), ordinary."""
    from tilingnn_amd.util.algorithms import DeviceLayout
    a, b, d, e = _synth(1500, 1), _synth(700, 2), _synth(2300, 3), _synth(40, 4, adj=4, col=4)
    b = DeviceLayout(b.node_feature, b.align_edge_index, b.align_edge_features, b.collide_edge_index[:, :0])
    one = DeviceLayout(torch.rand(1, 3, device=DEV), torch.zeros(2, 0, dtype=torch.int64, device=DEV),
                       torch.zeros(0, 15, device=DEV), torch.zeros(2, 0, dtype=torch.int64, device=DEV))
    return [a, b, one, d, e]


def _alive_masks(layouts, rng):
    masks = [(rng.uniform(size=int(l.node_feature.shape[0])) < 0.6).astype(np.int32) for l in layouts]
    masks[2][:] = 1
    masks[3][:] = 0                                              # every node dead
    return masks


class Packed:
    """The packed state the `_many` entries work on, and the calls."""

    def __init__(self, layouts):
        from tilingnn_amd._lib import lib
        from tilingnn_amd.util.algorithms import PackedLayouts
        self.pk = pk = PackedLayouts(layouts, DEV)
        K = self.K = pk.k
        self.x_out = torch.full((pk.n, pk.fx), float(SENTINEL), device=DEV)
        self.inverse = torch.full((pk.n,), SENTINEL, dtype=torch.int64, device=DEV)
        self.adj_out = torch.full((2 * max(pk.ea, 1),), SENTINEL, dtype=torch.int64, device=DEV)
        self.attr_out = torch.full((max(pk.ea, 1), pk.fe), float(SENTINEL), device=DEV)
        self.col_out = torch.full((2 * max(pk.ec, 1),), SENTINEL, dtype=torch.int64, device=DEV)
        self.counts = torch.full((K, 3), SENTINEL, dtype=torch.int64, device=DEV)
        self.err = torch.zeros(K, dtype=torch.int32, device=DEV)
        self.cws_bytes = int(lib.tgnn_sublayout_compact_many_workspace_bytes(K, pk.n, pk.ea, pk.ec))
        self.cws = torch.empty(self.cws_bytes, dtype=torch.uint8, device=DEV)

    def compact(self, alive, active=None, ws_bytes=None):
        from tilingnn_amd import _lib
        from tilingnn_amd._lib import lib, ptr
        pk = self.pk
        return lib.tgnn_sublayout_compact_many(
            self.K, ptr(active), ptr(pk.node_ptr), ptr(pk.adj_ptr), ptr(pk.col_ptr), pk.n, pk.ea, pk.ec, ptr(alive), ptr(pk.x), pk.fx,
            ptr(pk.adj), ptr(pk.attr), pk.fe, ptr(pk.col), ptr(self.x_out), ptr(self.inverse), ptr(self.adj_out), ptr(self.attr_out),
            ptr(self.col_out), ptr(self.counts), ptr(self.err), ptr(self.cws), self.cws_bytes if ws_bytes is None else ws_bytes,
            _lib.current_stream(DEV))

    def sub(self, k):
        n2, ea2, ec2 = (int(v) for v in self.counts[k].tolist())
        return self.pk.view(k, self.x_out, self.adj_out, self.attr_out, self.col_out, n2, ea2, ec2, self.inverse)


def _single_compact(layout, alive):
    """tgnn_sublayout_compact on one layout -> (counts, x, inverse, adj, attr, col) as numpy."""
    from tilingnn_amd.util.algorithms import SubLayoutBuilder
    sub = SubLayoutBuilder(layout).build(alive)
    return [t.cpu().numpy() for t in (sub.node_feature, sub.inverse_index, sub.align_edge_index, sub.align_edge_features,
                                      sub.collide_edge_index)]


# ------------------------------------------------------------------------------------------------ 1. the ABI, entry by entry
def test_compact_many_is_k_single_compactions():
    layouts = _five_layouts()
    rng = np.random.default_rng(0)
    masks = _alive_masks(layouts, rng)
    st = Packed(layouts)
    alive = _t(np.concatenate(masks), torch.int32)
    assert st.compact(alive) == 0
    torch.cuda.synchronize()
    assert st.err.cpu().tolist() == [0] * 5
    for k, (layout, mask) in enumerate(zip(layouts, masks)):
        sub = st.sub(k)
        got = [t.cpu().numpy() for t in (sub.node_feature, sub.inverse_index, sub.align_edge_index, sub.align_edge_features,
                                         sub.collide_edge_index)]
        if mask.any():
            want = _single_compact(layout, _t(mask, torch.int32))
            for g, w in zip(got, want):
                assert (g.size == 0 and w.size == 0) or (g.shape == w.shape and np.array_equal(g, w)), k
        else:
            assert all(g.size == 0 for g in got)
        assert np.array_equal(got[1], np.flatnonzero(mask))
    assert st.counts[3].cpu().tolist() == [0, 0, 0] and st.counts[2].cpu().tolist() == [1, 0, 0]
    # what lies behind a sub-layout inside its layout's part of the buffers was not written
    n0, n2 = st.pk.node_ptr_h[0], int(st.counts[0, 0])
    assert (st.inverse[n0 + n2:st.pk.node_ptr_h[1]] == SENTINEL).all()
    # inactive layouts are skipped: nothing of theirs is written
    st2 = Packed(layouts)
    active = _t(np.array([1, 0, 1, 0, 1]), torch.int32)
    assert st2.compact(alive, active) == 0
    torch.cuda.synchronize()
    for k in (1, 3):
        assert st2.counts[k].cpu().tolist() == [SENTINEL] * 3
        assert (st2.inverse[st2.pk.node_ptr_h[k]:st2.pk.node_ptr_h[k + 1]] == SENTINEL).all()
    for k in (0, 2, 4):
        assert torch.equal(st2.counts[k], st.counts[k]) and torch.equal(st2.sub(k).align_edge_index, st.sub(k).align_edge_index)


def test_round_many_and_finish_many_are_k_single_calls():
    from tilingnn_amd import _lib
    from tilingnn_amd._lib import check, lib, ptr
    layouts = _five_layouts()
    K = len(layouts)
    rng = np.random.default_rng(1)
    st = Packed(layouts)
    pk = st.pk
    seeds = [11, 2 ** 63 + 5, 0, 7, 12345]
    seeds_dev = torch.from_numpy(np.array(seeds, dtype=np.uint64).view(np.int64)).to(DEV)
    sizes = [pk.nodes(k) for k in range(K)]
    # state of the batched run (packed) and of the K single runs
    alive = torch.ones(pk.n, dtype=torch.int32, device=DEV)
    selected = torch.zeros(pk.n, dtype=torch.int32, device=DEV)
    saved = torch.ones(pk.n, dtype=torch.float64, device=DEV)
    n_sel = torch.zeros(K, dtype=torch.int64, device=DEV)
    err = torch.zeros(K, dtype=torch.int32, device=DEV)
    rws_bytes = int(lib.tgnn_greedy_round_many_workspace_bytes(K, pk.n))
    rws = torch.empty(rws_bytes, dtype=torch.uint8, device=DEV)
    solo = [dict(alive=torch.ones(n, dtype=torch.int32, device=DEV), selected=torch.zeros(n, dtype=torch.int32, device=DEV),
                 saved=torch.ones(n, dtype=torch.float64, device=DEV), tail=torch.zeros(2, dtype=torch.int64, device=DEV)) for n in sizes]
    from tilingnn_amd.util.algorithms import SubLayoutBuilder
    builders = [SubLayoutBuilder(l) for l in layouts]

    def compare():
        torch.cuda.synchronize()
        assert err.cpu().tolist() == [0] * K
        for k in range(K):
            sl = slice(pk.node_ptr_h[k], pk.node_ptr_h[k + 1])
            assert torch.equal(alive[sl], solo[k]["alive"]), k
            assert torch.equal(selected[sl], solo[k]["selected"]), k
            assert torch.equal(saved[sl], solo[k]["saved"]), k          # fp64, bit for bit
            assert int(n_sel[k]) == int(solo[k]["tail"][0]) and int(solo[k]["tail"][1]) == 0, k

    for rnd in (1, 2, 3):
        assert st.compact(alive) == 0
        torch.cuda.synchronize()
        counts = st.counts.cpu().numpy()
        probs = [_t(rng.uniform(0.05, 1.0, size=int(c[0])).astype(np.float32), torch.float32) if c[0] else None for c in counts]
        if probs[0] is not None and probs[0].numel() > 20:
            probs[0][:20] = 0.5                                           # ties
        table = torch.tensor([0 if (p is None or k == 1) else p.data_ptr() for k, p in enumerate(probs)], dtype=torch.int64).to(DEV)
        if probs[1] is not None:
            probs[1].fill_(1.0)                                           # layout 1's table entry is NULL = probability 1
        check(lib.tgnn_greedy_round_many(K, None, ptr(table), 1, ptr(pk.node_ptr), ptr(pk.col_ptr), pk.n, pk.ec, ptr(st.counts),
                                         ptr(st.inverse), ptr(st.col_out), rnd, ptr(seeds_dev), ptr(saved), ptr(alive), ptr(selected),
                                         ptr(n_sel), ptr(err), ptr(rws), rws_bytes, _lib.current_stream(DEV)))
        for k in range(K):
            s = solo[k]
            if not bool(s["alive"].any()):
                continue
            sub = builders[k].build(s["alive"])
            n2, ec2 = int(sub.node_feature.shape[0]), int(sub.collide_edge_index.shape[1])
            assert n2 == int(counts[k][0])
            wsb = int(lib.tgnn_greedy_round_workspace_bytes(n2))
            ws = torch.empty(wsb, dtype=torch.uint8, device=DEV)
            check(lib.tgnn_greedy_round(ptr(probs[k]), 1, ptr(sub.inverse_index), n2, ptr(sub.collide_edge_index) if ec2 else None, ec2,
                                        rnd, seeds[k], ptr(s["saved"]), ptr(s["alive"]), ptr(s["selected"]), ptr(s["tail"][:1]),
                                        ptr(s["tail"][1:].view(torch.int32)[:1]), ptr(ws), wsb, _lib.current_stream(DEV)))
        compare()
    # the finish: every layout that still has nodes and fits one block, in ONE launch, against tgnn_greedy_finish
    assert st.compact(alive) == 0
    torch.cuda.synchronize()
    counts = st.counts.cpu().numpy()
    fin_max = int(lib.tgnn_greedy_finish_max_nodes())
    words = [int(0 < c[0] <= fin_max) for c in counts]
    words[4] = 0                                                          # one of them left out on purpose: untouched
    assert sum(words) >= 2
    out = torch.full((K, 2), SENTINEL, dtype=torch.int32, device=DEV)
    check(lib.tgnn_greedy_finish_many(K, ptr(_t(np.array(words), torch.int32)), ptr(pk.node_ptr), ptr(pk.col_ptr), pk.n, pk.ec,
                                      ptr(st.counts), ptr(st.inverse), ptr(st.col_out), 4, 1000, ptr(seeds_dev), ptr(saved), ptr(alive),
                                      ptr(selected), ptr(n_sel), ptr(err), ptr(out), _lib.current_stream(DEV)))
    for k in range(K):
        if not words[k]:
            continue
        s = solo[k]
        sub = builders[k].build(s["alive"])
        n2, ec2 = int(sub.node_feature.shape[0]), int(sub.collide_edge_index.shape[1])
        one = torch.zeros(2, dtype=torch.int32, device=DEV)
        check(lib.tgnn_greedy_finish(ptr(sub.inverse_index), n2, ptr(sub.collide_edge_index) if ec2 else None, ec2, 4, 1000, seeds[k],
                                     ptr(s["saved"]), ptr(s["alive"]), ptr(s["selected"]), ptr(s["tail"][:1]),
                                     ptr(s["tail"][1:].view(torch.int32)[:1]), ptr(one), _lib.current_stream(DEV)))
        assert out[k].cpu().tolist() == one.cpu().tolist() and int(one[1]) == 0, k
    assert out[4].cpu().tolist() == [SENTINEL] * 2
    compare()


def test_score_sums_many_are_the_single_sums_bit_for_bit():
    from tilingnn_amd import _lib
    from tilingnn_amd._lib import check, lib, ptr
    layouts = _five_layouts() + [_synth(30000, 9, adj=40, col=2)]       # (the last one: more than one block per layout, 1.2M edges)
    K = len(layouts)
    st = Packed(layouts)
    pk = st.pk
    rng = np.random.default_rng(2)
    predict = (rng.uniform(size=pk.n) < 0.3).astype(np.float32)
    perim = rng.uniform(1.0, 9.0, size=pk.n).astype(np.float32)
    p_dev, per_dev = _t(predict, torch.float32), _t(perim, torch.float32)
    sums = torch.zeros(K, 3, dtype=torch.float64, device=DEV)
    wsb = int(lib.tgnn_solution_score_sums_many_workspace_bytes(K))
    ws = torch.empty(wsb, dtype=torch.uint8, device=DEV)
    check(lib.tgnn_solution_score_sums_many(K, None, ptr(pk.node_ptr), ptr(pk.adj_ptr), pk.n, pk.ea, ptr(p_dev),
                                            C.c_void_p(pk.x.data_ptr() + 4 * (pk.fx - 1)), pk.fx, ptr(per_dev), ptr(pk.adj),
                                            C.c_void_p(pk.attr.data_ptr() + 4), pk.fe, ptr(sums), ptr(ws), wsb, _lib.current_stream(DEV)))
    wsb1 = int(lib.tgnn_unsupervised_loss_workspace_bytes(1))
    ws1 = torch.empty(wsb1, dtype=torch.uint8, device=DEV)
    for k, l in enumerate(layouts):
        sl = slice(pk.node_ptr_h[k], pk.node_ptr_h[k + 1])
        n, ea = int(l.node_feature.shape[0]), int(l.align_edge_index.shape[1])
        x, attr, adj = l.node_feature.contiguous(), l.align_edge_features.contiguous(), l.align_edge_index.contiguous()
        pk_, perk = p_dev[sl].clone(), per_dev[sl].clone()
        one = torch.zeros(3, dtype=torch.float64, device=DEV)
        check(lib.tgnn_solution_score_sums(ptr(pk_), C.c_void_p(x.data_ptr() + 4 * 2), 3, ptr(perk), n, ptr(adj) if ea else None, ea,
                                           C.c_void_p(attr.data_ptr() + 4) if ea else None, 15, ptr(one), ptr(ws1), wsb1,
                                           _lib.current_stream(DEV)))
        assert torch.equal(sums[k].view(torch.int64), one.view(torch.int64)), (k, sums[k].tolist(), one.tolist())
    assert float(sums[5, 1]) != 0.0


# ------------------------------------------------------------------------------------------------ 2. / 3. the contract
def _solver(net, graph=None):
    from tilingnn_amd.solver.ml_solver.ml_solver import ML_Solver
    return ML_Solver(None, DEV, graph, net, num_prob_maps=1)


def _check_invariants(result, layout):
    sel, _, order = result
    n = int(layout.node_feature.shape[0])
    col = layout.collide_edge_index.cpu().numpy().reshape(2, -1)
    k = _check_selection(sel, col, n)
    assert len(order) == k and sorted(order) == list(np.flatnonzero(sel))


def _assert_contract(ms, layouts, seed):
    from tilingnn_amd.util import algorithms as alg
    got = alg.solve_many_by_device_greedy(ms, layouts, seed=seed)
    rounds = list(alg.solve_many_by_device_greedy.last_rounds)
    assert len(got) == len(layouts) == len(rounds)
    for k, layout in enumerate(layouts):
        sel, score, order = alg.solve_by_device_greedy(ms, layout, seed=seed)
        want_rounds = alg.solve_by_device_greedy.last_rounds
        print(f"layout {k} ({int(layout.node_feature.shape[0])} nodes, seed {seed}): {int(sel.sum())} tiles, {want_rounds} rounds "
              f"(batched: {int(got[k][0].sum())} tiles, {rounds[k]} rounds)")
        assert np.array_equal(got[k][0], sel), k
        assert got[k][2] == order, k
        assert rounds[k] == want_rounds, k
        assert got[k][1] == score, k                                       # (None == None for bare DeviceLayouts)
        _check_invariants(got[k], layout)
    return got, rounds


SIZES_A = (300, 520, 900, 1300, 1900, 2600, 3300, 4000)


@pytest.mark.parametrize("seed", [0, 7])
def test_eight_layouts_in_one_loop_are_their_single_solves(seed):
    layouts = [_synth(n, 20 + i) for i, n in enumerate(SIZES_A)]
    net, _ = make_net(DEV)
    _, rounds = _assert_contract(_solver(net), layouts, seed)
    assert len(set(rounds)) > 1, "sizes were chosen so that layouts leave the loop in different rounds"


def test_mid_size_layouts_join_the_loop():
    """6 000 and 20 000 nodes take the mid-size persistent forward; no other test pins that path's side-by-side bits to its solo
    bits, so that is asserted first.  Should it fail, the finding is reported and the batched solves are still held to the
    invariants that do not depend on the single-layout code."""
    from tilingnn_amd.util import algorithms as alg
    layouts = [_synth(n, 20 + i) for i, n in enumerate(SIZES_A)] + [_synth(6000, 40), _synth(20000, 41)]
    net, _ = make_net(DEV)
    mid = [(l.node_feature, l.align_edge_index, l.align_edge_features, l.collide_edge_index) for l in layouts[-2:]]
    solo = [net(x=l[0], adj_e_index=l[1], adj_e_features=l[2], col_e_idx=l[3])[0].clone() for l in mid]
    side = net.forward_many(mid)
    torch.cuda.synchronize()
    same = [bool(torch.equal(a, b)) for a, b in zip(solo, side)]
    print(f"mid-size forward_many == forward: {same}")
    if all(same):
        _assert_contract(_solver(net), layouts, 0)
    else:
        got = alg.solve_many_by_device_greedy(_solver(net), layouts, seed=0)
        for res, layout in zip(got, layouts):
            _check_invariants(res, layout)
        pytest.fail(f"the mid-size persistent forward is not bit-identical side by side and alone: {same}")


@pytest.fixture(scope="module")
def bunny_crops(ring9):  # noqa: F811
    from tilingnn_amd.tiling import tile_factory as tf
    from tilingnn_amd.util.shape_processor import load_polygons
    ext, holes = load_polygons(os.path.join(SIL, "bunny.txt"))
    crops = tf.crop_multiple_layouts_from_contour(ext, holes, ring9.graph, device=str(DEV), coverage=True, **CROP_KW)
    assert 12 <= len(crops) < 24
    return ring9.graph, [c[0] for c in crops]


def test_bunny_crops_solve_and_score_like_the_single_layout_path(bunny_crops):
    from tilingnn_amd.util import algorithms as alg
    graph, layouts = bunny_crops
    net, _ = make_net(DEV)
    ms = _solver(net, graph)
    ms.device_greedy_min_nodes = 0
    ms.device_greedy_seed = 5
    got = alg.solve_many_by_device_greedy(ms, layouts, seed=5)
    rounds = list(alg.solve_many_by_device_greedy.last_rounds)
    for k, layout in enumerate(layouts):
        out, score = ms.solve(layout)
        print(f"crop {k}: {int(layout.node_feature.shape[0])} nodes, score {score!r} (batched {got[k][1]!r}), "
              f"{alg.solve_by_device_greedy.last_rounds} rounds (batched {rounds[k]})")
        assert isinstance(got[k][1], float) and got[k][1] == score, k
        assert np.array_equal(got[k][0], out.predict) and got[k][2] == out.predict_order, k
        assert rounds[k] == alg.solve_by_device_greedy.last_rounds
        sel, _, order = got[k]
        col = np.asarray(layout.collide_edge_index).reshape(2, -1)
        assert len(order) == _check_selection(sel, col, int(layout.node_feature.shape[0]))


# ------------------------------------------------------------------------------------------------ 4. ML_Solver.solve_many
def test_ml_solver_solve_many(bunny_crops):
    import copy
    graph, layouts = bunny_crops
    layouts = layouts[:6]
    before = copy.deepcopy([(l.node_feature, l.align_edge_index, l.align_edge_features, l.collide_edge_index) for l in layouts])
    net, _ = make_net(DEV)
    ms = _solver(net, graph)
    assert ms.solve_many([]) == []
    outs = ms.solve_many(layouts, seed=3)
    assert len(outs) == len(layouts)
    for k, ((out, score), layout) in enumerate(zip(outs, layouts)):
        assert out is not layout and isinstance(score, float)
        assert np.array_equal(out.node_feature, layout.node_feature) and out.predict.shape == (layout.node_feature.shape[0],)
        want = ms.predict(layout)
        assert out.predict_probs.dtype == want.dtype and out.predict_probs.shape == want.shape
        assert np.array_equal(out.predict_probs.view(np.int32), want.view(np.int32)), k     # bitwise
        assert sorted(out.predict_order) == list(np.flatnonzero(out.predict))
        assert not hasattr(layout, "predict_order") or layout.predict_order is not out.predict_order
    for old, l in zip(before, layouts):
        for a, b in zip(old, (l.node_feature, l.align_edge_index, l.align_edge_features, l.collide_edge_index)):
            assert np.array_equal(a, b)
    # input order: solving the reversed list gives the reversed results
    rev = ms.solve_many(layouts[::-1], seed=3)
    for (a, sa), (b, sb) in zip(outs, rev[::-1]):
        assert np.array_equal(a.predict, b.predict) and sa == sb and a.predict_order == b.predict_order


# ------------------------------------------------------------------------------------------------ 5. errors are errors
def test_a_bad_edge_index_names_its_layout_and_writes_nothing_out_of_range():
    from tilingnn_amd.util import algorithms as alg
    from tilingnn_amd.util.algorithms import DeviceLayout
    layouts = [_synth(n, 50 + i) for i, n in enumerate((400, 300, 500, 350, 450))]
    bad_adj = layouts[3].align_edge_index.clone()
    bad_adj[1, 17] = 350                                                   # one past the last node of layout 3
    layouts[3] = DeviceLayout(layouts[3].node_feature, bad_adj, layouts[3].align_edge_features, layouts[3].collide_edge_index)
    st = Packed(layouts)
    alive = torch.ones(st.pk.n, dtype=torch.int32, device=DEV)
    assert st.compact(alive) == 0
    torch.cuda.synchronize()
    assert st.err.cpu().tolist() == [0, 0, 0, 1, 0]
    good = [_synth(n, 50 + i) for i, n in enumerate((400, 300, 500, 350, 450))]
    ref = Packed(good)
    assert ref.compact(alive) == 0
    torch.cuda.synchronize()
    for k in (0, 1, 2, 4):                                                 # the other layouts: exactly what they are without the bad one
        for a, b in zip((st.sub(k).node_feature, st.sub(k).align_edge_index, st.sub(k).collide_edge_index, st.sub(k).inverse_index),
                        (ref.sub(k).node_feature, ref.sub(k).align_edge_index, ref.sub(k).collide_edge_index, ref.sub(k).inverse_index)):
            assert torch.equal(a, b)
    # layout 3 lost the one bad edge and nothing else; behind its compacted edges the sentinel is intact
    assert st.counts[3].cpu().tolist() == [350, int(bad_adj.shape[1]) - 1, int(layouts[3].collide_edge_index.shape[1])]
    a0, a1 = st.pk.adj_ptr_h[3], st.pk.adj_ptr_h[4]
    assert (st.adj_out[2 * a1 - 2:2 * a1] == SENTINEL).all() and (st.attr_out[a1 - 1] == SENTINEL).all() and a1 - a0 == bad_adj.shape[1]
    net, _ = make_net(DEV)
    with pytest.raises(IndexError, match="3"):
        alg.solve_many_by_device_greedy(_solver(net), layouts, seed=0)


def test_bad_arguments_get_the_argument_status():
    from tilingnn_amd._lib import lib, ptr
    layouts = [_synth(300, 1), _synth(200, 2)]
    st = Packed(layouts)
    pk = st.pk
    alive = torch.ones(pk.n, dtype=torch.int32, device=DEV)
    assert st.compact(alive, ws_bytes=64) == -2 and b"workspace" in lib.tgnn_last_error()
    args = [ptr(pk.node_ptr), ptr(pk.adj_ptr), ptr(pk.col_ptr), pk.n, pk.ea, pk.ec, ptr(alive), ptr(pk.x), pk.fx, ptr(pk.adj), ptr(pk.attr),
            pk.fe, ptr(pk.col), ptr(st.x_out), ptr(st.inverse), ptr(st.adj_out), ptr(st.attr_out), ptr(st.col_out), ptr(st.counts),
            ptr(st.err), ptr(st.cws), st.cws_bytes, None]
    assert lib.tgnn_sublayout_compact_many(-1, None, *args) == -1
    assert lib.tgnn_sublayout_compact_many(2, None, None, *args[1:]) == -1 and b"offset table" in lib.tgnn_last_error()
    assert lib.tgnn_greedy_round_many(-1, None, None, 1, None, None, 0, 0, *([None] * 3), 1, *([None] * 7), 0, None) == -1
    assert lib.tgnn_greedy_round_many(2, None, ptr(alive), 1, None, None, pk.n, pk.ec, *([None] * 3), 1, *([None] * 7), 0, None) == -1
    assert lib.tgnn_greedy_finish_many(2, None, *([None] * 2), pk.n, pk.ec, *([None] * 3), 1, 1, *([None] * 7), None) == -1
    assert lib.tgnn_solution_score_sums_many(2, None, ptr(pk.node_ptr), ptr(pk.adj_ptr), pk.n, pk.ea, ptr(alive), ptr(alive), 3, ptr(alive),
                                             ptr(pk.adj), ptr(pk.attr), 15, ptr(st.counts), ptr(st.cws), 8, None) == -2
    assert lib.tgnn_solution_score_sums_many(-2, *([None] * 3), 0, 0, *([None] * 2), 1, *([None] * 3), 1, *([None] * 2), 0, None) == -1
    torch.cuda.synchronize()
    assert (st.counts == SENTINEL).all()                                   # nothing was launched


def test_max_rounds_and_empty_input():
    from tilingnn_amd.util import algorithms as alg
    net, _ = make_net(DEV)
    ms = _solver(net)
    assert alg.solve_many_by_device_greedy(ms, []) == [] and alg.solve_many_by_device_greedy.last_rounds == []
    with pytest.raises(RuntimeError, match="still unlabelled after 1 rounds"):
        alg.solve_many_by_device_greedy(ms, [_synth(3000, 3), _synth(500, 4)], seed=1, max_rounds=1)
    # per-layout seeds: layout k with seeds[k] is the single solve with that seed
    layouts = [_synth(600, 5), _synth(600, 5)]
    got = alg.solve_many_by_device_greedy(ms, layouts, seeds=[1, 2])
    for k, s in enumerate((1, 2)):
        sel, _, order = alg.solve_by_device_greedy(ms, layouts[k], seed=s)
        assert np.array_equal(got[k][0], sel) and got[k][2] == order
    assert not np.array_equal(got[0][0], got[1][0])
