"""The conditions the NNConv op tests (tests/test_nnconv32_ops.py) rest on, checked on the CPU: every kernel of the width-32
NNConv is reached by some case and every case lands on the kernel it names (tests/nnconv_cases.py: dispatch); the type-count
boundaries fall where the table says; `graph` has the row classes it promises, with their exact in-degrees; the fp64 oracle
evaluated in fp32 by torch passes both gates (a correct fp32 implementation stands inside the bounds); three perturbed copies fail
the element-wise gate; the reference is the pinned oracle's."""
import pytest
import torch

from oracle import tilingnn_oracle as orc
from tests import nnconv_cases as nc


def test_every_kernel_is_reached_and_every_case_lands_on_its_kernel():
    reached = set()
    for case in nc.CASES:
        g = nc.graph(case.n, case.T, case.n + case.T)
        name, fast, blocks = nc.dispatch(case.c, case.n, case.T, case.ldh, int(g.deg.max()), case.form)
        assert name == case.kernel, case
        if name == "refused":
            continue
        assert fast == case.fast, case
        assert 1 <= blocks <= nc.MAX_PARTIALS, case
        reached.add((name, fast))
    want = {(k, f) for k in nc.KERNELS for f in nc.FAST.get(k, (None,))}
    assert reached == want, (want - reached, reached - want)
    # the fp16-pair instantiation with FAST = false exists and cannot be launched: its entry point takes packed rows only
    assert nc.dispatch(32, 65, 13, 36, 5, "cols_f16")[0] == "refused" and nc.dispatch(32, 65, 13, 36, 5, "eg")[0] == "refused"


def test_block_counts_the_row_counts_are_there_for():
    tiled16 = {1: 1, 15: 1, 16: 1, 17: 1, 64: 1, 65: 2, 129: 3, 513: 8, 1254: 16, 4099: 64, 14337: 224, 28673: 224, 66003: 224}
    assert set(tiled16) == set(nc.ROW_COUNTS)
    assert {n: nc.tiled_blocks(n, 1) for n in nc.ROW_COUNTS} == tiled16
    assert nc.tiled_blocks(14336, 1) == 224 and -(-(-(-14337 // 16)) // 4) == 225          # 896 tiles fill the cap, 897 pass it
    assert [nc.tiled_blocks(n, 2) for n in (14337, 28672, 28673, 66003)] == [224, 448, 448, 448]
    assert {n: nc.lds_blocks(n) for n in (1, 16, 17, 64, 65, 129, 513, 1254, 4099, 66003)} == {
        1: 1, 16: 1, 17: 2, 64: 4, 65: 5, 129: 8, 513: 32, 1254: 72, 4099: 256, 66003: 256}
    # tgnn_debug_set_block_caps at 2 000 rows (125 tiles, 32 blocks without a cap): 1, 7, 8, 9 -> 8; two blocks per CU below 11 types
    assert [nc.tiled_blocks(nc.CAP_ROWS, 1, cap) for cap in nc.BLOCK_CAPS] == [1, 7, 8, 8]
    assert [nc.tiled_blocks(nc.CAP_ROWS, 2, cap) for cap in nc.BLOCK_CAPS] == [2, 8, 16, 16]
    assert [nc.tiled_blocks(nc.CAP_ROWS, 1, cap, eg=True) for cap in nc.BLOCK_CAPS] == [1, 7, 8, 8]
    assert nc.tiled_blocks(nc.CAP_ROWS) == 32
    # the generic kernel: 256 // c rows per block, at most 512 blocks
    assert [nc.dispatch(c, 1254, 13, c, 700, "csr")[2] for c in nc.GENERIC_WIDTHS] == [40, 251, 314, 512, 512]


def test_type_boundaries_fall_where_the_table_says():
    d = lambda T, kernel, deg=627: nc.dispatch(32, nc.TYPE_ROWS, T, 32, deg, kernel)[0]
    assert [d(T, "cols") for T in (0, 10, 11, 22, 23)] == [nc.COLS8, nc.COLS8, nc.COLS16, nc.COLS16, "refused"]
    assert [d(T, "cols_f16") for T in (1, 22, 23)] == [nc.COLS16F, nc.COLS16F, "refused"]
    assert [d(T, "eg") for T in (1, 22, 23)] == [nc.EG, nc.EG, "refused"]
    assert [d(T, "csr") for T in (0, 30, 31, 300)] == [nc.LDS, nc.LDS, nc.GENERIC, nc.GENERIC]
    assert d(0, "eg", 0) == "refused" and d(0, "cols_f16", 0) == "refused"
    assert [d(13, "eg", deg) for deg in (0, 1, 2048, 2049)] == ["refused", nc.EG, nc.EG, "refused"]
    assert nc.dispatch(48, 1254, 13, 48, 9, "cols")[0] == nc.dispatch(48, 1254, 13, 48, 9, "eg")[0] == "refused"
    assert nc.dispatch(32, 1254, 13, 32, 9, "columns")[0] == "refused"
    # kernel=None: groups first, then columns, then the CSR kernels
    assert nc.dispatch(32, 1254, 13, 32, 9, None, groups=True)[0] == nc.EG
    assert nc.dispatch(32, 1254, 13, 32, 2049, None, groups=True)[0] == nc.COLS16
    assert [nc.dispatch(32, 1254, T, 32, 9, None)[0] for T in (0, 10, 11, 22, 23, 31)] == [nc.COLS8, nc.COLS8, nc.COLS16, nc.COLS16, nc.LDS,
                                                                                          nc.GENERIC]
    assert nc.dispatch(64, 1254, 13, 64, 9, None)[0] == nc.GENERIC
    # the arithmetic behind the limits (csrc/nnconv_cols.hip, nnconv.hip)
    assert ((10 + 1) * 6144 + 8 * 1280) * 2 == 155648 <= 160 * 1024 < ((11 + 1) * 6144 + 8 * 1280) * 2 == 167936
    assert ((160 * 1024 - 256) // 4 - 16 * 320) // 1536 - 1 == nc.COLS_MAX_TYPES
    assert (nc.LDS_MAX_TYPES + 1) * 5120 <= 160 * 1024 - 256 < (nc.LDS_MAX_TYPES + 2) * 5120


GRAPHS = sorted({(c.n, c.T) for c in nc.CASES})


@pytest.mark.parametrize("n,T", GRAPHS)
def test_graph_has_the_row_classes_it_promises(n, T):
    g = nc.graph(n, T, n + T)
    again = nc.graph.__wrapped__(n, T, n + T)
    assert all(torch.equal(a, b) for a, b in zip((g.src, g.dst, g.typ, g.deg, g.attr), (again.src, again.dst, again.typ, again.deg, again.attr)))
    deg = torch.bincount(g.dst, minlength=n)
    assert torch.equal(deg, g.deg) and bool((g.dst[1:] >= g.dst[:-1]).all())
    assert int(g.src.numel()) == 0 or (0 <= int(g.src.min()) and int(g.src.max()) < g.n_src)
    if T == 0:
        assert g.src.numel() == 0 and g.T == 0
        return
    assert int(deg.max()) <= nc.EG_MAX_IN_DEGREE
    assert sorted(set(g.typ.tolist())) == list(range(T)), "every type is used"
    assert torch.equal(torch.unique(g.attr, dim=0).shape[0] * torch.ones(1), T * torch.ones(1))
    rows = g.rows
    edges = lambda v: [(int(s), int(t)) for s, t in zip(g.src[g.dst == v], g.typ[g.dst == v])]
    want = ["deg17"] if n == 1 else ["deg0_last"]
    if n >= 48:
        want += ["deg0_tile"] + [name for name, _ in nc._CLASSES if name != "from_halo"]
    assert set(want) <= set(rows), (want, rows)
    assert len(set(rows.values())) == len(rows), "one row per class"
    for name, v in rows.items():
        if name == "deg0_tile":
            assert v == 16 and int(deg[16:32].sum()) == 0
        elif name == "deg0_last":
            assert v == n - 1 and int(deg[v]) == 0
        elif name.startswith("deg"):
            assert int(deg[v]) == int(name[3:]), name
        elif name == "hub":
            assert int(deg[v]) == nc.hub_degree(n) and len({t for _, t in edges(v)}) == 1
            assert n < 64 or v == n - 3
        elif name == "distinct":
            assert int(deg[v]) == min(T, 12) == len({t for _, t in edges(v)})
        elif name == "dup":
            e = edges(v)
            assert len(e) == 3 and e[0] == e[1]
        elif name == "self":
            e = edges(v)
            assert e[0][0] == v and e[1][0] == v and (T == 1 or e[0][1] != e[1][1])
        elif name == "from_first":
            assert [s for s, _ in edges(v)] == [0] * 5
        elif name == "from_last":
            assert [s for s, _ in edges(v)] == [n - 1] * 5
    # below 17 types: a row with two in-edges of one type (the column kernel's pre-add) past nnconv32_lds_kernel's 15 pipelined items
    assert len({t for _, t in edges(rows["deg17"])}) == min(T, 17)


def test_halo_graph_reads_the_rows_behind_the_destinations():
    for n in (65, 1254):
        g = nc.graph(n, nc.OP_TYPES, n + nc.OP_TYPES, nc.HALO)
        assert g.n_src == n + nc.HALO and int(g.src.max()) >= n
        v = g.rows["from_halo"]
        assert bool((g.src[g.dst == v] >= n).all()) and int((g.dst == v).sum()) == 4
        assert len(set(g.src[g.src >= n].tolist())) >= nc.HALO // 2


HOST_CASES = sorted({(c.c, c.n, c.T) for c in nc.CASES if c.n <= 4099 and c.kernel != "refused"})


@pytest.mark.parametrize("c,n,T", HOST_CASES)
def test_fp32_torch_evaluation_passes_both_gates(c, n, T):
    """The oracle in fp32 (torch on the CPU) against the oracle in fp64, under the csr form's bound -- the smallest c0, no floor --
    with LeakyReLU and without, at every magnitude."""
    torch.set_num_threads(8)
    for magnitude in nc.MAGNITUDES if c == 32 else (1.0,):
        p = nc.problem(n, T, 0, c, magnitude)
        for leaky in (False, True):
            ref = nc.leaky_ref(p.ref) if leaky else p.ref
            got = nc.reference(p.g, p.op, leaky, torch.float32).y
            rel, ratio = nc.measure(got, ref, "csr")
            print(f"nnconv c {c} n {n} T {T} magnitude {magnitude:g} leaky {int(leaky)}: fp32 torch rel_max_err {rel:.3e}, error / bound {ratio:.3f}")
            assert nc.gate_failures(got, ref, "csr", p.g) == []


@pytest.mark.parametrize("root_scale", nc.ROOT_SCALES)
@pytest.mark.parametrize("table", nc.TABLES)
def test_fp32_torch_evaluation_at_the_root_scales_and_saturated_tables(root_scale, table):
    for magnitude in nc.MAGNITUDES:
        p = nc.problem(1254, nc.OP_TYPES, 0, 32, magnitude, root_scale, table)
        got = nc.reference(p.g, p.op, False, torch.float32).y
        assert nc.gate_failures(got, p.ref, "csr", p.g) == [], (magnitude, root_scale, table)
        for form in ("cols_f16", "eg"):                        # (the fp16 forms' bounds lie above it: c0 and the floor only add)
            assert bool((nc.bound(p.ref, form) >= nc.bound(p.ref, "csr")).all())


@pytest.mark.parametrize("n", [17, 1254])
def test_perturbed_copies_fail_the_element_wise_gate(n):
    p = nc.problem(n)
    g, v = p.g, p.g.rows["deg17"]
    first = int(torch.nonzero(g.dst == v)[0])
    keep = torch.ones(g.src.numel(), dtype=torch.bool)
    keep[first + 3] = False
    dropped = g._replace(src=g.src[keep], dst=g.dst[keep], typ=g.typ[keep])
    swapped_typ = g.typ.clone()
    swapped_typ[first + 3] = (swapped_typ[first + 3] + 1) % g.T
    swapped = g._replace(typ=swapped_typ)
    for name, got in (("one in-edge of the degree-17 row dropped", nc.reference(dropped, p.op).y),
                      ("one edge's type swapped", nc.reference(swapped, p.op).y)):
        for form in nc.FORMS:
            bad = nc.gate_failures(got.float(), p.ref, form, g)
            assert any(b.startswith("element-wise") for b in bad), (name, form)
            over = ~((got.float().double() - p.ref.y).abs() <= nc.bound(p.ref, form))
            assert torch.nonzero(over.any(1)).squeeze(1).tolist() == [v], (name, form)
            assert "deg17" in bad[-1]
    # the mean taken by deg + 1: every row with 1 .. 33 in-edges is off (at the hub's in-degree the bound of a dot product of
    # length 32 x 628 is as wide as the 1 / 628 the mean moves by: what such a row can show is left to the max-norm gate)
    d = p.ref.deg.double().unsqueeze(1)
    rootpart = p.op.h[:n].double() @ p.op.root.double() + p.op.bias.double()
    wrong = (p.ref.y - rootpart) * d.clamp(min=1) / (d + 1) + rootpart
    for form in nc.FORMS:
        bad = nc.gate_failures(wrong.float(), p.ref, form, g)
        assert any(b.startswith("element-wise") for b in bad), form
        over = ~((wrong.float().double() - p.ref.y).abs() <= nc.bound(p.ref, form))
        assert bool(over.any(1)[(p.ref.deg > 0) & (p.ref.deg <= 33)].all()) and not bool(over.any(1)[p.ref.deg == 0].any()), form
    # ... and a NaN fails both gates
    nan = p.ref.y.float().clone()
    nan[3, 5] = float("nan")
    assert len(nc.gate_failures(nan, p.ref, "csr", g)) == 2


def test_reference_is_the_pinned_oracle():
    """nnconv_cases.reference against oracle.nnconv_mean_dedup (the port of the reference's NNConv, pinned by
    tests/test_oracle_vs_reference_golden.py) on one small case, the table coming from the oracle's own edge MLP."""
    g = nc.graph(129, 5, 3)
    gen = torch.Generator().manual_seed(2)
    pre = "g"
    sd = {f"{pre}.mlp.mlp.0.linear.weight": torch.randn(32, 4, generator=gen) * 0.5, f"{pre}.mlp.mlp.0.linear.bias": torch.randn(32, generator=gen) * 0.1,
          f"{pre}.mlp.mlp.1.linear.weight": torch.randn(64, 32, generator=gen) * 0.2, f"{pre}.mlp.mlp.1.linear.bias": torch.randn(64, generator=gen) * 0.1,
          f"{pre}.mlp.mlp.2.linear.weight": torch.randn(1024, 64, generator=gen) * 0.2, f"{pre}.mlp.mlp.2.linear.bias": torch.randn(1024, generator=gen) * 0.1,
          f"{pre}.nnConv.root": torch.randn(32, 32, generator=gen) * 0.3, f"{pre}.nnConv.bias": torch.randn(32, generator=gen)}
    sd64 = orc.cast_sd(sd, torch.float64)
    h = torch.randn(129, 32, generator=gen)
    table = torch.stack([g.attr[torch.nonzero(g.typ == t)[0, 0]] for t in range(g.T)])
    with torch.no_grad():
        want = orc.nnconv_mean_dedup(h.double(), torch.stack([g.src, g.dst]), g.attr.double(), sd64, pre)
        wtab = orc.edge_weight_matrices(table.double(), sd64, f"{pre}.mlp", 32, 32)
    # (the table in fp64: Operands are cast by reference(); a float64 table passes through unchanged)
    ref = nc.reference(g, nc.Operands(h, wtab, sd[f"{pre}.nnConv.root"], sd[f"{pre}.nnConv.bias"]))
    assert orc.rel_max_err(ref.y, want) < 1e-13
    assert torch.equal(ref.deg, g.deg) and bool((ref.mag >= ref.y.abs() * (1 - 1e-12)).all())


def test_edge_mlp_cases():
    for T in nc.EW_TYPES:
        for fe in nc.EW_FE:
            table, attr, rep, sd = nc.edge_mlp_problem(T, fe, 32)
            assert torch.equal(attr[rep.long()], table), "the representative edge of type t carries row t"
            assert T < 3 or not bool((rep[1:] > rep[:-1]).all()), "representatives are not in type order"
            zeros, ones = nc.edge_mlp_saturation(table, sd)
            assert zeros >= 1 and ones >= 1, (T, fe, zeros, ones)
            # the oracle's edge MLP in fp32 (torch) stands inside the composed bound and the max-norm gate
            want, bnd = nc.edge_mlp_reference(table, sd, 32)
            with torch.no_grad():
                got = orc.edge_weight_matrices(table, sd, "g.mlp", 32, 32)
            assert orc.rel_max_err(got, want) < nc.REL_MAX_TOL and bool(((got.double() - want).abs() <= bnd).all()), (T, fe)
    assert [nc.edge_table_kernel(fe, 32) for fe in nc.EW_FE] == ["edge_weight_table_chunks_kernel"] * 4 + ["edge_weight_table_kernel"]
    assert nc.edge_table_kernel(4, 64) == "edge_weight_table_chunks_kernel" and nc.edge_table_kernel(4, 8) == "edge_weight_table_kernel"
    want, bnd = nc.edge_mlp_reference(*[nc.edge_mlp_problem(17, 4, 8)[i] for i in (0, 3)], 8)
    print(f"edge MLP bound at T 17, fe 4, c 8: median {float(bnd.median()):.2e}, max {float(bnd.max()):.2e}")
    assert want.shape == bnd.shape == (17, 8, 8) and bool((bnd > 0).all()) and float(bnd.max()) < 1e-3
