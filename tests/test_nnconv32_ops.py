"""NNConv at width 32 kernel by kernel against fp64 as an op (csrc/nnconv_cols.hip: nnconv32_cols_kernel in its 8-wave, 16-wave and
fp16-pair forms, FAST and not; csrc/nnconv_eg.hip: nnconv32_eg_kernel; csrc/nnconv.hip: nnconv32_lds_kernel, nnconv_generic_kernel,
the two edge_weight_table kernels).  Reference semantics: GraphConv.forward, graph_networks/layers/edge_conv.py:24-27 of the
reference -- restated in fp64 by tests/nnconv_cases.py: reference, pinned to the oracle by tests/test_nnconv_cases_host.py.

Every expectation, the graphs with their prescribed row classes, the dispatch and both gates (max-norm 2e-6 and the element-wise
bound with its derived c0 and fp16 floors) come from tests/nnconv_cases.py; that every case lands on the kernel it names is checked
on the CPU (tests/test_nnconv_cases_host.py).  Measured error / bound per form and case: profiles/nnconv32_ops_errors.txt."""
import ctypes as C
import types

import pytest
import torch

from oracle import tilingnn_oracle as orc
from tests import dense_oracle as do
from tests import nnconv_cases as nc

pytestmark = pytest.mark.gpu
SENTINEL = -7.0e4                     # a large finite value: what must not be read (padding) or written (guard rows, partial rows)


@pytest.fixture(scope="module")
def dev():
    if not torch.cuda.is_available():
        pytest.skip("needs a GPU")
    return torch.device("cuda:0")


_graphs = {}


def device_graph(g, dev, groups=False):
    """The prepared layout of nc.graph (once per process) and, per library type, the case's type it stands for: the library numbers
    the distinct attribute rows itself; its type t is matched through ONE edge that carries it (type_rep_edge)."""
    from tilingnn_amd import ops
    key = (g.n, g.T, g.n_src, int(g.deg.max()) if g.n else 0, groups)
    if key not in _graphs:
        adj = torch.stack([g.src, g.dst]).to(dev)
        pg = ops.prepare_graph(g.n, adj, g.attr.to(dev), torch.zeros(2, 0, dtype=torch.int64, device=dev), groups=groups,
                               n_src_nodes=g.n_src if g.n_src != g.n else None)
        assert pg.n_types == g.T and pg.max_in_degree == int(g.deg.max())
        cls = g.typ.to(dev)[pg.type_rep_edge[:g.T].long()]
        assert sorted(cls.tolist()) == list(range(g.T))
        _graphs[key] = (pg, cls)
    return _graphs[key]


def on_device(p, dev, form):
    pg, cls = device_graph(p.g, dev, groups=(form == "eg"))
    return pg, p.op.h.to(dev), p.op.wtab.to(dev)[cls].contiguous(), p.op.root.to(dev), p.op.bias.to(dev)


def new_part(c, dev):
    return torch.full((do.MAX_PARTIALS * 2 * c,), SENTINEL, dtype=torch.float64, device=dev)


def check_partials(part, npart, out, blocks, c=32):
    """The partial rows returned, summed in fp64, against fp64 sums of the fp32 values actually stored (dense_oracle.PARTIAL_RTOL);
    as many rows as the launch has blocks; the rows behind them untouched."""
    assert npart == blocks, (npart, blocks)
    rows = part[:npart * 2 * c].view(npart, 2 * c).cpu()
    ratio = do.partial_sum_ratio(rows, out.cpu())
    assert ratio <= 1.0, f"partial sums off by {ratio:.3g} x rtol {do.PARTIAL_RTOL:g}"
    assert bool((part[npart * 2 * c:] == SENTINEL).all()), "partial rows behind n_partials were written"
    return ratio


def run_and_gate(p, dev, form, leaky, what, degree_bound=None, blocks=None, debug_cap=0):
    """One call of ops.nnconv_mean(kernel=form) on problem p: finite, both gates, the partial rows; prints the measured figures."""
    from tilingnn_amd import ops
    pg, h, wtab, root, bias = on_device(p, dev, form)
    part = new_part(32, dev)
    out, npart = ops.nnconv_mean(h, pg, wtab, root, bias, ops.ACT_LEAKY_RELU if leaky else ops.ACT_NONE, part, kernel=form,
                                 **({"max_in_degree": degree_bound} if degree_bound else {}))
    ref = nc.leaky_ref(p.ref) if leaky else p.ref
    got = out.cpu()
    rel, ratio = nc.measure(got, ref, form, degree_bound)
    name, _, want_blocks = nc.dispatch(32, p.g.n, p.g.T, 32, degree_bound or int(p.g.deg.max()), form, debug_cap=debug_cap)
    print(f"nnconv32 {form:8s} {what}: {name}, {npart} blocks, rel_max_err {rel:.3e}, error / bound {ratio:.3f}")
    assert out.shape == (p.g.n, 32) and bool(torch.isfinite(out).all())
    bad = nc.gate_failures(got, ref, form, p.g, degree_bound)
    assert bad == [], f"{form} {what}: " + "; ".join(bad)
    check_partials(part, npart, out, want_blocks if blocks is None else blocks)
    return out, part, npart


# ---------------------------------------------------------------------------------------------- the forms as ops
ROW_CASES = [(f, n) for f in nc.FORMS for n in nc.ROW_COUNTS]
TYPE_CASES = [(f, T) for f in nc.FORMS for T in nc.TYPE_COUNTS]


@pytest.mark.parametrize("leaky", [False, True], ids=["none", "leaky"])
@pytest.mark.parametrize("form,n", ROW_CASES, ids=[f"{f}-{n}" for f, n in ROW_CASES])
def test_op_against_fp64(dev, form, n, leaky):
    """Every form at every row count of nc.ROW_COUNTS, 13 edge types, with LeakyReLU and without: both gates on every element,
    BatchNorm partial rows (their sums, their number = the launch's blocks, a sentinel behind them).  A failure names the row
    classes (nc.graph) of the rows over the bound."""
    run_and_gate(nc.problem(n), dev, form, leaky, f"rows {n} T {nc.OP_TYPES} leaky {int(leaky)}")


@pytest.mark.parametrize("form,T", TYPE_CASES, ids=[f"{f}-T{T}" for f, T in TYPE_CASES])
def test_op_against_fp64_type_counts(dev, form, T):
    """1 254 rows at the type counts where the dispatch changes (nc.TYPE_COUNTS): 0 (no adjacency edge: the CSR arrays are one
    allocated element each), 1, 10 | 11 (two 8-wave blocks per CU | one 16-wave block), 16 | 17, 22 | 23 (the last that fits the
    tiled kernels' LDS image | refused by them), 30 | 31 (LDS table | generic CSR kernel), 300.  Where the table says "refused",
    ValueError and nothing else."""
    from tilingnn_amd import ops
    p = nc.problem(nc.TYPE_ROWS, T)
    if nc.TYPE_COUNTS[T][form] == "refused":
        pg, h, wtab, root, bias = on_device(p, dev, "cols")
        with pytest.raises(ValueError, match="edge types|in-degree"):
            ops.nnconv_mean(h, pg, wtab, root, bias, ops.ACT_NONE, new_part(32, dev), kernel=form)
        return
    assert nc.dispatch(32, nc.TYPE_ROWS, T, 32, int(p.g.deg.max()), form)[0] == nc.TYPE_COUNTS[T][form]
    run_and_gate(p, dev, form, True, f"rows {nc.TYPE_ROWS} T {T} leaky 1")


MAG_CASES = [(f, n) for f in nc.FORMS for n in nc.MAGNITUDE_ROWS]


@pytest.mark.parametrize("form,n", MAG_CASES, ids=[f"{f}-{n}" for f, n in MAG_CASES])
def test_magnitudes_and_root_scales(dev, form, n):
    """Rows of magnitude 1e-3, 1, 1e3 (the bias with them) x root matrices scaled 2^-12, 0.3, 16 on every form -- the fp16 forms
    scale rows and weights by powers of two from max|h| and max|root| --, and the two saturated tables (every weight exactly 0.0,
    exactly 1.0f) at magnitude 1."""
    for magnitude in nc.MAGNITUDES:
        for root_scale in nc.ROOT_SCALES:
            run_and_gate(nc.problem(n, nc.OP_TYPES, 0, 32, magnitude, root_scale), dev, form, True,
                         f"rows {n} magnitude {magnitude:g} root x {root_scale:g}")
    for table in ("zeros", "ones"):
        for root_scale in (nc.ROOT_SCALES[0], nc.ROOT_SCALES[2]):
            run_and_gate(nc.problem(n, nc.OP_TYPES, 0, 32, 1.0, root_scale, table), dev, form, False, f"rows {n} table {table} root x {root_scale:g}")


@pytest.mark.parametrize("n", nc.MAGNITUDE_ROWS)
def test_cols_f16_and_the_in_degree_bound(dev, n):
    """The fp16-pair column kernel scales the summed rows by a power of two from the in-degree BOUND it is handed: the layout's own
    largest in-degree (the hub's), 4 x and 64 x that.  Both gates on every row, the hub row looked at by itself."""
    p = nc.problem(n)
    hub, d = p.g.rows["hub"], int(p.g.deg.max())
    assert int(p.g.deg[hub]) == d == nc.hub_degree(n)
    for k in (1, 4, 64):
        out, _, _ = run_and_gate(p, dev, "cols_f16", True, f"rows {n} in-degree bound {k} x {d}", degree_bound=k * d)
        ref = nc.leaky_ref(p.ref)
        e_hub = orc.rel_max_err(out[hub:hub + 1].cpu(), ref.y[hub:hub + 1])
        print(f"nnconv32 cols_f16 rows {n} bound {k} x {d}: hub row {e_hub:.3e} of its own max")
        assert e_hub < nc.REL_MAX_TOL


# ---------------------------------------------------------------------------------------------- through the C ABI: strides, guard rows
def raw_call(form, pg, h, ldh, wtab, root, bias, act, out, part, dev, n_src_rows=None):
    """The form's entry point on raw pointers -> (status, n_partials): ops.nnconv_mean's calls with h's stride and `out` free."""
    from tilingnn_amd._lib import lib, ptr
    n, T = pg.n_nodes, pg.n_types
    npart = C.c_int32(-1)
    rows = int(h.shape[0]) if n_src_rows is None else n_src_rows
    wimg = torch.empty(lib.tgnn_nnconv_weight_image_floats(T), dtype=torch.float32, device=dev)
    bounds = torch.empty(2, dtype=torch.int32, device=dev)
    if form == "csr":
        st = lib.tgnn_nnconv_mean_fwd(ptr(h), ldh, ptr(pg.adj_rowptr), ptr(pg.adj_src), ptr(pg.adj_type), ptr(wtab), T, ptr(root), ptr(bias), n, 32, act,
                                      ptr(out), ptr(part), C.byref(npart), None)
    elif form == "cols":
        t = pg.cols
        st = lib.tgnn_nnconv_mean_cols_fwd(ptr(h), ldh, ptr(t.tile_col_ptr), ptr(t.col_meta), ptr(t.col_src), ptr(wtab), T, ptr(root), ptr(bias), n, 32,
                                           act, ptr(out), ptr(wimg), ptr(part), C.byref(npart), None)
    elif form == "cols_f16":
        t = pg.cols
        st = lib.tgnn_nnconv_mean_cols_f16_fwd(ptr(h), ldh, rows, ptr(t.tile_col_ptr), ptr(t.col_meta), ptr(t.col_src), ptr(wtab), T, ptr(root),
                                               ptr(bias), n, pg.max_in_degree, act, ptr(out), ptr(wimg), ptr(bounds), ptr(part), C.byref(npart), None)
    else:
        t = pg.groups
        st = lib.tgnn_nnconv_mean_eg_fwd(ptr(h), ldh, rows, ptr(t.tile_grp_ptr), ptr(t.grp), ptr(wtab), T, ptr(root), ptr(bias), n, act, ptr(out),
                                         ptr(wimg), ptr(bounds), ptr(part), C.byref(npart), None)
    torch.cuda.synchronize()
    return st, npart.value


STRIDE_CASES = [(c.form, c.n, c.T, c.ldh) for c in nc.CASES if c.group == "strides"]


@pytest.mark.parametrize("form,n,T,ldh", STRIDE_CASES, ids=[f"{f}-{n}-T{T}-ldh{l}" for f, n, T, l in STRIDE_CASES])
def test_strided_rows(dev, form, n, T, ldh):
    """tgnn_nnconv_mean_cols_fwd and tgnn_nnconv_mean_fwd on rows 36 and 40 floats apart: a view of a wider buffer whose padding
    holds a large finite sentinel.  For the column kernel this is the only road to nnconv32_cols_kernel<.., FAST = false> (the
    masked gather: row * row_bytes), in its 8-wave (T = 10) and 16-wave (T = 13) shapes.  Both gates, the partial rows, and the
    packed call beside it: the column kernel's header says FAST is "same arithmetic, same bits", and that is asserted; the CSR
    kernels read the same values in the same order whatever the stride: the same bits too."""
    from tilingnn_amd import ops
    p = nc.problem(n, T)
    pg, h, wtab, root, bias = on_device(p, dev, form)
    name, fast, blocks = nc.dispatch(32, n, T, ldh, int(p.g.deg.max()), form)
    assert (name, fast) == next((c.kernel, c.fast) for c in nc.CASES if c.group == "strides" and (c.form, c.n, c.T, c.ldh) == (form, n, T, ldh))
    wide = torch.full((n, ldh), SENTINEL, device=dev)
    wide[:, :32] = h
    ref = nc.leaky_ref(p.ref)
    outs = []
    for rows, ld in ((wide, ldh), (h, 32)):
        out, part = torch.empty(n, 32, device=dev), new_part(32, dev)
        st, npart = raw_call(form, pg, rows, ld, wtab, root, bias, ops.ACT_LEAKY_RELU, out, part, dev)
        assert st == 0
        rel, ratio = nc.measure(out.cpu(), ref, form)
        print(f"nnconv32 {form:8s} rows {n} T {T} ldh {ld}: {name}, {npart} blocks, rel_max_err {rel:.3e}, error / bound {ratio:.3f}")
        bad = nc.gate_failures(out.cpu(), ref, form, p.g)
        assert bad == [], f"{form} ldh {ld}: " + "; ".join(bad)
        check_partials(part, npart, out, blocks)
        outs.append(out)
    differ = int((outs[0] != outs[1]).any(1).sum())
    print(f"nnconv32 {form:8s} rows {n} T {T}: ldh {ldh} against packed rows: {differ} rows differ")
    assert differ == 0


GUARD_CASES = [(f, n) for f in nc.FORMS for n in nc.GUARD_ROWS]


@pytest.mark.parametrize("form,n", GUARD_CASES, ids=[f"{f}-{n}" for f, n in GUARD_CASES])
def test_rows_behind_the_last_are_left_alone(dev, form, n):
    """`out` is the first n rows of an [n + 16, 32] buffer prefilled with a sentinel: the 16 rows behind -- the rest of the last
    tile and more -- keep it bit for bit; the n rows pass both gates."""
    from tilingnn_amd import ops
    p = nc.problem(n)
    pg, h, wtab, root, bias = on_device(p, dev, form)
    for act, ref in ((ops.ACT_NONE, p.ref), (ops.ACT_LEAKY_RELU, nc.leaky_ref(p.ref))):
        buf = torch.full((n + 16, 32), SENTINEL, device=dev)
        part = new_part(32, dev)
        st, npart = raw_call(form, pg, h, 32, wtab, root, bias, act, buf, part, dev)
        assert st == 0
        assert bool((buf[n:] == SENTINEL).all()), f"{form}: {int((buf[n:] != SENTINEL).any(1).sum())} guard rows written"
        bad = nc.gate_failures(buf[:n].cpu(), ref, form, p.g)
        assert bad == [], "; ".join(bad)
        check_partials(part, npart, buf[:n], nc.dispatch(32, n, nc.OP_TYPES, 32, int(p.g.deg.max()), form)[2])


@pytest.mark.parametrize("form", ["cols", "cols_f16", "csr"])
@pytest.mark.parametrize("n", [65, 1254])
def test_halo_rows(dev, form, n):
    """A shard's layout: 50 source rows behind the n destination rows (n_src_nodes > n), one row fed by halo rows alone.  (The
    edge-group kernel has this test in tests/test_nnconv_eg.py.)"""
    p = nc.problem(n, nc.OP_TYPES, nc.HALO)
    assert p.g.n_src == n + nc.HALO and "from_halo" in p.g.rows and p.op.h.shape[0] == n + nc.HALO
    run_and_gate(p, dev, form, True, f"rows {n} + {nc.HALO} halo rows")


@pytest.mark.parametrize("form", nc.FORMS)
@pytest.mark.parametrize("n", nc.REPEAT_ROWS)
def test_two_runs_give_the_same_bits(dev, form, n):
    """Output and partial rows: no atomics, no order that depends on timing, in any form."""
    p = nc.problem(n)
    a = run_and_gate(p, dev, form, True, f"rows {n} first run")
    b = run_and_gate(p, dev, form, True, f"rows {n} second run")
    assert a[2] == b[2] and torch.equal(a[0], b[0]) and torch.equal(a[1], b[1])


CAP_CASES = [(c.form, c.T) for c in nc.CASES if c.group == "caps"]


def test_block_caps(dev, debug_hooks):
    """tgnn_debug_set_block_caps of 1, 7, 8, 9 blocks on the tiled kernels (the column kernel in its three shapes, the groups) at
    2 000 rows: 125 tiles, a wave walks up to 8 tiles and the steady-state loop crosses tile boundaries; 7 | 8: without | with the
    XCD swizzle; 9 -> 8.  Both gates, the partial rows, the block count; the caps are restored whatever happens.  (One test for the
    four kernels: under the production library it runs once more in a process of its own, against the debug build.)"""
    if debug_hooks:
        return
    from tilingnn_amd._lib import lib
    for form, T in CAP_CASES:
        p = nc.problem(nc.CAP_ROWS, T)
        try:
            for cap in nc.BLOCK_CAPS:
                lib.tgnn_debug_set_block_caps(cap, 0)
                _, _, npart = run_and_gate(p, dev, form, True, f"rows {nc.CAP_ROWS} T {T} cap {cap}", debug_cap=cap)
                assert npart <= 2 * cap
        finally:
            lib.tgnn_debug_set_block_caps(0, 0)
        run_and_gate(p, dev, form, True, f"rows {nc.CAP_ROWS} T {T} no cap", blocks=nc.tiled_blocks(nc.CAP_ROWS, 2 if T <= 10 and form == "cols" else 1))


# ---------------------------------------------------------------------------------------------- refusals, kernel=None
def test_refusals(dev):
    """A named form runs or raises ValueError naming the limit; none falls back.  23 edge types under the tiled forms (the type-
    count test), in-degree 2 049 under "eg" -- with 2 048, the last it takes, inside both gates, the hub row by itself --, width 48
    under the tiled forms, an unknown name."""
    from tilingnn_amd import ops
    p = nc.problem(nc.TYPE_ROWS, nc.OP_TYPES, hub=2048)
    hub = p.g.rows["hub"]
    assert int(p.g.deg[hub]) == 2048 == int(p.g.deg.max())
    out, _, _ = run_and_gate(p, dev, "eg", False, "rows 1254 hub 2048")
    e_hub = orc.rel_max_err(out[hub:hub + 1].cpu(), p.ref.y[hub:hub + 1])
    print(f"nnconv32 eg hub row of 2048 in-edges: {e_hub:.3e} of its own max")
    assert e_hub < nc.REL_MAX_TOL
    q = nc.problem(nc.TYPE_ROWS, nc.OP_TYPES, hub=2049)
    pg, h, wtab, root, bias = on_device(q, dev, "eg")
    assert pg.max_in_degree == 2049 and pg.groups is not None
    with pytest.raises(ValueError, match="in-degrees 1 ... 2048"):
        ops.nnconv_mean(h, pg, wtab, root, bias, kernel="eg")
    # kernel=None on the same layout: the columns, as before (tests/test_nnconv_eg.py: in-degrees beyond the limit); inside the gates
    part = new_part(32, dev)
    out, npart = ops.nnconv_mean(h, pg, wtab, root, bias, ops.ACT_NONE, part)
    assert nc.gate_failures(out.cpu(), q.ref, "cols", q.g) == []
    check_partials(part, npart, out, nc.dispatch(32, nc.TYPE_ROWS, nc.OP_TYPES, 32, 2049, None, groups=True)[2])
    for name in ("columns", "f16", "lds", ""):
        with pytest.raises(ValueError, match="unknown NNConv kernel"):
            ops.nnconv_mean(h, pg, wtab, root, bias, kernel=name)
    # width 48
    g48 = nc.problem(5, nc.OP_TYPES, 0, 48)
    pg48, cls = device_graph(g48.g, dev)
    args = (g48.op.h.to(dev), pg48, g48.op.wtab.to(dev)[cls].contiguous(), g48.op.root.to(dev), g48.op.bias.to(dev))
    for form in ("cols", "cols_f16", "eg"):
        with pytest.raises(ValueError, match="width 32"):
            ops.nnconv_mean(*args, kernel=form)
    # "csr" is force_csr_kernel=True
    r = nc.problem(129)
    pg, h, wtab, root, bias = on_device(r, dev, "csr")
    assert torch.equal(ops.nnconv_mean(h, pg, wtab, root, bias, kernel="csr")[0], ops.nnconv_mean(h, pg, wtab, root, bias, force_csr_kernel=True)[0])


NONE_CASES = sorted({(c.n, c.T) for c in nc.CASES if c.group in ("rows", "types")})


@pytest.mark.parametrize("groups", [False, True], ids=["columns", "groups"])
def test_kernel_none_never_raises_and_lands_where_dispatch_says(dev, groups):
    """Every (rows, types) of the tables with kernel=None, on a layout prepared with columns and on one prepared with groups: no
    ValueError, the block count of the kernel `dispatch` names, the same bits as that kernel called by name."""
    from tilingnn_amd import ops
    by_name = {nc.COLS8: "cols", nc.COLS16: "cols", nc.EG: "eg", nc.LDS: "csr", nc.GENERIC: "csr"}
    for n, T in NONE_CASES:
        p = nc.problem(n, T)
        pg, cls = device_graph(p.g, dev, groups)
        h, wtab, root, bias = p.op.h.to(dev), p.op.wtab.to(dev)[cls].contiguous(), p.op.root.to(dev), p.op.bias.to(dev)
        name, _, blocks = nc.dispatch(32, n, T, 32, int(p.g.deg.max()) if T else 0, None, groups=groups and pg.groups is not None)
        part = new_part(32, dev)
        out, npart = ops.nnconv_mean(h, pg, wtab, root, bias, ops.ACT_LEAKY_RELU, part)
        form = by_name[name]
        bad = nc.gate_failures(out.cpu(), nc.leaky_ref(p.ref), form, p.g)
        assert bad == [], f"rows {n} T {T} -> {name}: " + "; ".join(bad)
        check_partials(part, npart, out, blocks)
        assert torch.equal(out, ops.nnconv_mean(h, pg, wtab, root, bias, ops.ACT_LEAKY_RELU, kernel=form)[0]), (n, T, name)


# ---------------------------------------------------------------------------------------------- the generic kernel at other widths
@pytest.mark.parametrize("n", nc.GENERIC_ROWS)
@pytest.mark.parametrize("c", nc.GENERIC_WIDTHS)
def test_csr_at_other_widths(dev, c, n):
    """nnconv_generic_kernel: c < 32 and widths that do not divide 256 (idle threads in a block), 64, and 256 (one row per block;
    3 types: the table is T x 256 KiB).  The gates with 32 replaced by c."""
    from tilingnn_amd import ops
    T = 3 if c == 256 else nc.OP_TYPES
    p = nc.problem(n, T, 0, c)
    pg, cls = device_graph(p.g, dev)
    name, _, blocks = nc.dispatch(c, n, T, c, int(p.g.deg.max()), "csr")
    assert name == nc.GENERIC
    args = (p.op.h.to(dev), pg, p.op.wtab.to(dev)[cls].contiguous(), p.op.root.to(dev), p.op.bias.to(dev))
    for leaky in (False, True):
        ref = nc.leaky_ref(p.ref) if leaky else p.ref
        part = new_part(c, dev)
        out, npart = ops.nnconv_mean(*args, ops.ACT_LEAKY_RELU if leaky else ops.ACT_NONE, part, kernel="csr")
        rel, ratio = nc.measure(out.cpu(), ref, "csr")
        print(f"nnconv generic c {c} rows {n} T {T} leaky {int(leaky)}: {npart} blocks, rel_max_err {rel:.3e}, error / bound {ratio:.3f}")
        assert out.shape == (n, c) and bool(torch.isfinite(out).all())
        bad = nc.gate_failures(out.cpu(), ref, "csr", p.g)
        assert bad == [], "; ".join(bad)
        check_partials(part, npart, out, blocks, c)
        assert torch.equal(out, ops.nnconv_mean(*args, ops.ACT_LEAKY_RELU if leaky else ops.ACT_NONE)[0])      # kernel=None: the same


# ---------------------------------------------------------------------------------------------- the edge MLP's table
EW_CASES = [(T, fe, c) for c in nc.EW_WIDTHS for T in nc.EW_TYPES for fe in nc.EW_FE]


@pytest.mark.parametrize("T,fe,c", EW_CASES, ids=[f"T{T}-fe{fe}-c{c}" for T, fe, c in EW_CASES])
def test_edge_weight_table(dev, T, fe, c):
    """ops.edge_weight_table (edge_weight_table_chunks_kernel: fe <= 64 and c c a multiple of 256, 16 types per pass;
    edge_weight_table_kernel: one block per type otherwise) against the fp64 edge MLP (oracle.edge_weight_matrices) on the distinct
    attribute rows, the representative edges NOT in type order, one attribute row driving sigmoids of layer 1 to exactly 0 and
    exactly 1.0f.  Gates: the max-norm gate, and dense_oracle's sigmoid bound composed over the three layers
    (nc.edge_mlp_reference) on every element."""
    from tilingnn_amd import ops
    table, attr, rep, sd = nc.edge_mlp_problem(T, fe, c)
    want, bnd = nc.edge_mlp_reference(table, sd, c)
    zeros, ones = nc.edge_mlp_saturation(table, sd)
    assert zeros >= 1 and ones >= 1
    graph = types.SimpleNamespace(n_types=T, type_rep_edge=rep.to(dev))
    mlp = [sd[f"g.mlp.mlp.{i}.linear.{k}"].to(dev) for i in range(3) for k in ("weight", "bias")]
    got = ops.edge_weight_table(attr.to(dev), graph, *mlp, c).cpu()
    assert got.shape == (T, c, c) and bool(torch.isfinite(got).all())
    err = (got.double() - want).abs()
    rel, ratio = orc.rel_max_err(got, want), float((err / bnd).max())
    print(f"edge table T {T} fe {fe} c {c}: {nc.edge_table_kernel(fe, c)}, rel_max_err {rel:.3e}, error / bound {ratio:.3f}, "
          f"{int((got == 1).sum())} entries 1.0f, {int((got == 0).sum())} entries 0.0f")
    assert rel < nc.REL_MAX_TOL
    assert ratio <= 1.0, f"{int((err > bnd).sum())} elements over the bound, worst {ratio:.3g} x"
    assert bool(((got > 0) | (want < 2.0 ** -126)).all()) and bool((got <= 1).all())
