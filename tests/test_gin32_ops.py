"""GINConv at width 32 kernel by kernel against the fp64 oracle (csrc/gin.hip: gin_aggregate_kernel<32>, gin32_mlp_kernel,
gin32_mlp16_kernel, gin32_fused_kernel, gin_generic_kernel; reference semantics: CollConv.forward, graph_networks/layers/
coll_conv.py:24-27 of the reference -- the oracle's gin_conv, LeakyReLU behind it).

* the three width-32 forms as ops (tgnn_gin32_fwd, ops.gin(kernel="bf16x3" | "f16" | "fused")) at the row counts of
  tests/gin_cases.py -- every block count where the tile share, the XCD swizzle or the BatchNorm fold changes shape --, with and
  without a folded BatchNorm record, magnitudes 1e-3 ... 1e3, BatchNorm partial rows, bit-repeatability; the forms against each other;
* the fp16-pair kernel's power-of-two weight scales; strides, halo rows and the misaligned route; the generic kernel at widths
  8 ... 256; the refusals of tgnn_gin32_fwd;
* the forward runs these ops: under each switch setting its collision buffers ARE the op of the matching form, and the BatchNorm
  record its GIN kernel folds in-kernel is the fp64 batch statistics of its rows (1, 2, 7, 8, 16 and 24 blocks); the default fused
  regime at 200 003 nodes; CollConv including its BatchNorm.
The conditions the cases rest on (no saturated layer, the fp32 floor below the gate) are checked on the CPU:
tests/test_gin_cases_host.py."""
import ctypes as C
import types

import pytest
import torch

from oracle import tilingnn_oracle as orc
from tests import gin_cases as gc

pytestmark = pytest.mark.gpu
GATE = gc.GATE
PREFIX = gc.PREFIX


@pytest.fixture(scope="module")
def dev():
    if not torch.cuda.is_available():
        pytest.skip("needs a GPU")
    return torch.device("cuda:0")


_graphs = {}


def col_graph(n, dev):
    """The collision CSR of gc.collision_edges(n, n) on the device (built once)."""
    from tilingnn_amd import ops
    if n not in _graphs:
        rowptr, src, _, _ = ops.build_csr(gc.collision_edges(n, n).to(dev), n, True)
        _graphs[n] = types.SimpleNamespace(n_nodes=n, col_rowptr=rowptr, col_src=src)
    return _graphs[n]


def worst_row(out, want, graph):
    w = int((out.cpu().double() - want).abs().max(1).values.argmax())
    return w, int(graph.col_rowptr[w + 1] - graph.col_rowptr[w])


def check_partials(part, npart, want, n, c):
    """BatchNorm partial rows [blocks][sum c | sum of squares c] in fp64: the tolerances of tests/test_gin64_mfma.py."""
    assert 1 <= npart <= 512
    p = part[:npart * 2 * c].view(npart, 2 * c).sum(0).cpu()
    assert torch.allclose(p[:c], want.sum(0), rtol=1e-6, atol=1e-6 * float(want.abs().max()) * n)
    assert torch.allclose(p[c:], (want * want).sum(0), rtol=1e-5, atol=1e-6 * float(want.abs().max()) ** 2 * n)


# ---------------------------------------------------------------------------------------------- the three forms as ops
OP_CASES = [(v, n) for v in gc.VARIANTS for n in gc.ROW_COUNTS] + [(2, n) for n in gc.FUSED_ONLY_ROW_COUNTS]


@pytest.mark.parametrize("variant,n", OP_CASES, ids=[f"{gc.VARIANTS[v]}-{n}" for v, n in OP_CASES])
def test_op_against_fp64(dev, variant, n):
    """Gate: 1e-6 of the largest output for every (BatchNorm record or none) x (magnitude 1e-3, 1, 1e3) x (LeakyReLU; none as
    well for the bf16 x 3 form, the only one that takes it).  The references are computed once per process (gc.problem).
    Measured on an MI355X: see profiles/gin32_ops_errors.txt."""
    from tilingnn_amd import ops
    kernel = gc.VARIANTS[variant]
    graph = col_graph(n, dev)
    assert gc.dispatch(32, n, 32, True, variant)[1] == gc.gin32_blocks(n)
    for with_stat in (False, True):
        for scale in gc.MAGNITUDES:
            p = gc.problem(n, 32, with_stat, scale)
            params = [t.to(dev) for t in gc.param_list(p.sd)]
            a = p.a.to(dev)
            stat = p.stat.to(dev) if with_stat else None
            for leaky in ((True, False) if variant == 0 else (True,)):
                want = orc.leaky_relu(p.want) if leaky else p.want
                act = ops.ACT_LEAKY_RELU if leaky else ops.ACT_NONE
                part = ops.new_partials(32, dev)
                out, npart = ops.gin(a, graph, *params, act=act, in_stat=stat, partials=part, kernel=kernel)
                err = orc.rel_max_err(out.cpu(), want)
                w, deg = worst_row(out, want, graph)
                print(f"gin32 {kernel} n {n} stat {int(with_stat)} scale {scale:g} leaky {int(leaky)}: rel_max_err {err:.3e} "
                      f"(fp32 torch {p.f32_err:.3e}; {npart} blocks; worst row {w}, in-degree {deg})")
                assert out.shape == (n, 32) and bool(torch.isfinite(out).all())
                assert err < GATE
                assert npart == gc.gin32_blocks(n)
                check_partials(part, npart, want, n, 32)
                # the same bits on a second call, output and partial rows
                part2 = ops.new_partials(32, dev)
                out2, npart2 = ops.gin(a, graph, *params, act=act, in_stat=stat, partials=part2, kernel=kernel)
                assert npart2 == npart and torch.equal(out, out2) and torch.equal(part[:npart * 64], part2[:npart * 64])


@pytest.mark.parametrize("n", sorted(gc.ROW_COUNTS))
def test_variants_against_each_other(dev, n):
    """The fused kernel claims the arithmetic of the two-launch bf16 x 3 form in the same order: the same bits, with and without a
    record.  ops.gin(kernel=None) at width 32 IS the bf16 x 3 form.  The fp16-pair kernel is another kernel (where a difference
    can show at all: a few rows may round alike)."""
    from tilingnn_amd import ops
    graph = col_graph(n, dev)
    for with_stat in (False, True):
        p = gc.problem(n, 32, with_stat, 1.0)
        params = [t.to(dev) for t in gc.param_list(p.sd)]
        a = p.a.to(dev)
        stat = p.stat.to(dev) if with_stat else None
        run = lambda kernel, act=ops.ACT_LEAKY_RELU: ops.gin(a, graph, *params, act=act, in_stat=stat, partials=ops.new_partials(32, dev),
                                                             kernel=kernel)
        o0, np0 = run("bf16x3")
        o1, np1 = run("f16")
        o2, np2 = run("fused")
        od, npd = run(None)
        assert torch.equal(o2, o0), f"fused != bf16x3 in {int((o2 != o0).any(1).sum())} rows (n {n}, record {with_stat})"
        assert torch.equal(od, o0) and np0 == np1 == np2 == npd
        assert torch.equal(run(None, ops.ACT_NONE)[0], run("bf16x3", ops.ACT_NONE)[0])
        if n >= 200:
            assert not torch.equal(o1, o0)


WS_CASES = [(v, n) for v in (0, 1) for n in gc.WEIGHT_SCALE_ROWS]


@pytest.mark.parametrize("variant,n", WS_CASES, ids=[f"{gc.VARIANTS[v]}-{n}" for v, n in WS_CASES])
def test_weight_scales(dev, variant, n):
    """The fp16-pair kernel scales its W2 / W3 images by powers of two from max |W2|, max |W3| (pow2_scale_for; 0 -> 1): weights
    2^-12 and 16 times the usual, and all-zero matrices; the bf16 x 3 kernel beside it.  Scaled down or zero: the gate of 1e-6
    (plain fp32 is within 3.9e-7).  Scaled up by 16, plain fp32 itself leaves 1e-6 (3e-7 ... 3.3e-6): the gate is
    max(1e-6, 4 x the error of the fp32 torch evaluation of the oracle on the same inputs) -- an fp16 pair carries 22 significand
    bits against fp32's 24."""
    from tilingnn_amd import ops
    kernel = gc.VARIANTS[variant]
    graph = col_graph(n, dev)
    for w2s, w3s in gc.WEIGHT_SCALES:
        p = gc.problem(n, 32, False, 1.0, w2s, w3s)
        params = [t.to(dev) for t in gc.param_list(p.sd)]
        part = ops.new_partials(32, dev)
        out, npart = ops.gin(p.a.to(dev), graph, *params, act=ops.ACT_LEAKY_RELU, partials=part, kernel=kernel)
        want = orc.leaky_relu(p.want)
        err = orc.rel_max_err(out.cpu(), want)
        gate = GATE if max(w2s, w3s) <= 1.0 else max(GATE, 4.0 * p.f32_err)
        print(f"gin32 {kernel} n {n} W2 x {w2s:g} W3 x {w3s:g}: rel_max_err {err:.3e} (fp32 torch {p.f32_err:.3e}, gate {gate:.2e})")
        assert bool(torch.isfinite(out).all())
        assert err < gate
        check_partials(part, npart, want, n, 32)


# ---------------------------------------------------------------------------------------------- strides, halo rows, misalignment
def _gin_fwd_raw(a, lda, graph, params, n, act, dev, stat=None):
    """tgnn_gin_fwd at width 32 on a raw pointer / stride -> (out, partial rows, blocks)."""
    from tilingnn_amd import ops
    from tilingnn_amd._lib import check, lib, ptr
    out = torch.empty(n, 32, device=dev)
    z = torch.empty(n, 32, device=dev)
    part = ops.new_partials(32, dev)
    npart = C.c_int32(0)
    check(lib.tgnn_gin_fwd(ptr(a), lda, ptr(stat), ptr(graph.col_rowptr), ptr(graph.col_src), *[ptr(t) for t in params], n, 32, act,
                           ptr(out), ptr(z), ptr(part), C.byref(npart), None))
    torch.cuda.synchronize()
    return out, part, npart.value


@pytest.mark.parametrize("n", [37, 1254])
def test_strides_and_the_misaligned_route(dev, n):
    """Rows 36 floats apart stay on the matrix cores (the same bits as packed rows); rows 33 floats apart and rows that start one
    float past a 16-byte boundary take the generic kernel at width 32.  All against fp64 at 1e-6, with a record and without;
    tgnn_gin_aggregate on the strided rows against the fp64 neighbourhood sum."""
    from tilingnn_amd import ops
    from tilingnn_amd._lib import check, lib, ptr
    graph = col_graph(n, dev)
    for with_stat in (False, True):
        p = gc.problem(n, 32, with_stat, 1.0)
        params = [t.to(dev) for t in gc.param_list(p.sd)]
        stat = p.stat.to(dev) if with_stat else None
        want = orc.leaky_relu(p.want)
        a = p.a.to(dev)
        packed, _, np_packed = _gin_fwd_raw(a, 32, graph, params, n, ops.ACT_LEAKY_RELU, dev, stat)
        assert np_packed == gc.dispatch(32, n, 32, True, None)[1]
        for lda, offset in ((36, 0), (33, 0), (32, 1)):
            buf = torch.full((n * lda + 8,), 7.0e4, device=dev)          # (what lies between the rows must not be read)
            rows = buf[offset:offset + n * lda].view(n, lda)
            rows[:, :32] = a
            assert rows.data_ptr() % 16 == 4 * offset
            kernels, blocks = gc.dispatch(32, n, lda, offset == 0, None)
            out, part, npart = _gin_fwd_raw(rows, lda, graph, params, n, ops.ACT_LEAKY_RELU, dev, stat)
            err = orc.rel_max_err(out.cpu(), want)
            print(f"gin32 lda {lda} offset {offset} n {n} stat {int(with_stat)}: {kernels[-1]}, rel_max_err {err:.3e}, {npart} blocks")
            assert npart == blocks
            assert err < GATE
            check_partials(part, npart, want, n, 32)
            if lda == 36:
                assert torch.equal(out, packed)
        # the aggregate alone on rows 36 floats apart
        buf = torch.full((n, 36), 7.0e4, device=dev)
        buf[:, :32] = a
        z = torch.empty(n, 32, device=dev)
        check(lib.tgnn_gin_aggregate(ptr(buf), 36, ptr(stat), ptr(graph.col_rowptr), ptr(graph.col_src), ptr(params[0]), n, 32, ptr(z), None))
        x64 = gc.apply_record(p.a, p.stat, torch.float64) if with_stat else p.a.double()
        keep = p.ei[0] != p.ei[1]
        z64 = 1.25 * x64 + torch.zeros_like(x64).index_add_(0, p.ei[1][keep], x64[p.ei[0][keep]])
        assert orc.rel_max_err(z.cpu(), z64) < GATE


@pytest.mark.parametrize("n", [37, 1254])
def test_halo_rows(dev, n):
    """50 source rows behind the n destination rows (what a shard of the sharded forward reads): 3 n edges from anywhere among the
    n + 50 rows, every halo row used; the op and the aggregate alone against fp64."""
    from tilingnn_amd import ops
    from tilingnn_amd._lib import check, lib, ptr
    halo = 50
    g = torch.Generator().manual_seed(n + 7)
    src = torch.cat([torch.randint(0, n + halo, (3 * n,), generator=g), torch.arange(n, n + halo)])
    dst = torch.randint(0, n, (3 * n + halo,), generator=g)
    ei = torch.stack([src, dst])
    rowptr, col_src, _, err_flag = ops.build_csr(ei.to(dev), n, True, n_src_nodes=n + halo)
    assert int(err_flag) == 0
    graph = types.SimpleNamespace(n_nodes=n, col_rowptr=rowptr, col_src=col_src)
    a = torch.randn(n + halo, 32, generator=g)
    sd = gc.gin_weights(ei, n, n + 1, 32)
    with torch.no_grad():
        want = orc.leaky_relu(orc.gin_conv(a.double(), ei, orc.cast_sd(sd, torch.float64), PREFIX))[:n]
    params = [t.to(dev) for t in gc.param_list(sd)]
    part = ops.new_partials(32, dev)
    out, npart = ops.gin(a.to(dev), graph, *params, act=ops.ACT_LEAKY_RELU, partials=part)
    err = orc.rel_max_err(out.cpu(), want)
    print(f"gin32 halo n {n} + {halo}: rel_max_err {err:.3e}")
    assert out.shape == (n, 32) and err < GATE
    check_partials(part, npart, want, n, 32)
    for kernel in gc.VARIANTS.values():
        assert orc.rel_max_err(ops.gin(a.to(dev), graph, *params, act=ops.ACT_LEAKY_RELU, kernel=kernel)[0].cpu(), want) < GATE
    z = torch.empty(n, 32, device=dev)
    check(lib.tgnn_gin_aggregate(ptr(a.to(dev)), 32, None, ptr(rowptr), ptr(col_src), ptr(params[0]), n, 32, ptr(z), None))
    keep = src != dst
    x64 = a.double()
    z64 = (1.25 * x64 + torch.zeros_like(x64).index_add_(0, dst[keep], x64[src[keep]]))[:n]
    assert orc.rel_max_err(z.cpu(), z64) < GATE


# ---------------------------------------------------------------------------------------------- the generic kernel
@pytest.mark.parametrize("n", gc.GENERIC_ROWS)
@pytest.mark.parametrize("c", gc.GENERIC_WIDTHS)
def test_generic_widths(dev, c, n):
    """gin_generic_kernel: c < 64 (idle lanes in the aggregate and output loops), 64, between, and 256 (the limit of its LDS
    rows), with and without a record, LeakyReLU and none; the gate of the width-32 kernels."""
    from tilingnn_amd import ops
    graph = col_graph(n, dev)
    assert gc.dispatch(c, n, c, True, None)[0] == (gc.GENERIC,)
    for with_stat in (False, True):
        p = gc.problem(n, c, with_stat, 1.0)
        params = [t.to(dev) for t in gc.param_list(p.sd)]
        stat = p.stat.to(dev) if with_stat else None
        for leaky in (True, False):
            want = orc.leaky_relu(p.want) if leaky else p.want
            part = ops.new_partials(c, dev)
            out, npart = ops.gin(p.a.to(dev), graph, *params, act=ops.ACT_LEAKY_RELU if leaky else ops.ACT_NONE, in_stat=stat,
                                 partials=part)
            err = orc.rel_max_err(out.cpu(), want)
            print(f"gin generic c {c} n {n} stat {int(with_stat)} leaky {int(leaky)}: rel_max_err {err:.3e} (fp32 torch {p.f32_err:.3e})")
            assert out.shape == (n, c) and bool(torch.isfinite(out).all())
            assert npart == gc.dispatch(c, n, c, True, None)[1]
            assert err < GATE
            check_partials(part, npart, want, n, c)


# ---------------------------------------------------------------------------------------------- refusals
def test_refusals_and_the_empty_layout(dev):
    """Everything tgnn_gin32_fwd refuses comes back as TGNN_ERR_UNSUPPORTED with a message, launches nothing (`out` keeps its
    sentinel, the block count its value) and never falls back to the generic kernel."""
    from tilingnn_amd import ops
    from tilingnn_amd._lib import lib, ptr
    n = 37
    graph = col_graph(n, dev)
    p = gc.problem(n, 32, False, 1.0)
    params = [t.to(dev) for t in gc.param_list(p.sd)]
    a = p.a.to(dev)
    sentinel = -123.0
    out = torch.full((n * 32 + 4,), sentinel, device=dev)
    z = torch.empty(n * 32 + 4, device=dev)
    a_wide = torch.zeros(n * 36 + 4, device=dev)
    npart = C.c_int32(7)
    L, NONE = ops.ACT_LEAKY_RELU, ops.ACT_NONE

    def call(variant, a_=a, lda=32, c=32, act=L, out_=out, z_=z, rows=n):
        return lib.tgnn_gin32_fwd(ptr(a_), lda, None, ptr(graph.col_rowptr), ptr(graph.col_src), *[ptr(t) for t in params], rows, c, act,
                                  variant, ptr(out_), ptr(z_), None, C.byref(npart), None)

    for v in (0, 1, 2):
        assert call(v, c=64, lda=64) == -4 and b"width 32" in lib.tgnn_last_error(), v
        assert call(v, c=8) == -4, v
        assert call(v, a_=a_wide, lda=33) == -4 and b"aligned" in lib.tgnn_last_error(), v       # lda no multiple of 4
        assert call(v, a_=a_wide[1:]) == -4 and b"aligned" in lib.tgnn_last_error(), v           # a 4 bytes off
        assert call(v, out_=out[1:]) == -4 and b"aligned" in lib.tgnn_last_error(), v
        assert call(v, rows=2 ** 24) == -4 and b"2 GB" in lib.tgnn_last_error(), v               # n * 128 >= 2^31 (nothing is read)
    for v in (0, 1):
        assert call(v, z_=z[1:]) == -4 and b"aligned" in lib.tgnn_last_error(), v
    for v in (1, 2):
        assert call(v, act=NONE) == -4 and b"LeakyReLU" in lib.tgnn_last_error(), v
        assert call(v, a_=a_wide, lda=36) == -4 and b"packed" in lib.tgnn_last_error(), v
    assert call(3) == -1 and call(-1) == -1                                                  # no such variant
    assert call(0, a_=a_wide, lda=16) == -1 and b"lda" in lib.tgnn_last_error()              # rows shorter than the width
    torch.cuda.synchronize()
    assert npart.value == 7 and bool((out == sentinel).all())                                # (nothing ran)
    for v in (0, 1, 2):
        npart.value = 7
        assert call(v, rows=0) == 0 and npart.value == 0                                     # no rows: OK, 0 partial rows
    torch.cuda.synchronize()
    assert bool((out == sentinel).all())
    # ... and the same call goes through once nothing is wrong with it
    assert call(2) == 0 and npart.value == 1
    torch.cuda.synchronize()
    assert torch.equal(out[:n * 32].view(n, 32), ops.gin(a, graph, *params, act=L, kernel="fused")[0])
    # ops.gin: the width-32 names at another width, and a refusal as the library's error
    from tilingnn_amd._lib import TgnnError
    p64 = gc.problem(5, 64, False, 1.0)
    with pytest.raises(ValueError, match="width-32"):
        ops.gin(p64.a.to(dev), col_graph(5, dev), *[t.to(dev) for t in gc.param_list(p64.sd)], kernel="fused")
    with pytest.raises(TgnnError, match="LeakyReLU"):
        ops.gin(a, graph, *params, act=NONE, kernel="f16")


# ---------------------------------------------------------------------------------------------- the forward runs these ops
def _forward_buffers(net, inputs, n, dev):
    """One inference forward -> (graph, slots [D + 1][n][32], a2 parity-0 / parity-1 buffers, stat2 records [2][4][32]): the
    workspace's carves as tests/test_gin_fused.py::_run reads them (csrc/forward.hip: carve), all left on the device.  The
    records: stat1, stat2[0], stat2[1], stat_i[0 .. 1] (512 bytes each at width 32) and stat_f[0 .. 3] (4 096 bytes each) are the
    last pieces of the workspace, 256 bytes before its end."""
    from tilingnn_amd import _lib, ops
    x, adj, attr, col = inputs
    graph = ops.prepare_graph(n, adj, attr, col)
    dims = net._dims()
    table, _ = net._param_table()
    ws_bytes = _lib.lib.tgnn_forward_workspace_bytes(C.byref(dims), n, graph.n_types)
    ws = torch.zeros(ws_bytes, dtype=torch.uint8, device=dev)
    probs = torch.empty(n, 1, device=dev)
    g = graph.c_struct()
    _lib.check(_lib.lib.tgnn_forward(C.byref(dims), table, ops.ptr(x), ops.ptr(attr), C.byref(g), 0, 0, ops.ptr(probs), ops.ptr(ws), ws_bytes,
                                    _lib.current_stream(dev), _lib.side_stream(dev)))
    torch.cuda.synchronize()
    f = ws.view(torch.float32)
    d = net.network_depth
    al = lambda k: (k + 63) // 64 * 64
    o = al((d + 1) * n * 32)
    o = al(o + n * 32)                                          # a1
    a2 = [f[o:o + n * 32].view(n, 32).clone(), f[al(o + n * 32):al(o + n * 32) + n * 32].view(n, 32).clone()]
    slots = f[:(d + 1) * n * 32].view(d + 1, n, 32).clone()
    s0 = (ws_bytes - 256 - 4 * 4096 - 4 * 512) // 4
    stat2 = f[s0:s0 + 256].view(2, 4, 32).clone()
    return graph, slots, a2, stat2, probs


def _check_record(stat, rows, bn, what):
    """A BatchNorm record against the fp64 batch statistics of the rows it was folded from: stat_ok of
    tests/test_training_sizes.py, at its tolerances."""
    a = rows.double().cpu()
    mean = a.mean(0)
    ginv = bn.weight.detach().double().cpu() / torch.sqrt(((a - mean) ** 2).mean(0) + 1e-5)
    s = stat.cpu()
    e_mean = orc.rel_max_err(s[0].double() + s[1].double(), mean)
    e_ginv = orc.rel_max_err(s[2], ginv)
    e_beta = orc.rel_max_err(s[3], bn.bias.detach().double().cpu())
    print(f"{what}: record vs fp64 batch statistics: mean {e_mean:.2e}, gamma / sigma {e_ginv:.2e}, beta {e_beta:.2e}")
    assert e_mean < 2e-3 and e_ginv < 2e-3 and e_beta < 1e-6, what


@pytest.mark.parametrize("n", gc.FORWARD_ROWS)
def test_the_forward_runs_these_ops(dev, n, general_schedule):
    """Depth 2 on the general schedule, under the default switches, tgnn_set_gin_mlp_f16(1) and tgnn_set_gin_fused(2): a2 of
    layer 0 IS the op of the matching form on slot 0; the record the GIN kernel's last blocks folded (GinFin, at 1, 2, 7, 8, 16
    and 24 blocks) is the fp64 batch statistics of those rows; a2 of layer 1 IS the op on (a2 of layer 0, that record)."""
    from tests.test_hip_parity import make_net
    from tests.test_mid_layout import _layout
    from tilingnn_amd import _lib, ops
    inputs, _ = _layout(n, dev, seed=3, ea_per=3, ec_per=3)
    net, _ = make_net(dev, depth=2)
    prev_f16, prev_fused = _lib.lib.tgnn_set_gin_mlp_f16(0), _lib.lib.tgnn_set_gin_fused(1)
    try:
        assert (prev_f16, prev_fused) == (0, 1)                  # the defaults
        for variant in (0, 1, 2):
            if variant == 1:
                _lib.lib.tgnn_set_gin_mlp_f16(1)
            if variant == 2:
                _lib.lib.tgnn_set_gin_mlp_f16(0)
                _lib.lib.tgnn_set_gin_fused(2)
            graph, slots, a2, stat2, probs = _forward_buffers(net, inputs, n, dev)
            assert bool(torch.isfinite(probs).all())
            kernel = gc.VARIANTS[variant]
            for i in (0, 1):
                layer = net.brch_2_coll_conv_layers[i]
                mlp = [t.detach() for t in layer.ginConv._mlp_params()]
                src, rec = (slots[0], None) if i == 0 else (a2[0], stat2[0])
                part = ops.new_partials(32, dev)
                want, npart = ops.gin(src, graph, layer.ginConv.eps, *mlp, act=ops.ACT_LEAKY_RELU, in_stat=rec, partials=part, kernel=kernel)
                assert npart == gc.gin32_blocks(n)
                assert torch.equal(a2[i], want), (kernel, i, int((a2[i] != want).any(1).sum()))
                _check_record(stat2[i], a2[i], layer.batch_norm, f"n {n} ({npart} blocks) {kernel} layer {i}")
    finally:
        _lib.lib.tgnn_set_gin_mlp_f16(prev_f16)
        _lib.lib.tgnn_set_gin_fused(prev_fused)


def test_the_default_fused_regime(dev):
    """200 003 nodes, no switch touched: the forward runs gin32_fused_kernel (from 200 000 nodes on), 14 tiles per team through a
    hand-over ring of 6 -- every slot reused twice.  Layer 0's collision rows against fp64 at 1e-6, equal to the op bit for bit
    (and so to the two-launch form: test_variants_against_each_other), and the folded record."""
    from tests.test_hip_parity import make_net
    from tests.test_mid_layout import _layout
    from tilingnn_amd import _lib, ops
    n = 200003
    assert _lib.lib.tgnn_set_gin_fused(1) == 1 and _lib.lib.tgnn_set_gin_mlp_f16(0) == 0      # the defaults
    assert gc.forward_default_variant(n) == 2
    inputs, _ = _layout(n, dev, seed=3, ea_per=3, ec_per=6)
    net, sd = make_net(dev, depth=1)
    graph, slots, a2, stat2, probs = _forward_buffers(net, inputs, n, dev)
    layer = net.brch_2_coll_conv_layers[0]
    mlp = [t.detach() for t in layer.ginConv._mlp_params()]
    fused, npart = ops.gin(slots[0], graph, layer.ginConv.eps, *mlp, act=ops.ACT_LEAKY_RELU, partials=ops.new_partials(32, dev), kernel="fused")
    two, _ = ops.gin(slots[0], graph, layer.ginConv.eps, *mlp, act=ops.ACT_LEAKY_RELU, kernel="bf16x3")
    assert npart == 224
    assert torch.equal(a2[0], fused), int((a2[0] != fused).any(1).sum())
    assert torch.equal(fused, two)
    with torch.no_grad():
        want = orc.leaky_relu(orc.gin_conv(slots[0].double().cpu(), inputs[3].cpu(), orc.cast_sd(sd, torch.float64), "brch_2_coll_conv_layers.0"))
    err = orc.rel_max_err(a2[0].cpu(), want)
    print(f"default forward n {n}: GINConv_0 (gin32_fused_kernel, {npart} blocks) vs fp64 {err:.3e}")
    assert err < GATE
    _check_record(stat2[0], a2[0], layer.batch_norm, f"n {n} fused layer 0")


# ---------------------------------------------------------------------------------------------- CollConv including its BatchNorm
@pytest.mark.parametrize("n", [1254, 30000])
def test_collconv_including_its_batch_norm(dev, n):
    """GINConv -> LeakyReLU -> train-mode BatchNorm per form against orc.coll_conv at smoke()'s gate of 4e-5.  1 254: smoke()'s own
    inputs (the labyrinth layout behind the init MLP, make_state_dict's weights -- columns that vary by ~1 % of their value, the
    ill-conditioned case the reviews quote); 30 000: the op case's inputs with a random gamma / beta."""
    from tilingnn_amd import ops
    if n == 1254:
        from tests.golden_util import graph_tensors, load_labyrinth_graph
        from tilingnn_amd.weights import make_state_dict
        sd = make_state_dict(15, 20, 32, 1, 3, seed=0)
        sd64 = orc.cast_sd(sd, torch.float64)
        xc, _, _, colc, _ = graph_tensors(load_labyrinth_graph(), torch.float64)
        prefix = "brch_2_coll_conv_layers.0"
        with torch.no_grad():
            a = orc.init_node_feature_trans(xc, sd64).float()
        gsd = {k.replace(prefix, PREFIX): v for k, v in sd.items() if k.startswith(prefix + ".")}
        ei = colc
    else:
        p = gc.problem(n, 32, False, 1.0)
        a, ei = p.a, p.ei
        g = torch.Generator().manual_seed(9)
        gsd = dict(p.sd)
        gsd[f"{PREFIX}.batch_norm.weight"] = 1 + 0.3 * torch.randn(32, generator=g)
        gsd[f"{PREFIX}.batch_norm.bias"] = 0.2 * torch.randn(32, generator=g)
    with torch.no_grad():
        want = orc.coll_conv(a.double(), ei, orc.cast_sd(gsd, torch.float64), PREFIX)
        floor = orc.rel_max_err(orc.coll_conv(a, ei, gsd, PREFIX), want)
    graph = col_graph(n, dev)
    params = [gsd[f"{PREFIX}.ginConv.eps"]] + [gsd[f"{PREFIX}.ginConv.nn.mlp.{i}.linear.{k}"] for i in range(3) for k in ("weight", "bias")]
    params = [t.to(dev) for t in params]
    bn = torch.nn.BatchNorm1d(32).to(dev).train()
    with torch.no_grad():
        bn.weight.copy_(gsd[f"{PREFIX}.batch_norm.weight"])
        bn.bias.copy_(gsd[f"{PREFIX}.batch_norm.bias"])
    for kernel in gc.VARIANTS.values():
        part = ops.new_partials(32, dev)
        out, npart = ops.gin(a.to(dev), graph, *params, act=ops.ACT_LEAKY_RELU, partials=part, kernel=kernel)
        got = ops.batch_norm(out, part, npart, bn)
        err = orc.rel_max_err(got.cpu(), want)
        print(f"CollConv + BatchNorm n {n} {kernel}: rel_max_err {err:.3e} (fp32 torch {floor:.3e})")
        assert err < 4e-5, kernel
