"""ops.dense_act over the whole dispatch of dense_act_impl (csrc/dense.hip) against the fp64 reference of tests/dense_oracle.py:
every kernel the case tables of tests/dense_cases.py name, at the row counts and widths where each goes wrong (see that module;
tests/test_dense_oracle_host.py shows which kernel each case reaches and that the gates hold plain fp32 and reject what a wrong
kernel produces).  Every case: the max-norm gate and the element-wise gate on every element; where partial sums were asked for,
their fp64 total against the fp64 sums of the fp32 values stored.  A failure names the kernel, the shape, the row count and the
first element over its bound.  Every measured figure goes to the table printed when the module ends (profiles/dense_ops_errors.txt
is one run of it)."""
import ctypes as C

import pytest
import torch

from tests import dense_cases as dc
from tests import dense_oracle as do

pytestmark = pytest.mark.gpu

WORST = {}          # kernel -> [element-wise ratio, max-norm error, partial-sum ratio, cases]


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "GPU tests need a GPU"
    yield torch.device("cuda:0")
    print("\n# kernel: worst error / element-wise bound, worst max-norm error, worst partial-sum difference / (1e-12 |sum|), cases")
    for kernel in sorted(WORST):
        r, e, p, c = WORST[kernel]
        print("dense_ops_errors: %-16s %.3f  %.3e  %.3e  %d" % (kernel, r, e, p, c))


def note(kernel, ratio, rel, part):
    w = WORST.setdefault(kernel, [0.0, 0.0, 0.0, 0])
    w[0], w[1], w[2], w[3] = max(w[0], ratio), max(w[1], rel), max(w[2], part), w[3] + 1


def on_device(a, dev, misaligned=False):
    if not misaligned:
        return a.to(dev)
    buf = torch.empty(a.numel() + 1, dtype=torch.float32, device=dev)      # one float past the allocation's 16-byte boundary
    view = buf[1:].view(a.shape)
    view.copy_(a)
    assert view.data_ptr() % 16 == 4 and view.is_contiguous()
    return view


def run_one(ops, dev, kernel, label, a, w, b, rec, act, want_partials, slot_major, f16_split, pre, bad, cus=None):
    """One call of ops.dense_act, both gates, the partial sums.  Returns the output."""
    m = int(w.shape[0])
    partials = ops.new_partials(m, dev) if want_partials else None
    got, n_part = ops.dense_act(a, w, b, act, in_stat=rec, partials=partials, slot_major=slot_major, f16_split=f16_split)
    f16 = bool(f16_split)
    ref = do.reference(a, w, b, act, rec, slot_major, pre=pre)
    rel, ratio = do.measure(got, ref, act, f16)
    fails = do.gate_failures(got, ref, act, f16)
    part = 0.0
    if want_partials:
        rows = partials[:max(n_part, 0) * 2 * m].view(-1, 2 * m)
        fails += do.partial_failures(rows, n_part, got, True)
        expected = dc.expected_partial_rows(kernel, got.shape[0], cus)              # (the count tells the kernels apart)
        if expected not in (None, n_part):
            fails.append("%d partial rows, %s gives %d" % (n_part, kernel, expected))
        if 1 <= n_part <= do.MAX_PARTIALS:
            part = do.partial_sum_ratio(rows, got)
    elif kernel.startswith("out1") and n_part != 0:
        fails.append("n_partials %d from the out_dim == 1 kernel" % n_part)
    note(kernel, ratio, rel, part)
    bad += ["%s %s act %d: %s" % (kernel, label, act, f) for f in fails]
    return got


PLAIN_GROUPS = [g for g in dc.GROUPS if g.kind != "f16"]


@pytest.mark.parametrize("group,shape", dc.group_shapes(PLAIN_GROUPS),
                         ids=lambda v: v.name if isinstance(v, dc.Group) else dc.shape_id(v))
def test_dense_act_against_fp64(dev, group, shape):
    from tilingnn_amd import ops
    assert (ops.ACT_NONE, ops.ACT_LEAKY_RELU, ops.ACT_SIGMOID) == (dc.NONE, dc.LEAKY, dc.SIGMOID)
    k, m, cw = dc.shape_dims(group, shape)
    slot_major = group.kind == "slots"
    bad = []
    for n in group.rows:
        for stat in group.stats:
            a, w, b, rec = dc.make_inputs(group, shape, n, stat)
            a, w, b = on_device(a, dev, group.kind == "misaligned"), w.to(dev), b.to(dev)
            rec = rec.to(dev) if rec is not None else None
            pre = do.pre_activation(a, w, b, rec, slot_major)
            for want_partials in group.partials:
                kernel = dc.dispatch(group.kind, k, m, n, cw, stat, want_partials)
                assert kernel in group.kernels
                for act in group.acts:
                    run_one(ops, dev, kernel, "%s n %d in_stat %s partials %s" % (dc.shape_id(shape), n, stat, want_partials),
                            a, w, b, rec, act, want_partials, slot_major, False, pre, bad)
    assert not bad, "\n".join(bad)


@pytest.mark.parametrize("k,m,kernel", [(32, 1, "out1<8>"), (32, 32, "mfma<1,true>"), (36, 40, "mfma<2,false>"), (32, 64, "split<1,1>")])
def test_batchnorm_on_load_keeps_the_means_low_half(dev, k, m, kernel):
    """Near-constant input columns, v = 1000 + 2^-10 randn with the record from their fp64 statistics (what the collision
    branch hands the final MLP): both gates hold only if the kernel subtracts mean_lo as well -- with the record's low half
    zeroed the same reference is thousands of bounds away (tests/test_dense_oracle_host.py)."""
    from tilingnn_amd import ops
    n = 1254
    v, w, b, rec = (t.to(dev) for t in dc.near_constant_case(n, k, m))
    assert dc.dispatch("plain", k, m, n, stat=True) == kernel
    pre = do.pre_activation(v, w, b, rec)
    bad = []
    got = run_one(ops, dev, kernel, "near-constant %d -> %d" % (k, m), v, w, b, rec, dc.NONE, False, False, False, pre, bad)
    assert not bad, "\n".join(bad)
    dropped = rec.clone()
    dropped[1] = 0
    assert do.gate_failures(got, do.reference(v, w, b, dc.NONE, dropped), dc.NONE)       # (the gate tells the two records apart)


F16_GROUP = next(g for g in dc.GROUPS if g.kind == "f16")


@pytest.mark.parametrize("shape", F16_GROUP.shapes, ids=dc.shape_id)
def test_fp16_pair_kernels_against_fp64(dev, shape):
    """The fp16-pair block-tile kernels below the rows kernels' threshold, f16_split = "tile" and True (the same kernel: the same
    bits), with one all-zero slot, the whole input zero (the result is act(b) exactly: a bound of zero must not turn into a
    scale of inf) and one slot at 2^20 times the others (the bound is per slot)."""
    from tilingnn_amd import ops
    group = F16_GROUP
    k, m, cw = dc.shape_dims(group, shape)
    bad = []
    for n in group.rows:
        base, w, b, _ = dc.make_inputs(group, shape, n)
        base, w, b = base.to(dev), w.to(dev), b.to(dev)
        for variant in dc.f16_variants(shape):
            a = dc.apply_variant(base, variant)
            pre = do.pre_activation(a, w, b, None, True)
            for act in group.acts:
                outs = []
                for mode in dc.f16_modes(m):
                    for want_partials in group.partials:
                        kernel = dc.dispatch("f16", k, m, n, cw, False, want_partials, True, mode is True)
                        assert kernel in group.kernels
                        outs.append(run_one(ops, dev, kernel, "%s n %d %s f16_split %r partials %s"
                                            % (dc.shape_id(shape), n, variant, mode, want_partials), a, w, b, None, act, want_partials,
                                            True, mode, pre, bad))
                if not all(torch.equal(o, outs[0]) for o in outs):
                    bad.append("%s n %d %s act %d: the result depends on f16_split / partials" % (dc.shape_id(shape), n, variant, act))
                if variant == "zero":
                    want = torch.nn.functional.leaky_relu(b, 0.01) if act == dc.LEAKY else b
                    if not torch.equal(outs[0], want.expand_as(outs[0])):
                        bad.append("%s n %d act %d: zero input does not give act(b) exactly" % (dc.shape_id(shape), n, act))
    assert not bad, "\n".join(bad)


@pytest.fixture
def rows_mode_restored():
    from tilingnn_amd import _lib
    prev = _lib.lib.tgnn_set_dense_rows_mode(-1)             # (out of range: reads the mode, changes nothing)
    yield prev
    _lib.lib.tgnn_set_dense_rows_mode(prev)


@pytest.mark.parametrize("shape", dc.ROWS_GROUP.shapes, ids=dc.shape_id)
def test_rows_kernels_under_every_rows_mode(dev, shape, rows_mode_restored):
    """From 49 152 rows on f16_split=True takes a rows-per-wave kernel, which one by tgnn_set_dense_rows_mode: 2 (default) and 0
    dense_f16_rows_kernel, 3 dense_f16_rows2_kernel, 6 and 10 dense_f16_halves_kernel for 256 outputs (dense_cases.dispatch).
    Every mode: both gates, the bits of the block-tile kernel (f16_split="tile"), the partial sums."""
    from tilingnn_amd import _lib, ops
    assert rows_mode_restored == 2
    group = dc.ROWS_GROUP
    k, m, cw = dc.shape_dims(group, shape)
    act = group.acts[0]
    cus = torch.cuda.get_device_properties(dev).multi_processor_count
    bad = []
    for n in group.rows:
        a, w, b, _ = dc.make_inputs(group, shape, n)
        a, w, b = a.to(dev), w.to(dev), b.to(dev)
        pre = do.pre_activation(a, w, b, None, True)
        label = "%s n %d" % (dc.shape_id(shape), n)
        tile = run_one(ops, dev, dc.dispatch("f16", k, m, n, cw, f16=True), label + " tile", a, w, b, None, act, True, True, "tile",
                       pre, bad)
        for mode in dc.ROWS_MODES:
            _lib.lib.tgnn_set_dense_rows_mode(mode)
            assert _lib.lib.tgnn_set_dense_rows_mode(-1) == mode
            kernel = dc.dispatch("f16", k, m, n, cw, f16=True, wimg=True, rows_mode=mode)
            assert kernel.startswith(("rows", "halves"))
            for want_partials in group.partials:
                got = run_one(ops, dev, kernel, label + " mode %d partials %s" % (mode, want_partials), a, w, b, None, act,
                              want_partials, True, True, pre, bad, cus=cus * ((mode >> 2) & 3) if kernel.startswith("halves") else cus)
                if not torch.equal(got, tile):
                    bad.append("%s %s mode %d: not the bits of the block-tile kernel, %d elements differ"
                               % (kernel, label, mode, int((got != tile).sum())))
            _lib.lib.tgnn_set_dense_rows_mode(2)
    assert not bad, "\n".join(bad)


def test_set_dense_rows_mode_refuses_values_out_of_range(rows_mode_restored):
    from tilingnn_amd import _lib
    for bad_mode in (-1, 16, 1 << 20):
        assert _lib.lib.tgnn_set_dense_rows_mode(bad_mode) == rows_mode_restored
    assert _lib.lib.tgnn_set_dense_rows_mode(3) == rows_mode_restored
    assert _lib.lib.tgnn_set_dense_rows_mode(rows_mode_restored) == 3


# ------------------------------------------------------------------------------------------ argument rules
SENTINEL = -7.25


def test_refused_calls_raise_and_leave_the_output_untouched(dev):
    from tilingnn_amd import _lib, ops
    lib, ptr = _lib.lib, _lib.ptr
    stream = _lib.current_stream(dev)
    n = 130
    g = torch.Generator().manual_seed(3)
    w64 = torch.randn(64, 64, generator=g).to(dev)
    b64 = torch.randn(64, generator=g).to(dev)
    rec = do.stat_record(*(torch.rand(64, generator=g, dtype=torch.float64) + 0.5 for _ in range(4))).to(dev)
    # a slot width that is no multiple of 32
    a48 = torch.randn(2, n, 48, generator=g).to(dev)
    w96 = torch.randn(64, 96, generator=g).to(dev)
    with pytest.raises(ValueError, match="multiple of 32"):
        ops.dense_act(a48, w96, b64, ops.ACT_NONE, slot_major=True)
    out = torch.full((n, 64), SENTINEL, device=dev)
    n_part = C.c_int32(77)
    rc = lib.tgnn_dense_act_slots_fwd(ptr(a48), 48, n * 48, None, ptr(w96), ptr(b64), n, 96, 64, 0, ptr(out), 64, None,
                                      C.byref(n_part), stream)
    assert rc == -1 and b"slot width" in lib.tgnn_last_error()
    # in_dim mismatch, row-major and slot-major
    a = torch.randn(n, 32, generator=g).to(dev)
    with pytest.raises(ValueError, match="in_dim 64, got 32"):
        ops.dense_act(a, w64, b64, ops.ACT_NONE)
    a2 = torch.randn(3, n, 32, generator=g).to(dev)
    with pytest.raises(ValueError, match="in_dim 64, got 96"):
        ops.dense_act(a2, w64, b64, ops.ACT_NONE, slot_major=True)
    rc = lib.tgnn_dense_act_slots_fwd(ptr(a2), 64, n * 64, None, ptr(w96), ptr(b64), n, 96, 64, 0, ptr(out), 64, None,
                                      C.byref(n_part), stream)                   # (a slot width that does not divide in_dim)
    assert rc == -1
    # fp16 pairs with an input BatchNorm
    with pytest.raises(ValueError, match="no input BatchNorm"):
        ops.dense_act(a2[:2].contiguous(), w64, b64, ops.ACT_NONE, in_stat=rec, slot_major=True, f16_split=True)
    # fewer than 64 outputs on the fp16-pair ABI
    w32 = torch.randn(32, 64, generator=g).to(dev)
    with pytest.raises(_lib.TgnnError) as err:
        ops.dense_act(a2[:2].contiguous(), w32, b64[:32].contiguous(), ops.ACT_NONE, slot_major=True, f16_split="tile")
    assert err.value.code == -1
    bounds = torch.zeros(3, dtype=torch.int32, device=dev)
    rc = lib.tgnn_dense_act_slots_f16_fwd(ptr(a2), 32, n * 32, ptr(w32), ptr(b64), n, 64, 32, 0, ptr(out), 64, ptr(bounds), None, None,
                                          C.byref(n_part), stream)
    assert rc == -1
    torch.cuda.synchronize()
    assert bool((out == SENTINEL).all()) and n_part.value == 77


def test_no_rows_is_ok_with_no_partial_rows(dev):
    from tilingnn_amd import _lib, ops
    w = torch.randn(64, 32).to(dev)
    b = torch.randn(64).to(dev)
    for a, slot_major in ((torch.empty(0, 32, device=dev), False), (torch.empty(1, 0, 32, device=dev), True)):
        out, n_part = ops.dense_act(a, w, b, ops.ACT_LEAKY_RELU, partials=ops.new_partials(64, dev), slot_major=slot_major)
        assert tuple(out.shape) == (0, 64) and n_part == 0
    n_part = C.c_int32(77)
    out = torch.full((4, 64), SENTINEL, device=dev)
    rc = _lib.lib.tgnn_dense_act_fwd(None, 32, 32, None, _lib.ptr(w), _lib.ptr(b), 0, 32, 64, 1, _lib.ptr(out), 64, None,
                                     C.byref(n_part), _lib.current_stream(dev))
    torch.cuda.synchronize()
    assert rc == 0 and n_part.value == 0 and bool((out == SENTINEL).all())
