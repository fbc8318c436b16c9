"""tgnn_bn_finalize, tgnn_bn_apply, tgnn_merge_fwd and ops.batch_norm as ops (csrc/bn_merge.hip) against fp64.

bn_finalize gets partial rows made in the test -- the fp64 column sums of a random fp32 matrix split at random over the rows, no
producer kernel involved -- at every count that changes the kernel's path: 16 row groups, loads unrolled 32 x, 8 x and singly, so
1 / 15 / 16 / 17 (single rows), 127 / 128 / 129 (the 8 x 16 tier starts at 113 + group) and 511 / 512 (the 32 x 16 tier).
bn_apply and merge are held element by element: bn_apply1 is ((v - mean_hi) - mean_lo) * ginv + beta, three roundings, and the
record's ginv carries one, so |err| <= 4 * 2^-24 * (|v - mean| ginv + |want|); merge by the product rule over two such bounds
plus one rounding for the product and one for the residual.  The mean's split into hi + lo is what keeps this bound on the
near-constant columns of the collision branch (v = 1000 + 2^-10 randn: tests/test_dense_oracle_host.py shows the bound fails
when the low half is ignored)."""
import pytest
import torch

from tests import dense_oracle as do

pytestmark = pytest.mark.gpu

U32 = 2.0 ** -24
EPS32 = float(torch.tensor(1e-5, dtype=torch.float32))         # eps and momentum cross the ABI as floats (as torch's own fp32
MOM32 = float(torch.tensor(0.1, dtype=torch.float32))          # BatchNorm casts them): 0.1f = 0.1 (1 + 1.5e-8)


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "GPU tests need a GPU"
    return torch.device("cuda:0")


def make_bn(f, dev, seed):
    g = torch.Generator().manual_seed(seed)
    bn = torch.nn.BatchNorm1d(f).to(dev)
    with torch.no_grad():
        bn.weight.copy_(1.0 + 0.25 * torch.randn(f, generator=g))
        bn.bias.copy_(0.25 * torch.randn(f, generator=g))
        bn.running_mean.copy_(torch.randn(f, generator=g))
        bn.running_var.copy_(0.5 + torch.rand(f, generator=g))
        bn.num_batches_tracked.fill_(41)
    return bn


def buffers(bn):
    return bn.running_mean.clone(), bn.running_var.clone(), bn.num_batches_tracked.clone()


def split_sums(x, n_partials, seed):
    """fp64 column sums [sum | sum of squares] of x, and partial rows [n_partials, 2 f] that add up to them: random positive
    fractions, the last row the remainder (all parts of one sign: re-adding them in any order is good to 2^-53 n_partials)."""
    x64 = x.double()
    sums = torch.cat([x64.sum(0), (x64 * x64).sum(0)])
    g = torch.Generator().manual_seed(seed)
    frac = torch.rand(n_partials, sums.numel(), generator=g, dtype=torch.float64).to(x.device) + 0.05
    frac = frac / frac.sum(0)
    rows = frac * sums
    rows[-1] = sums - rows[:-1].sum(0)
    return sums, rows.contiguous()


def ulps(got, want64):
    """|got - want| in ulp of fp32 at want, the worst element"""
    return float(((got.double() - want64).abs() / do.ulp32(want64)).max())


def check_record(stat, mean, var, bn, bad, label, mean_tol=2.0 ** -45, ginv_ulp=2.0):
    mh, ml = stat[0].double(), stat[1].double()
    rel = float((((mh + ml) - mean).abs() / mean.abs().clamp(min=1e-300)).max())
    if not rel <= mean_tol:
        bad.append("%s: mean_hi + mean_lo off by %.3g relative" % (label, rel))
    if not bool((stat[0] == mean.float()).all()):
        bad.append("%s: mean_hi is not the mean rounded to fp32" % label)
    want_ginv = bn.weight.detach().double() / torch.sqrt(var + EPS32)
    if not ulps(stat[2], want_ginv) <= ginv_ulp:
        bad.append("%s: ginv off by %.2f ulp" % (label, ulps(stat[2], want_ginv)))
    if not torch.equal(stat[3], bn.bias.detach()):
        bad.append("%s: beta is not the bias" % label)


@pytest.mark.parametrize("f", [32, 48, 64, 256])
def test_bn_finalize_on_synthesised_partial_rows(dev, f):
    from tilingnn_amd import ops
    n_rows = 777
    x = (torch.randn(n_rows, f, generator=torch.Generator().manual_seed(f)) * 1.5 + 0.75).to(dev)
    x64 = x.double()
    bad = []
    for n_partials in (1, 15, 16, 17, 127, 128, 129, 511, 512):
        label = "f %d, %d partial rows" % (f, n_partials)
        sums, rows = split_sums(x, n_partials, 100 * f + n_partials)
        mean, var = sums[:f] / n_rows, x64.var(0, unbiased=False)
        # mode 0, running buffers untouched
        bn = make_bn(f, dev, f)
        before = buffers(bn)
        stat = ops.bn_finalize(rows, n_partials, n_rows, bn, update_running=False)
        check_record(stat, mean, var, bn, bad, label)
        if not all(torch.equal(a, b) for a, b in zip(before, buffers(bn))):
            bad.append(label + ": update_running=False changed a buffer")
        # mode 0 with the update: torch.nn.BatchNorm1d's rule in fp64 (momentum 0.1, unbiased variance)
        stat_u = ops.bn_finalize(rows, n_partials, n_rows, bn, update_running=True)
        # (from random buffers the update cancels, 0.9 rm + 0.1 mean ~ 0 in some columns, and 0.1f - 0.1 = 1.5e-9 shows as
        #  3 .. 11 ulp of the RESULT: the fp64 rule is evaluated with the momentum the library was handed; from torch's start
        #  state, below, with 0.1 itself -- there the float costs 0.25 ulp)
        want_rm = (1.0 - MOM32) * before[0].double() + MOM32 * mean
        want_rv = (1.0 - MOM32) * before[1].double() + MOM32 * var * (n_rows / (n_rows - 1.0))
        if not torch.equal(stat_u, stat):
            bad.append(label + ": the record depends on update_running")
        if not (ulps(bn.running_mean, want_rm) <= 1.0 and ulps(bn.running_var, want_rv) <= 1.0):
            bad.append("%s: running mean / var off by %.2f / %.2f ulp" % (label, ulps(bn.running_mean, want_rm),
                                                                         ulps(bn.running_var, want_rv)))
        if int(bn.num_batches_tracked) != 42:
            bad.append("%s: num_batches_tracked %d" % (label, int(bn.num_batches_tracked)))
        fresh = torch.nn.BatchNorm1d(f).to(dev)                           # running_mean 0, running_var 1, momentum 0.1
        ops.bn_finalize(rows, n_partials, n_rows, fresh, update_running=True)
        off = (ulps(fresh.running_mean, 0.1 * mean), ulps(fresh.running_var, 0.9 + 0.1 * var * (n_rows / (n_rows - 1.0))))
        if not (max(off) <= 1.0 and int(fresh.num_batches_tracked) == 1):
            bad.append("%s: from the start state, running mean / var off by %.2f / %.2f ulp" % ((label,) + off))
        # mode 1 then mode 2: the bits of mode 0, record and buffers
        bn2 = make_bn(f, dev, f)
        got_sums = ops.bn_sums(rows, n_partials, f)
        rel = float(((got_sums - sums).abs() / sums.abs()).max())
        if not rel <= 2.0 ** -45:
            bad.append("%s: mode 1 sums off by %.3g relative" % (label, rel))
        stat2 = ops.bn_stat_from_sums(got_sums, n_rows, bn2, update_running=True)
        if not (torch.equal(stat2, stat) and all(torch.equal(a, b) for a, b in zip(buffers(bn), buffers(bn2)))):
            bad.append(label + ": mode 1 + mode 2 differ from mode 0")
    assert not bad, "\n".join(bad)


@pytest.mark.parametrize("f", [32, 48, 256])
def test_bn_finalize_mode3_builds_the_record_from_the_running_buffers(dev, f):
    from tilingnn_amd import ops
    bn = make_bn(f, dev, 7 + f)
    before = buffers(bn)
    stat = ops.bn_finalize(None, 1, 1, bn, update_running=False, mode=3)
    bad = []
    check_record(stat, bn.running_mean.double(), bn.running_var.double(), bn, bad, "mode 3", mean_tol=0.0, ginv_ulp=1.0)
    assert not bad, "\n".join(bad)
    assert bool((stat[1] == 0).all())                                    # (an fp32 mean has no low half)
    assert all(torch.equal(a, b) for a, b in zip(before, buffers(bn)))


def test_bn_finalize_constant_column_and_the_negative_variance_clamp(dev):
    """1000.1 in every row.  64 rows in 16 partial rows of 4 rows each: every sum is exact in fp64 (1000.1f squared has 48
    bits), so is the mean, and the variance comes out as exactly 0: ginv = gamma / sqrt(eps).  A producer's rounding can leave
    the sum of squares a hair short of n mean^2: the same rows with that column's squares reduced by 2^-40 give a variance of
    -9e-7, which the clamp must turn into 0 (unclamped: ginv 4.9 % off, or NaN for a larger deficit)."""
    from tilingnn_amd import ops
    f, n_rows, n_partials, col = 32, 64, 16, 3
    x = torch.randn(n_rows, f, generator=torch.Generator().manual_seed(11))
    x[:, col] = 1000.1
    x = x.to(dev)
    chunks = x.double().view(n_partials, n_rows // n_partials, f)
    rows = torch.cat([chunks.sum(1), (chunks * chunks).sum(1)], dim=1).contiguous()
    c = float(x[0, col])
    assert float(rows[:, f + col].sum()) == n_rows * c * c and float(rows[:, col].sum()) == n_rows * c
    short = rows.clone()
    short[:, f + col] *= 1.0 - 2.0 ** -40
    for label, part in (("exact sums", rows), ("squares short by 2^-40", short)):
        bn = make_bn(f, dev, 13)
        before = buffers(bn)
        stat = ops.bn_finalize(part, n_partials, n_rows, bn, update_running=True)
        assert bool(torch.isfinite(stat).all()), label
        want = bn.weight.detach().double()[col] / torch.sqrt(torch.tensor(EPS32, dtype=torch.float64, device=dev))
        assert ulps(stat[2, col], want) <= 1.0, (label, float(stat[2, col]), float(want))
        assert float(stat[0, col]) == c and float(stat[1, col]) == 0.0, label
        assert ulps(bn.running_var[col], 0.9 * before[1][col].double()) <= 1.0, label
        assert bool(torch.isfinite(bn.running_var).all() and torch.isfinite(bn.running_mean).all()), label


def test_bn_finalize_of_a_single_row_is_finite(dev):
    from tilingnn_amd import ops
    f = 48
    x = torch.randn(1, f, generator=torch.Generator().manual_seed(2)).to(dev) * 3
    sums = torch.cat([x.double().sum(0), (x.double() ** 2).sum(0)]).contiguous()
    bn = make_bn(f, dev, 3)
    stat = ops.bn_stat_from_sums(sums, 1, bn, update_running=True)
    assert bool(torch.isfinite(stat).all())
    assert bool(torch.isfinite(bn.running_mean).all() and torch.isfinite(bn.running_var).all())
    assert torch.equal(stat[0], x[0])                                    # the mean of one row is the row
    want = bn.weight.detach().double() / torch.sqrt(torch.tensor(EPS32, dtype=torch.float64, device=dev))
    assert float(((stat[2].double() - want).abs() / want.abs()).max()) < 1e-3     # (variance 0 up to the rounding of x^2 - x x)


# ------------------------------------------------------------------------------------------ bn_apply
def random_record(f, dev, seed, offset=0.0):
    g = torch.Generator().manual_seed(seed)
    mean = offset + torch.randn(f, generator=g, dtype=torch.float64)
    var = 0.25 + 2.0 * torch.rand(f, generator=g, dtype=torch.float64)
    gamma = 1.0 + 0.25 * torch.randn(f, generator=g, dtype=torch.float64)
    beta = 0.25 * torch.randn(f, generator=g, dtype=torch.float64)
    return do.stat_record(mean, var, gamma, beta).to(dev)


def bn_want_and_bound(v, stat):
    s = stat.double()
    centred = (v.double() - s[0]) - s[1]
    want = centred * s[2] + s[3]
    return want, 4.0 * U32 * (centred.abs() * s[2].abs() + want.abs())


def bn_apply_failures(got, v, stat, label):
    want, bnd = bn_want_and_bound(v, stat)
    err = (got.double() - want).abs()
    if bool((err <= bnd).all()):
        return []
    over = torch.nonzero(~(err <= bnd))
    r, c = (int(i) for i in over[0])
    return ["%s: %d elements over the bound, first at row %d column %d: got %.9g want %.9g (bound %.3g)"
            % (label, over.shape[0], r, c, float(got[r, c]), float(want[r, c]), float(bnd[r, c]))]


@pytest.mark.parametrize("f", [32, 33, 64, 256])
def test_bn_apply_against_fp64(dev, f):
    from tilingnn_amd import ops
    bad = []
    for n in (1, 7, 1254, 70001):
        v = (torch.randn(n, f, generator=torch.Generator().manual_seed(n + f)) * 1.5 + 0.5).to(dev)
        stat = random_record(f, dev, 5 * f + n, offset=0.5)
        bad += bn_apply_failures(ops.bn_apply(v, stat), v, stat, "f %d n %d" % (f, n))
    assert not bad, "\n".join(bad)


@pytest.mark.parametrize("n", [1, 7, 1254, 70001])
def test_bn_apply_packed_path_and_generic_path_agree_bit_for_bit(dev, n):
    """f = 32 with ldv = ldo = 32 takes the float4 path of bn_apply_kernel, with ldv = ldo = 64 the generic one"""
    from tilingnn_amd import _lib, ops
    v = torch.randn(n, 32, generator=torch.Generator().manual_seed(n)).to(dev)
    stat = random_record(32, dev, n)
    packed = ops.bn_apply(v, stat)
    wide_in = torch.full((n, 64), 3.5, device=dev)
    wide_in[:, :32] = v
    wide_out = torch.full((n, 64), -7.25, device=dev)
    _lib.check(_lib.lib.tgnn_bn_apply(_lib.ptr(wide_in), 64, _lib.ptr(stat), n, 32, _lib.ptr(wide_out), 64, _lib.current_stream(dev)))
    assert torch.equal(wide_out[:, :32], packed)
    assert bool((wide_out[:, 32:] == -7.25).all())
    assert not bn_apply_failures(packed, v, stat, "packed n %d" % n)


def test_bn_apply_on_near_constant_columns_with_bn_finalizes_own_record(dev):
    """v = 1000 + 2^-10 randn: the low half of the mean is 0.03 standard deviations (tests/test_dense_oracle_host.py: the bound
    fails without it)"""
    from tilingnn_amd import ops
    n, f = 1254, 32
    v = (1000.0 + 2.0 ** -10 * torch.randn(n, f, generator=torch.Generator().manual_seed(5), dtype=torch.float64)).float().to(dev)
    rows = torch.stack([do.column_sums(c) for c in v.split(128)]).contiguous()
    bn = make_bn(f, dev, 9)
    stat = ops.bn_finalize(rows, rows.shape[0], n, bn, update_running=False)
    assert float(stat[1].abs().max()) > 2e-6                              # (there is a low half)
    v64 = v.double()
    mean = v64.mean(0)
    assert float((((stat[0].double() + stat[1].double()) - mean).abs() / mean).max()) <= 2.0 ** -45
    got = ops.bn_apply(v, stat)
    assert not bn_apply_failures(got, v, stat, "near-constant")
    dropped = stat.clone()
    dropped[1] = 0
    assert bn_apply_failures(got, v, dropped, "without mean_lo")          # (the gate tells the two apart)
    # and the result is the BatchNorm of v: fp64 two-pass statistics; the one-pass variance in fp64 is good to
    # 2^-53 n mean^2 / var = 1e-13 * 1254 * 1e6 / 1e-6 relative at worst, here 1e-4
    want = (v64 - mean) / torch.sqrt(v64.var(0, unbiased=False) + EPS32) * bn.weight.detach().double() + bn.bias.detach().double()
    assert float((got.double() - want).abs().max()) < 1e-3 * float(want.abs().max())


# ------------------------------------------------------------------------------------------ merge
@pytest.mark.parametrize("c", [32, 64, 96])
def test_merge_against_fp64(dev, c):
    from tilingnn_amd import ops
    bad = []
    for n in (1, 37, 4099):
        g = torch.Generator().manual_seed(1000 * c + n)
        a1 = (torch.randn(n, c, generator=g) * 1.5 + 0.5).to(dev)
        a2 = (torch.randn(n, c, generator=g) * 0.7 - 0.25).to(dev)
        resid_t = torch.randn(n, c, generator=g).to(dev)
        st1, st2 = random_record(c, dev, c + n, 0.5), random_record(c, dev, 2 * c + n, -0.25)
        y1, b1 = bn_want_and_bound(a1, st1)
        y2, b2 = bn_want_and_bound(a2, st2)
        for resid in (None, resid_t):
            want = y1 * y2 + (resid.double() if resid is not None else 0.0)
            # product rule over the two bn_apply bounds, one rounding for the product, one for the sum with the residual
            bnd = y1.abs() * b2 + y2.abs() * b1 + b1 * b2 + U32 * (y1 * y2).abs() + (U32 * want.abs() if resid is not None else 0.0)
            for want_h2 in (False, True):
                label = "c %d n %d resid %s h2 %s" % (c, n, resid is not None, want_h2)
                buf = torch.full((3, n, c), -7.25, device=dev)
                out, h2 = ops.merge(a1, st1, a2, st2, resid, out=buf[1], want_h2=want_h2)
                if out.data_ptr() != buf[1].data_ptr() or (h2 is None) == want_h2:
                    bad.append(label + ": outputs")
                if not bool((buf[0] == -7.25).all() and (buf[2] == -7.25).all()):
                    bad.append(label + ": a neighbouring slot changed")
                err = (buf[1].double() - want).abs()
                if not bool((err <= bnd).all()):
                    bad.append("%s: %d elements over the bound, worst %.3g x" % (label, int((~(err <= bnd)).sum()),
                                                                                float((err / bnd).max())))
                if want_h2:
                    bad += bn_apply_failures(h2, a2, st2, label + " h2")
    assert not bad, "\n".join(bad)


# ------------------------------------------------------------------------------------------ ops.batch_norm
def test_batch_norm_train_mode_needs_two_rows(dev):
    from tilingnn_amd import ops
    bn = make_bn(32, dev, 1).train()
    before = buffers(bn)
    v = torch.randn(1, 32).to(dev)
    with pytest.raises(ValueError, match="Expected more than 1 value per channel when training"):
        ops.batch_norm(v, do.column_sums(v).view(1, -1).contiguous(), 1, bn)
    assert all(torch.equal(a, b) for a, b in zip(before, buffers(bn)))


@pytest.mark.parametrize("n", [1, 300])
def test_batch_norm_eval_mode_uses_the_running_statistics(dev, n):
    from tilingnn_amd import ops
    f = 64
    bn = make_bn(f, dev, 4).eval()
    before = buffers(bn)
    v = (torch.randn(n, f, generator=torch.Generator().manual_seed(n)) * 2 + 1).to(dev)
    rows = do.column_sums(v).view(1, -1).contiguous()
    got = ops.batch_norm(v, rows, 1, bn)
    assert all(torch.equal(a, b) for a, b in zip(before, buffers(bn)))
    centred = v.double() - bn.running_mean.double()
    ginv = bn.weight.detach().double() / torch.sqrt(bn.running_var.double() + EPS32)
    want = centred * ginv + bn.bias.detach().double()
    assert bool(((got.double() - want).abs() <= 4.0 * U32 * (centred.abs() * ginv.abs() + want.abs())).all())
