"""fp64 reference and gates of the dense Linear op (csrc/dense.hip through ops.dense_act): tests/test_dense_ops.py on the GPU,
tests/test_dense_oracle_host.py on the CPU.  Plain torch, no GPU import: every function works on the device its arguments are on.

The op:  act( BN_in(a) @ W.T + b ),  BN_in from a stat record [4, F] = (mean_hi, mean_lo, ginv, beta) as
((v - mean_hi) - mean_lo) * ginv + beta, a slot-major input [S, N, C] read as the concatenation of its slots.

Two gates, both on every element of every case:
  * the project's max-norm gate  max|got - want| / max|want| < 2e-6  (oracle.tilingnn_oracle.rel_max_err);
  * an element-wise, scale-aware one.  With z the pre-activation,
        |got_z - want_z| <= gamma * ( |BN_in(a)| @ |W|^T + |b| ),   gamma = (K + 8) * 2^-24 :
    the standard bound of an fp32 dot product of length K accumulated in any order, plus eight roundings for the BatchNorm
    on load, the bias, the activation's product and the store (the fp32 slope of LeakyReLU, 0.01f, is 2.2e-8 off the
    reference's 0.01: less than one of those roundings).  The fp16-pair kernels keep elements below 2^-39 of the operand's maximum
    only to 2^-39 of that maximum (the comment above dense_split_kernel): + K * 2^-38 * max|a| * max|W|.
    LeakyReLU is 1-Lipschitz and sigmoid 1/4-Lipschitz: both keep the bound; sigmoid adds 3.25 ulp of the result for its form
    (tests/test_sigmoid_form.py) and 2 ulp for the hardware's exp2 / reciprocal (that file's docstring).
The bounds are derived, not measured; the measured ratios error / bound are recorded in profiles/dense_ops_errors.txt."""
from collections import namedtuple

import torch

from oracle import tilingnn_oracle as orc

ACT_NONE, ACT_LEAKY_RELU, ACT_SIGMOID = 0, 1, 2        # include/tgnn.h: TGNN_ACT_*
U32 = 2.0 ** -24                                       # unit roundoff of fp32
REL_MAX_TOL = 2e-6                                     # the project's max-norm gate (tests/test_hip_parity.py)
SIGMOID_ULPS = 3.25 + 2.0
PARTIAL_RTOL = 1e-12                                   # (test_fp16_pair_split_kernels... of tests/test_hip_parity.py)
MAX_PARTIALS = 512                                     # TGNN_BN_MAX_PARTIALS

Ref = namedtuple("Ref", "y mag k a_max w_max")


def flatten(a, slot_major):
    """[S, N, C] -> [N, S C], the concatenation of the slots (what torch.cat of the skip connections would give)."""
    return a.permute(1, 0, 2).reshape(a.shape[1], -1) if slot_major else a


def stat_record(mean, var, gamma, beta, eps=1e-5):
    """fp64 vectors -> the fp32 record [4, F] the kernels read, built as tgnn_bn_finalize builds it: the mean split hi / lo."""
    mh = mean.float()
    ml = (mean - mh.double()).float()
    return torch.stack([mh, ml, (gamma / torch.sqrt(var + eps)).float(), beta.float()]).contiguous()


def bn_in(x64, stat):
    if stat is None:
        return x64
    s = stat.double()
    return ((x64 - s[0]) - s[1]) * s[2] + s[3]


def act64(z, act):
    if act == ACT_LEAKY_RELU:
        return torch.nn.functional.leaky_relu(z, 0.01)
    if act == ACT_SIGMOID:
        return torch.sigmoid(z)
    assert act == ACT_NONE
    return z


def reference(a, w, b, act, stat=None, slot_major=False, pre=None):
    """fp64 result, the magnitude sum |BN_in(a)| @ |W|^T + |b| of the bound, and the operands' maxima (fp16 floor).
    pre: the (z, mag, a_max, w_max) an earlier call with the same operands returned through pre_activation()."""
    z, mag, a_max, w_max = pre if pre is not None else pre_activation(a, w, b, stat, slot_major)
    return Ref(act64(z, act), mag, int(w.shape[1]), a_max, w_max)


def pre_activation(a, w, b, stat=None, slot_major=False):
    x = bn_in(flatten(a, slot_major).double(), stat)
    w64, b64 = w.double(), b.double()
    a_max = float(a.abs().max()) if a.numel() else 0.0
    return x @ w64.t() + b64, x.abs() @ w64.abs().t() + b64.abs(), a_max, float(w.abs().max())


def column_sums(y):
    """[2 m] fp64: column sums and sums of squares"""
    y = y.double()
    return torch.cat([y.sum(0), (y * y).sum(0)])


def ulp32(y64):
    """spacing of fp32 at |y| (normal range)"""
    _, e = torch.frexp(y64.abs().clamp(min=2.0 ** -126))
    return torch.ldexp(torch.ones_like(y64), e - 24)


def bound(ref, act, f16_pairs=False):
    bz = (ref.k + 8) * U32 * ref.mag
    if f16_pairs:
        bz = bz + ref.k * 2.0 ** -38 * ref.a_max * ref.w_max
    if act == ACT_SIGMOID:
        bz = bz + SIGMOID_ULPS * ulp32(ref.y)
    return bz


def measure(got, ref, act, f16_pairs=False):
    """(max-norm relative error, worst error / bound over all elements); NaN where `got` holds one"""
    err = (got.double() - ref.y).abs()
    bnd = bound(ref, act, f16_pairs)
    ratio = torch.where((err == 0) & (bnd == 0), torch.zeros_like(err), err / bnd.clamp(min=1e-300))
    return orc.rel_max_err(got, ref.y), float(ratio.max())


def gate_failures(got, ref, act, f16_pairs=False):
    """[] or what failed, as text.  Written so that a NaN fails."""
    if tuple(got.shape) != tuple(ref.y.shape):
        return ["shape %s, want %s" % (tuple(got.shape), tuple(ref.y.shape))]
    rel, ratio = measure(got, ref, act, f16_pairs)
    bad = []
    if not rel < REL_MAX_TOL:
        bad.append("max-norm error %.3e (gate %.0e)" % (rel, REL_MAX_TOL))
    if not ratio <= 1.0:
        err = (got.double() - ref.y).abs()
        over = torch.nonzero(~(err <= bound(ref, act, f16_pairs)))
        r, c = (int(v) for v in over[0])
        bad.append("element-wise: %d elements over the bound, worst %.3g x; first at row %d column %d: got %.9g want %.9g"
                   % (over.shape[0], ratio, r, c, float(got[r, c]), float(ref.y[r, c])))
    return bad


def partial_sum_ratio(rows, got):
    """The returned partial rows [n_partials, 2 m] (fp64) summed in fp64 against the fp64 sums of the fp32 values stored:
    worst |difference| / (PARTIAL_RTOL |sum|) over the 2 m entries."""
    want = column_sums(got)
    have = rows.double().sum(0)
    diff = (have - want).abs()
    ratio = torch.where(diff == 0, torch.zeros_like(diff), diff / (PARTIAL_RTOL * want.abs()).clamp(min=1e-300))
    return float(ratio.max())


def partial_failures(rows, n_partials, got, requested, out1_kernel=False):
    bad = []
    if not requested:
        return bad
    if out1_kernel:
        return [] if n_partials == 0 else ["n_partials %d from the out_dim == 1 kernel" % n_partials]
    if not 1 <= n_partials <= MAX_PARTIALS:
        return ["n_partials %d outside [1, %d]" % (n_partials, MAX_PARTIALS)]
    ratio = partial_sum_ratio(rows, got)
    if not ratio <= 1.0:
        bad.append("partial sums off by %.3g x rtol %.0e" % (ratio, PARTIAL_RTOL))
    return bad
