"""Case tables of the dense Linear op's tests (tests/test_dense_ops.py on the GPU, tests/test_dense_oracle_host.py on the CPU).

A plain module: the table of shapes by the kernel they are meant to reach, one seeded generator of inputs, and `dispatch`, a
restatement in Python of the conditions of dense_act_impl (csrc/dense.hip) -- the host test asserts case by case that every
case lands on the kernel its group names, and that every kernel named is reached.  Row counts are the smallest that reach each
code path (one row, one short of / one past a 128-row tile, more than one block, the grid caps, the swizzled grid of
dense_split_kernel at 8 row tiles, the 16 384-row threshold between its two tile shapes, the 49 152 rows where the rows kernels
begin)."""
from collections import namedtuple

import torch

from tests import dense_oracle as do

NONE, LEAKY, SIGMOID = do.ACT_NONE, do.ACT_LEAKY_RELU, do.ACT_SIGMOID
ROWS_KERNEL_MIN = 49152            # csrc/tgnn_common.h: kDenseRowsKernelMin
SPLIT_SMALL_ROWS = 16384           # dense_act_impl: small_rows

# kind: "plain" [N, K] row-major; "misaligned": the same, `a` one float past a 16-byte boundary; "slots": slot-major
# [S, N, C] through tgnn_dense_act_slots_fwd; "f16": slot-major through the fp16-pair ABI (f16_split = "tile" and True)
# shapes: (k, m) for plain kinds, (S, C, m) for slot kinds.  stats: the in_stat settings run; partials: the settings run
Group = namedtuple("Group", "name kind shapes rows acts stats partials kernels")

BOTH = (False, True)
GROUPS = [
    Group("out1", "plain", [(k, 1) for k in (4, 8, 16, 32, 64, 128, 256)], (1, 63, 257, 4099), (SIGMOID, NONE), BOTH, BOTH,
          {"out1<1>", "out1<2>", "out1<4>", "out1<8>", "out1<16>", "out1<32>", "out1<64>", "mfma<1,true>", "mfma<1,false>"}),
    # 8 200 rows x 64 lanes = 2 050 blocks of 256 threads: over the cap of 2 048, the grid-stride loop takes a second trip
    Group("out1-cap", "plain", [(256, 1)], (8200,), (SIGMOID, NONE), BOTH, BOTH, {"out1<64>", "mfma<1,true>"}),
    Group("out1-fallthrough", "plain", [(48, 1), (512, 1)], (1, 63, 257, 4099), (SIGMOID, NONE), BOTH, BOTH,
          {"mfma<1,true>", "mfma<1,false>"}),
    # 131 372 rows: 514 sweeps of 256 rows, over the 512 partial rows
    Group("in8", "plain", [(k, 32) for k in (1, 3, 5, 8)], (1, 31, 33, 1254, 131372), (LEAKY, NONE), (False,), BOTH, {"in8"}),
    Group("in8-fallthrough", "plain", [(9, 32), (3, 64), (3, 96), (3, 160)], (1, 31, 33, 1254), (LEAKY, NONE), BOTH, BOTH,
          {"mfma<1,false>", "mfma<2,false>", "mfma<4,false>", "mfma<8,false>"}),
    Group("mfma-fast", "plain", [(32, 32), (64, 32), (256, 17), (32, 48), (672, 33)], (1, 127, 129, 4099), (NONE, LEAKY, SIGMOID),
          BOTH, BOTH, {"mfma<1,true>", "mfma<2,true>"}),
    Group("mfma-slow", "plain", [(100, 96), (36, 200), (33, 129)], (129, 1254), (LEAKY, SIGMOID), BOTH, BOTH,
          {"mfma<4,false>", "mfma<8,false>"}),
    Group("mfma-misaligned", "misaligned", [(32, 32)], (129, 1254), (LEAKY, SIGMOID), BOTH, BOTH, {"mfma<1,false>"}),
    Group("split11", "plain", [(32, 64), (128, 64), (64, 72), (32, 200), (256, 128)], (1, 127, 129, 1024, 4099), (LEAKY, SIGMOID),
          BOTH, BOTH, {"split<1,1>"}),
    Group("split22", "plain", [(32, 128), (64, 200)], (16385, 17408), (LEAKY,), BOTH, BOTH, {"split<2,2>"}),
    Group("slots", "slots", [(5, 64, 64), (3, 96, 32), (3, 96, 128), (21, 32, 256)], (129, 4099), (LEAKY,), BOTH, BOTH,
          {"split<1,1>", "mfma<1,true>"}),
    Group("f16", "f16", [(s, 32, m) for s in (1, 2, 21) for m in (64, 96, 256)], (1, 129, 1024, 16385, 17408), (LEAKY, NONE),
          (False,), BOTH, {"split<1,1,f16>", "split<2,2,f16>"}),
]
# the rows kernels: [S, n, 32] -> m under tgnn_set_dense_rows_mode 2 (default), 0, 3, 6, 10
ROWS_GROUP = Group("rows", "f16", [(s, 32, m) for s in (1, 21) for m in (64, 128, 256)], (49152, 49279), (LEAKY,), (False,), BOTH,
                   {"rows<2>", "rows<4>", "rows<8>", "rows2<2>", "rows2<4>", "rows2<8>", "halves<8,4>",
                    "split<1,1,f16>", "split<2,2,f16>"})       # (the last two: the f16_split="tile" run each result is compared with)
ROWS_MODES = (2, 0, 3, 6, 10)
F16_VARIANTS = ("plain", "zero_slot", "zero", "big_slot")
BIG_SLOT = 2.0 ** 20


def shape_id(shape):
    return "x".join(str(v) for v in shape)


def group_shapes(groups=None):
    return [(g, s) for g in (groups if groups is not None else GROUPS) for s in g.shapes]


def shape_dims(group, shape):
    """(k, m, slot width or 0)"""
    if group.kind in ("slots", "f16"):
        s, c, m = shape
        return s * c, m, c
    return shape[0], shape[1], 0


def f16_modes(m):
    """f16_split values: the rows kernel's operand image exists for 64 / 128 / 256 outputs only"""
    return ("tile", True) if m in (64, 128, 256) else ("tile",)


def make_inputs(group, shape, n, stat=False, variant="plain"):
    """CPU tensors (a, w, b, stat record or None): seeded randn, weights scaled by k^-1/2; the record from random mean, var,
    gamma, beta in fp64 with the mean split hi / lo (tests/dense_oracle.py: stat_record).
    Outputs of up to 64 elements (one row, one column): the max-norm metric divides by max|want|, and a single dot product whose
    terms cancel (|z| = 0.02 of sum |x||w| happens) puts plain fp32 at the gate -- a property of the draw, not of a kernel.  Such
    a draw is repeated with the next seed until the fp64 pre-activation's largest value is an eighth of the largest magnitude
    sum; the element-wise gate does not care either way."""
    k, m, cw = shape_dims(group, shape)
    seed = 1_000_003 * k + 1009 * m + 31 * cw + n
    for attempt in range(32):
        g = torch.Generator().manual_seed(seed + 7919 * attempt)
        a = torch.randn(k // cw, n, cw, generator=g) if cw else torch.randn(n, k, generator=g)
        w = torch.randn(m, k, generator=g) * k ** -0.5
        b = torch.randn(m, generator=g)
        rec = None
        if stat:
            mean = 0.5 * torch.randn(k, generator=g, dtype=torch.float64)
            var = 0.25 + 2.0 * torch.rand(k, generator=g, dtype=torch.float64)
            gamma = 1.0 + 0.25 * torch.randn(k, generator=g, dtype=torch.float64)
            beta = 0.25 * torch.randn(k, generator=g, dtype=torch.float64)
            rec = do.stat_record(mean, var, gamma, beta)
        if n * m > 64:
            break
        z, mag, _, _ = do.pre_activation(a, w, b, rec, bool(cw))
        if float(z.abs().max()) >= float(mag.max()) / 8:
            break
    else:
        raise AssertionError("no well-conditioned draw for %s %s n %d" % (group.name, shape, n))
    return apply_variant(a, variant), w, b, rec


def near_constant_case(n=1254, k=32, m=32, seed=5):
    """v = 1000 + 2^-10 randn, the record from fp64 statistics of v: the BatchNorm's output is of order one, the low half of
    the mean is up to 2^-25 * 1000 = 3e-5 = 0.03 standard deviations"""
    g = torch.Generator().manual_seed(seed)
    v = (1000.0 + 2.0 ** -10 * torch.randn(n, k, generator=g, dtype=torch.float64)).float()
    v64 = v.double()
    rec = do.stat_record(v64.mean(0), v64.var(0, unbiased=False), torch.ones(k, dtype=torch.float64),
                         torch.zeros(k, dtype=torch.float64))
    w = torch.randn(m, k, generator=g) * k ** -0.5
    return v, w, torch.randn(m, generator=g), rec


def apply_variant(a, variant):
    """slot-major a [S, n, C]: one all-zero slot (the middle one), the whole input zero, slot 0 at 2^20 times the others"""
    if variant == "plain":
        return a
    a = a.clone()
    if variant == "zero_slot":
        a[a.shape[0] // 2] = 0
    elif variant == "zero":
        a.zero_()
    else:
        assert variant == "big_slot"
        a[0] *= BIG_SLOT
    return a


def f16_variants(shape):
    return tuple(v for v in F16_VARIANTS if not (shape[0] == 1 and v == "zero_slot"))     # (one slot: "zero" is that case)


def dispatch(kind, k, m, n, cw=0, stat=False, partials=False, f16=False, wimg=False, rows_mode=2):
    """The kernel dense_act_impl picks, from its conditions (csrc/dense.hip), for torch-allocated (256-byte aligned) operands."""
    aligned = kind != "misaligned"
    lda, akb, kps = (cw, n * cw, cw // 32) if cw else (k, 32, 1)
    vec_a = lda % 4 == 0 and akb % 4 == 0 and aligned
    if m == 1 and not partials and kps == 1 and akb == 32 and vec_a and 4 <= k <= 256 and k & (k - 1) == 0:
        return "out1<%d>" % (k // 4)
    if k <= 8 and m == 32 and not stat and kps == 1:
        return "in8"
    fast = vec_a and k % 4 == 0 and k % 32 == 0
    if fast and m >= 64 and lda % 8 == 0 and akb % 8 == 0 and k % 8 == 0:
        if f16 and wimg and n >= ROWS_KERNEL_MIN and m in (64, 128, 256) and (not stat or k <= 1024):
            tn = m // 32                  # (the resident kernels need in_stat: not reachable through the fp16-pair ABI)
            if tn == 8 and (rows_mode >> 2) & 3 and not stat and kps == 1:
                return "halves<8,4>"
            if rows_mode & 1 and kps == 1:
                return "rows2<%d>" % tn
            return "rows<%d>" % tn
        tile = "2,2" if m > 64 and n > SPLIT_SMALL_ROWS else "1,1"
        return "split<%s%s>" % (tile, ",f16" if f16 else "")
    nt = 8 if m > 128 else 4 if m > 64 else 2 if m > 32 else 1
    return "mfma<%d,%s>" % (nt, "true" if fast else "false")


def expected_partial_rows(kernel, n, cus=None):
    """n_partials by kernel: one partial row per block.  A block per 256 rows (dense_in8_kernel) or per 128-row tile (the
    block-tile kernels), capped at TGNN_BN_MAX_PARTIALS; the rows kernels are capped by the chip -- two blocks per compute unit
    (dense_f16_rows_kernel), one (rows2), one or two per unit over 2 items per tile, an even count (halves: `cus` is then
    blocks-per-unit x units) -- so each of them returns another count: what tells the test which one ran.  None: not known."""
    tiles = max(1, -(-n // 128))
    if kernel == "in8":
        return min(do.MAX_PARTIALS, max(1, -(-n // 256)))
    if kernel.startswith(("mfma", "split")):
        return min(do.MAX_PARTIALS, tiles)
    if cus is None:
        return None
    if kernel.startswith("rows2"):
        return min(do.MAX_PARTIALS, tiles, cus)
    if kernel.startswith("rows"):
        return min(do.MAX_PARTIALS, tiles, 2 * cus)
    assert kernel.startswith("halves")
    return min(do.MAX_PARTIALS, 2 * tiles, cus) & ~1


def group_kernels(group, rows_cap=None, modes=(2,)):
    """every kernel the group's cases reach, by `dispatch` (rows above rows_cap left out: the host test's view)"""
    seen = set()
    for shape in group.shapes:
        k, m, cw = shape_dims(group, shape)
        for n in group.rows:
            if rows_cap and n > rows_cap:
                continue
            for stat in group.stats:
                for partials in group.partials:
                    if group.kind == "f16":
                        for mode in f16_modes(m):
                            for rm in modes:
                                seen.add(dispatch(group.kind, k, m, n, cw, stat, partials, True, mode is True, rm))
                    else:
                        seen.add(dispatch(group.kind, k, m, n, cw, stat, partials))
    return seen
