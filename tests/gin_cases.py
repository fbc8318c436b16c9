"""Case tables of the GINConv op's tests (tests/test_gin32_ops.py on the GPU, tests/test_gin_cases_host.py on the CPU).

A plain module: the row counts with the reason each is there, seeded generators of edges, weights, rows and BatchNorm records,
the references (the fp64 oracle, and the oracle evaluated in fp32 by torch: the floor a correct fp32 kernel stands on), and
`dispatch`, a restatement in Python of the conditions of tgnn_gin_fwd / tgnn_gin32_fwd (csrc/gin.hip, csrc/gin32_plan.h) -- the
host test asserts case by case that every case lands on the kernel it names, and that every kernel named is reached."""
import functools
from collections import namedtuple

import torch

from oracle import tilingnn_oracle as orc

PREFIX = "c"
GATE = 1e-6                 # of the output's max-norm: the project's gate for this op (tests/test_gin_fused.py, test_gin64_mfma.py)
F32_FLOOR = 5e-7            # what the fp32 torch evaluation of the oracle must stay within at unit scale (the host test)
DEVICE_CUS = 256            # MI355X; the width-32 kernels leave 32 CUs to the other chain: at most 224 blocks
VARIANTS = {0: "bf16x3", 1: "f16", 2: "fused"}               # tgnn_gin32_fwd's variant -> ops.gin's kernel=

AGG, MLP, MLP16, FUSED, GENERIC = ("gin_aggregate_kernel<32>", "gin32_mlp_kernel", "gin32_mlp16_kernel", "gin32_fused_kernel",
                                   "gin_generic_kernel")
KERNELS = (AGG, MLP, MLP16, FUSED, GENERIC)

# row count -> why it is there (blocks: one per 128 rows, at most 224, from 8 on a multiple of 8)
ROW_COUNTS = {
    1: "empty XCD ranges in the aggregate (n x / 8), one partial tile",
    7: "empty XCD ranges in the aggregate",
    9: "XCD ranges of 1 and 2 rows",
    16: "one full tile",
    17: "tile tail: one row in the second tile",
    37: "tile tail, 3 tiles on 8 waves",
    200: "2 blocks",
    800: "7 blocks: the last count without the XCD swizzle",
    1000: "8 blocks: swizzle on; the first size with the hub row",
    2000: "16 blocks: 16 BatchNorm fold groups of one",
    3000: "24 blocks: fold groups of 2 and 1",
    1254: "the labyrinth layout's own collision edges",
    30000: "224 blocks: the cap",
    66003: "waves walk 2 - 3 tiles",
}
FUSED_ONLY_ROW_COUNTS = {200003: "the fused form's default regime: every slot of its hand-over ring is reused twice"}
MAGNITUDES = (1e-3, 1.0, 1e3)
# (W2, W3) scales of the fp16-pair kernel's power-of-two scaling; the last two leave plain fp32 over the gate (see the tests)
WEIGHT_SCALES = ((2.0 ** -12, 1.0), (1.0, 2.0 ** -12), (0.0, 1.0), (1.0, 0.0), (16.0, 1.0), (1.0, 16.0))
WEIGHT_SCALE_ROWS = (37, 1000, 4099)
GENERIC_WIDTHS = (8, 48, 64, 96, 256)
GENERIC_ROWS = (1, 5, 1254)
FORWARD_ROWS = (17, 200, 800, 1000, 2000, 3000)             # the in-kernel BatchNorm fold at 1, 2, 7, 8, 16, 24 blocks


def gin32_blocks(n, cap=DEVICE_CUS - 32):
    b = min(max((n + 127) // 128, 1), 512, cap)
    return b & ~7 if b >= 8 else b


def dispatch(c, n, lda, aligned, variant):
    """-> (kernels launched, blocks of the last one).  variant: None = tgnn_gin_fwd (ops.gin(kernel=None)), 0 / 1 / 2 =
    tgnn_gin32_fwd with LeakyReLU (which refuses: -> ("refused",), 0 -- instead of falling back)."""
    fast = c == 32 and lda % 4 == 0 and aligned
    if variant is None:
        if fast:
            return (AGG, MLP), gin32_blocks(n)
        return (GENERIC,), min(max((n + 3) // 4, 1), 512)
    if not fast or n * 128 >= 2 ** 31 or (variant != 0 and lda != 32):
        return ("refused",), 0
    return {0: (AGG, MLP), 1: (AGG, MLP16), 2: (FUSED,)}[variant], gin32_blocks(n)


def forward_default_variant(n):
    """The form tgnn_forward runs at width 32 with no switch touched (gin32_plan.h: gin32_variant, fused mode 1, fp16 off)."""
    return 2 if n >= 200000 else 0


Case = namedtuple("Case", "group c n lda aligned variant kernels")
CASES = (
    [Case("op", 32, n, 32, True, v, {0: (AGG, MLP), 1: (AGG, MLP16), 2: (FUSED,)}[v]) for v in VARIANTS for n in ROW_COUNTS]
    + [Case("op", 32, n, 32, True, 2, (FUSED,)) for n in FUSED_ONLY_ROW_COUNTS]
    + [Case("default", 32, n, 32, True, None, (AGG, MLP)) for n in (37, 1254)]
    + [Case("scales", 32, n, 32, True, v, {0: (AGG, MLP), 1: (AGG, MLP16)}[v]) for v in (0, 1) for n in WEIGHT_SCALE_ROWS]
    + [Case("lda36", 32, n, 36, True, None, (AGG, MLP)) for n in (37, 1254)]
    + [Case("halo", 32, n, 32, True, None, (AGG, MLP)) for n in (37, 1254)]
    + [Case("lda33", 32, n, 33, True, None, (GENERIC,)) for n in (37, 1254)]
    + [Case("misaligned", 32, n, 32, False, None, (GENERIC,)) for n in (37, 1254)]
    + [Case("generic", c, n, c, True, None, (GENERIC,)) for c in GENERIC_WIDTHS for n in GENERIC_ROWS]
)


# ---------------------------------------------------------------------------------------------- inputs
@functools.lru_cache(maxsize=None)
def collision_edges(n, seed):
    """[2, E] int64 on the CPU.  1 254: the labyrinth layout's collision edges.  Else 3 n random edges, the first 4 turned into
    self loops (the CSR drops them), rows n - 7 .. n - 1 without in-edges (n > 16), and from 1 000 nodes on 500 edges into row 5."""
    if n == 1254:
        from tests.golden_util import graph_tensors, load_labyrinth_graph
        return graph_tensors(load_labyrinth_graph(), torch.float32, "cpu")[3]
    g = torch.Generator().manual_seed(seed)
    e = 3 * n
    src = torch.randint(0, n, (e,), generator=g)
    dst = torch.randint(0, n - 7 if n > 16 else n, (e,), generator=g)
    k = min(4, e)
    src[:k] = dst[:k]                                        # self loops
    if n >= 1000:
        src = torch.cat([src, torch.randint(0, n, (500,), generator=g)])
        dst = torch.cat([dst, torch.full((500,), 5)])
    return torch.stack([src, dst])


def gin_weights(ei, n, seed, width, in_scale=1.0, w2_scale=1.0, w3_scale=1.0):
    """State-dict entries of one GINConv (fp32, CPU) for rows of magnitude in_scale: the recipe of
    tests/test_gin64_mfma.py::gin_weights at any width.  W1 ~ 0.25 sqrt(64 / width) / (in_scale sqrt(1 + mean in-degree)): `width`
    inputs of variance in_scale^2 ((1 + eps)^2 + degree) give layer 1's pre-activations a standard deviation of ~2 -- the first
    sigmoid is not saturated, and sum_k |W1_k z_k| is of order 1 - 10, where the gate of 1e-6 says something about a kernel (the
    docstring there).  w2_scale / w3_scale multiply W2 / W3 (not the biases)."""
    g = torch.Generator().manual_seed(seed)
    keep = ei[0] != ei[1]
    mean_deg = float(keep.sum()) / n
    s1 = 0.25 * (64.0 / width) ** 0.5 / (in_scale * (1.0 + mean_deg) ** 0.5)
    return {f"{PREFIX}.ginConv.eps": torch.tensor([0.25]),
            f"{PREFIX}.ginConv.nn.mlp.0.linear.weight": torch.randn(32, width, generator=g) * s1,
            f"{PREFIX}.ginConv.nn.mlp.0.linear.bias": torch.randn(32, generator=g) * 0.3,
            f"{PREFIX}.ginConv.nn.mlp.1.linear.weight": torch.randn(64, 32, generator=g) * 0.4 * w2_scale,
            f"{PREFIX}.ginConv.nn.mlp.1.linear.bias": torch.randn(64, generator=g) * 0.3,
            f"{PREFIX}.ginConv.nn.mlp.2.linear.weight": torch.randn(width, 64, generator=g) * 0.4 * w3_scale,
            f"{PREFIX}.ginConv.nn.mlp.2.linear.bias": torch.randn(width, generator=g) * 0.3}


def param_list(sd):
    """eps, w1, b1, w2, b2, w3, b3: the order of ops.gin."""
    return [sd[f"{PREFIX}.ginConv.eps"]] + [sd[f"{PREFIX}.ginConv.nn.mlp.{i}.linear.{k}"] for i in range(3) for k in ("weight", "bias")]


def bn_record(a, seed):
    """A BatchNorm record [4][C] fp32 of the rows `a` (mean hi, mean lo, gamma / sqrt(var + eps), beta) with random gamma / beta
    (1 + 0.3 r, 0.2 r, as tests/test_training_width64.py::_bn draws them), from fp64 batch statistics."""
    c = a.shape[1]
    g = torch.Generator().manual_seed(seed)
    gamma, beta = 1 + 0.3 * torch.randn(c, generator=g), 0.2 * torch.randn(c, generator=g)
    a64 = a.double()
    mean = a64.mean(0)
    var = ((a64 - mean) ** 2).mean(0)
    hi = mean.float()
    lo = (mean - hi.double()).float()
    ginv = (gamma.double() / torch.sqrt(var + 1e-5)).float()
    return torch.stack([hi, lo, ginv, beta]).contiguous()


def apply_record(a, stat, dtype):
    """The BatchNorm the record describes, as the kernels apply it: ((a - hi) - lo) * ginv + beta."""
    s = stat.to(dtype)
    return ((a.to(dtype) - s[0]) - s[1]) * s[2] + s[3]


def layer1_unsaturated_share(x64, ei, sd64):
    """From the oracle's arithmetic alone: the share of layer 1's pre-activations with |v| < 4."""
    keep = ei[0] != ei[1]
    z = (1.0 + sd64[f"{PREFIX}.ginConv.eps"]) * x64 + torch.zeros_like(x64).index_add_(0, ei[1][keep], x64[ei[0][keep]])
    v = orc.linear(z, sd64, f"{PREFIX}.ginConv.nn.mlp.0.linear")
    return float((v.abs() < 4).double().mean())


Problem = namedtuple("Problem", "n width ei a stat sd want share f32_err")


@functools.lru_cache(maxsize=None)
def problem(n, width=32, with_stat=False, scale=1.0, w2_scale=1.0, w3_scale=1.0):
    """One op call's inputs and references, computed once per process and shared by the tests (treat as read-only):
    rows a = scale * randn (+ 0.3 scale behind a record), the record or None, the weights (W1 follows the magnitude of what the MLP
    sees: behind a record that is 1 whatever the magnitude of `a`), want = the fp64 oracle's GINConv WITHOUT LeakyReLU, the share of
    unsaturated layer-1 pre-activations, and the max-norm error of the same oracle evaluated in fp32 by torch."""
    ei = collision_edges(n, n)
    gen = torch.Generator().manual_seed(n + 2)
    base = torch.randn(n, width, generator=gen)
    a = base * scale + (0.3 * scale if with_stat else 0.0)
    stat = bn_record(a, 4) if with_stat else None
    sd = gin_weights(ei, n, n + 1, width, 1.0 if with_stat else scale, w2_scale, w3_scale)
    sd64 = orc.cast_sd(sd, torch.float64)
    x64 = apply_record(a, stat, torch.float64) if with_stat else a.double()
    x32 = apply_record(a, stat, torch.float32) if with_stat else a
    with torch.no_grad():
        want = orc.gin_conv(x64, ei, sd64, PREFIX)
        got32 = orc.gin_conv(x32, ei, sd, PREFIX)
    return Problem(n, width, ei, a, stat, sd, want, layer1_unsaturated_share(x64, ei, sd64), orc.rel_max_err(got32, want))
