"""Case tables, generators, fp64 reference and gates of the NNConv op's tests at width 32 (tests/test_nnconv32_ops.py on the GPU,
tests/test_nnconv_cases_host.py on the CPU).  A plain module, no GPU import.

The op (GraphConv.forward of the reference, PyG NNConv with aggr="mean"):
    out[v] = 1 / max(deg_v, 1) * sum_{e: dst_e = v} h[src_e] @ W[type_e]  +  h[v] @ root  +  bias      (+ LeakyReLU)
`dispatch` restates in Python which kernel a call lands on and with how many blocks (ops.nnconv_mean, tgnn_nnconv_mean_fwd,
tgnn_nnconv_mean_cols(_f16)_fwd, launch_nnconv_cols, launch_cols_t, launch_nnconv_eg); `graph` builds a multigraph whose
in-degree profile is prescribed row class by row class; `reference` is the fp64 expectation with what the gates need.

Two gates, both on every element of every case, a NaN fails both:
  * the project's max-norm gate  max|got - want| / max|want| < 2e-6  (dense_oracle.REL_MAX_TOL, tests/test_nnconv_eg.py);
  * element-wise  |got - want| <= gamma_v * mag[v, o] + floor[v, o],   gamma_v = (c (deg_v + 1) + c0) * 2^-24,
        mag = 1 / max(deg, 1) * sum_e |h[src_e]| @ |W[type_e]| + |h[v]| @ |root| + |bias|.
    c (deg_v + 1) u is the bound of row v's dot product of length c (deg_v + 1) -- every in-edge and the root term -- summed in
    fp32 in ANY order (u = 2^-24; first order).  It is taken to cover every addition on the way to the accumulator: the chains of
    the CSR kernels (16 multiply-adds per half row, one per item, two cross-lane adds), the pre-add of same-type columns in the
    column kernel (deg_v - 1 additions at most) and the sums of the matrix pipe.  For the matrix pipe that is a statement about
    the hardware: a run of one type costs 6 (bf16 x 3) or 3 (fp16 pair) instructions of K = 32 on one accumulator, so the part
    covers them as long as an instruction rounds its accumulator no more than 5 (10) times; the pieces' products are exact in
    fp32 (8 x 8 and 11 x 11 significand bits).  The measured ratios (profiles/nnconv32_ops_errors.txt) say how far inside the
    kernels are.
    c0, per form, counts the roundings that are NOT additions of that dot product, in units of u relative to mag:
    LeakyReLU counts 2 everywhere: its product's rounding (1) and the fp32 slope 0.01f, 2.2e-8 = 0.37 u off the reference's 0.01.
      csr (nnconv32_lds_kernel, nnconv_generic_kernel)                                                              c0 = 6
          the generic kernel, the longer of the two: 1 / max(deg, 1) as a rounded reciprocal (1), its product with the edge
          sum (1), the root term joining the mean (1), the bias (1), LeakyReLU (2) = 6.  (The LDS kernel folds the reciprocal
          into its multiply-adds and the root term into the chain: 1 + 1 + 2 = 4.)  torch's fp32 evaluation of the oracle: the
          quotient (1), the two additions (2), LeakyReLU (2) = 5.
      cols (nnconv32_cols_kernel, bf16 x 3)                                                                         c0 = 8
          the summed rows and the weights split EXACTLY into three bf16 pieces (3 x 8 = 24 significand bits, truncating, the
          exponent range of fp32); of the nine cross terms the kernel drops mid.lo, lo.mid (2^-8 2^-16 = 1 u each) and lo.lo
          (2^-32): 2 + 2^-8; the root row's product with max(deg, 1) (1), unscale / max(deg, 1) (1), the multiply-add that
          applies it and adds the bias (1), LeakyReLU (2) = 7 + 2^-8, rounded up.
      cols_f16 (nnconv32_cols_kernel, fp16 pair)                                                                    c0 = 17
          an operand x scaled by a power of two s is kept as hi = RN16(s x), lo = RN16(s x - hi): to 2^-22 |s x| where lo is
          a normal fp16, to 2^-25 absolute where it is not (the floor below).  Summed rows 2^-22, weights 2^-22, the dropped
          lo.lo term 2^-22: 3 * 2^-22 = 12 u; then as cols: the root row's product (1), the quotient (1), the multiply-add (1),
          LeakyReLU (2) = 17; the second-order terms are below 2^-40.
      eg (nnconv32_eg_kernel, fp16 pairs twice)                                                                     c0 = 21
          gathered rows 2^-22, weights 2^-22, lo.lo 2^-22, and the messages M = G . W split once more into an fp16 pair for the
          second product, 2^-22 of |M| <= |G| @ |W|: 4 * 2^-22 = 16 u; the selection matrix (0 / 1, max(deg, 1) <= 2 048 on the
          root group's diagonal) is exact in fp16 and so are its products; v_rcp_f32 (1 ulp = 2 u) times the exact power of two
          (0), the multiply-add (1), LeakyReLU (2) = 21.
    floor (the fp16 forms only): where an fp16 piece is subnormal the pair keeps s x to 2^-25 absolute, that is 2^-25 / s of x.
      Summed over a row's terms -- each pairs one operand's absolute error with the other operand's magnitude --
          floor[v, o] = 2^-25 * ( B1[v, o] / sx  +  A1[v] / sw )          (+ 2 * 2^-25 / (sx sw) for eg: the message split)
          B1 = 1 / max(deg, 1) * sum_e sum_k |W[type_e][k, o]| + sum_k |root[k, o]|,   A1 = 1 / max(deg, 1) * sum_e |h[src_e]|_1 + |h[v]|_1
      (the column kernel splits the SUM of a type's rows, and the root row times max(deg, 1): one error of 2^-25 / sx per run
      instead of one per edge, and B1 counts one per edge: an upper bound), with the scales of the kernels' own rules:
          cols_f16:  sx = pow2_scale_for(max|h|, ceil log2 of the in-degree bound handed in),  sw = nnconv_weight_scale(max|root|)
          eg:        sx = pow2_scale_for(max|h|, 5), or 1 where 2^3 <= max|h| < 2^10;          sw = nnconv_weight_scale(max|root|) * 2^-15
      (kEgImageScale = 2^-15 keeps every weight below 1 so that a message stays below 2^15; the message split works in units of
      1 / (sx sw), once per edge and once for the root group, whose factor max(deg, 1) the final quotient takes off again).
      This is dense_oracle's  K * 2^-38 * max|a| * max|W|  with the sums written out instead of bounded by K maxima.
Both c0 and the floor come from the kernels' arithmetic, none from a measurement.  The fp64 oracle evaluated in fp32 by torch
stands inside the csr bound (the host test): a correct fp32 implementation passes before a kernel is asked to."""
import functools
import math
from collections import namedtuple

import numpy as np
import torch

from oracle import tilingnn_oracle as orc
from tests import dense_oracle as do

U32 = do.U32
REL_MAX_TOL = do.REL_MAX_TOL
DEVICE_CUS = 256                       # MI355X; the tiled kernels leave 32 CUs to the other chain of the forward
MAX_PARTIALS = do.MAX_PARTIALS         # TGNN_BN_MAX_PARTIALS (producer_blocks, tgnn_common.h)
COLS_MAX_TYPES = 22                    # tgnn_nnconv_cols_max_types(): (163 584 / 4 - 16 * 320) / 1 536 - 1
LDS_MAX_TYPES = 30                     # nnconv32_lds_kernel: (T + 1) * 5 120 B <= 163 584 B
EG_MAX_IN_DEGREE = 2048

COLS8, COLS16, COLS16F, EG, LDS, GENERIC = ("nnconv32_cols_kernel<8 waves>", "nnconv32_cols_kernel<16 waves>",
                                            "nnconv32_cols_kernel<16 waves, F16>", "nnconv32_eg_kernel", "nnconv32_lds_kernel",
                                            "nnconv_generic_kernel")
KERNELS = (COLS8, COLS16, COLS16F, EG, LDS, GENERIC)
FAST = {COLS8: (True, False), COLS16: (True, False), COLS16F: (True,)}    # FAST = packed rows (ldh == 32); the fp16-pair entry
#                                                                           point refuses any other stride, so <F16, FAST=false>
#                                                                           is compiled and never launched
FORMS = ("cols", "cols_f16", "eg", "csr")                                 # ops.nnconv_mean's kernel=
C0 = {"csr": 6, "cols": 8, "cols_f16": 17, "eg": 21}                       # derived in the module docstring

# row count -> why it is there (tiled kernels: 16-row tiles, 4 per block; nnconv32_lds_kernel: 16 rows per block)
ROW_COUNTS = {
    1: "one lane-row of one tile, 15 of 16 share slots empty",
    15: "tile tail: one row short of a tile",
    16: "one full tile",
    17: "tile tail: one row in the second tile",
    64: "one block, one tile per SIMD slot",
    65: "2 blocks, the second with one row; CSR: 5 blocks",
    129: "3 blocks; CSR: 9 blocks -> 8, the XCD row split switches on",
    513: "33 tiles -> 9 blocks -> 8: the round-down and the XCD swizzle switch on together",
    1254: "the labyrinth layout's size: 79 tiles, 20 -> 16 blocks",
    4099: "CSR: 257 blocks -> 256, its cap; the largest size of the host test's fp32 evaluation",
    14337: "first size past the 16-wave cap (224 blocks of 4 x 16 rows): waves walk more than one tile",
    28673: "the same for the 8-wave form (448 blocks)",
    66003: "waves walk 2 - 5 tiles; the benchmark's order of magnitude",
}
OP_TYPES = 13                          # the labyrinth layout's type count: what the row-count cases run at

# edge types at 1 254 rows -> the kernel each kernel= lands on ("refused": ValueError)
TYPE_COUNTS = {
    0: {"cols": COLS8, "cols_f16": "refused", "eg": "refused", "csr": LDS},     # no adjacency edge at all: in-degree bound 0
    1: {"cols": COLS8, "cols_f16": COLS16F, "eg": EG, "csr": LDS},
    10: {"cols": COLS8, "cols_f16": COLS16F, "eg": EG, "csr": LDS},             # last with two 8-wave blocks per CU
    11: {"cols": COLS16, "cols_f16": COLS16F, "eg": EG, "csr": LDS},
    16: {"cols": COLS16, "cols_f16": COLS16F, "eg": EG, "csr": LDS},
    17: {"cols": COLS16, "cols_f16": COLS16F, "eg": EG, "csr": LDS},
    22: {"cols": COLS16, "cols_f16": COLS16F, "eg": EG, "csr": LDS},            # last in the LDS image
    23: {"cols": "refused", "cols_f16": "refused", "eg": "refused", "csr": LDS},
    30: {"cols": "refused", "cols_f16": "refused", "eg": "refused", "csr": LDS},   # last LDS table
    31: {"cols": "refused", "cols_f16": "refused", "eg": "refused", "csr": GENERIC},
    300: {"cols": "refused", "cols_f16": "refused", "eg": "refused", "csr": GENERIC},
}
TYPE_ROWS = 1254
MAGNITUDES = (1e-3, 1.0, 1e3)
ROOT_SCALES = (2.0 ** -12, 0.3, 16.0)
TABLES = ("rand", "zeros", "ones")     # (0, 1); every entry exactly 0.0; exactly 1.0f (a saturated fp32 sigmoid)
MAGNITUDE_ROWS = (1254, 14337)
GENERIC_WIDTHS = (8, 48, 64, 96, 256)
GENERIC_ROWS = (1, 5, 1254)
STRIDES = (36, 40)
GUARD_ROWS = (1, 17, 65, 1254)
REPEAT_ROWS = (513, 14337)
CAP_ROWS, BLOCK_CAPS = 2000, (1, 7, 8, 9)
HALO = 50


def tiled_blocks(n, blocks_per_cu=1, debug_cap=0, eg=False, cus=DEVICE_CUS):
    """launch_cols_t / launch_nnconv_eg: one block per 4 tiles of 16 rows, at most (CUs - 32) x blocks per CU (tgnn_debug_set_
    block_caps: min(cap, CUs) x blocks per CU for the column kernel, min(cap, CUs) for the groups), from 8 on a multiple of 8."""
    b = -(-(-(-n // 16)) // 4)
    left = cus - 32
    cap = (left if left > cus // 4 else max(cus // 4, 1)) * blocks_per_cu
    if debug_cap > 0:
        cap = min(debug_cap, cus) * (1 if eg else blocks_per_cu)
    b = min(b, cap)
    if b >= 8:
        b &= ~7
    return max(b, 1)


def producer_blocks(n_rows, rows_per_block):
    """tgnn_common.h: producer_blocks"""
    return min(max(-(-n_rows // rows_per_block), 1), MAX_PARTIALS)


def lds_blocks(n):
    """tgnn_nnconv_mean_fwd, nnconv32_lds_kernel: one row per wave of 16, at most 256 blocks, from 8 on a multiple of 8"""
    b = min(producer_blocks(n, 16), 256)
    return b & ~7 if b >= 8 else b


def dispatch(c, n, T, ldh, max_in_degree, kernel, groups=False, debug_cap=0):
    """-> (kernel name, FAST, blocks) or ("refused", why, 0).  kernel: ops.nnconv_mean's kernel=; max_in_degree: the layout's
    (cols_f16: the bound handed in).  groups: the layout was prepared with edge groups (kernel=None only; a layout prepared
    without the column structure and without groups goes to the CSR kernels, which is not restated here)."""
    if kernel not in (None,) + FORMS:
        return "refused", "unknown kernel", 0
    if kernel is None:
        if groups and c == 32 and T <= COLS_MAX_TYPES and 1 <= max_in_degree <= EG_MAX_IN_DEGREE and n * 128 < 2 ** 31:
            kernel = "eg"
        elif c == 32 and T <= COLS_MAX_TYPES and n * 128 < 2 ** 31:
            kernel = "cols"
        else:
            kernel = "csr"
    if kernel in ("eg", "cols", "cols_f16"):
        if c != 32:
            return "refused", "width 32", 0
        if T > COLS_MAX_TYPES:
            return "refused", "edge types", 0
        if n * 128 >= 2 ** 31:
            return "refused", "2 GB", 0
    if kernel == "eg":
        if not 1 <= max_in_degree <= EG_MAX_IN_DEGREE:
            return "refused", "in-degree", 0
        if ldh != 32:
            return "refused", "packed rows", 0
        return EG, None, tiled_blocks(n, 1, debug_cap, eg=True)
    if kernel == "cols_f16":
        if max_in_degree < 1:
            return "refused", "in-degree", 0
        if ldh != 32:
            return "refused", "packed rows", 0
        return COLS16F, True, tiled_blocks(n, 1, debug_cap)
    if kernel == "cols":
        if ldh < 32 or ldh % 4:
            return "refused", "alignment", 0
        # two 8-wave blocks per CU while two images fit: ((T + 1) * 6 144 + 8 * 1 280) * 2 <= 160 KiB, that is T <= 10
        if ((T + 1) * 6144 + 8 * 1280) * 2 <= 160 * 1024:
            return COLS8, ldh == 32, tiled_blocks(n, 2, debug_cap)
        return COLS16, ldh == 32, tiled_blocks(n, 1, debug_cap)
    if ldh < c:
        return "refused", "ldh", 0
    if c == 32 and (T + 1) * 5120 <= 160 * 1024 - 256:
        return LDS, None, lds_blocks(n)
    if c > 256:
        return "refused", "width", 0
    return GENERIC, None, producer_blocks(n, 256 // c)


Case = namedtuple("Case", "group form c n T ldh kernel fast")


def _named(form, T):
    return TYPE_COUNTS[T][form] if T in TYPE_COUNTS else {"cols": COLS16, "cols_f16": COLS16F, "eg": EG, "csr": LDS}[form]


def _fast(name, ldh):
    return (ldh == 32) if name in FAST else None


# the GPU tests' parametrisation: every case names the kernel it is there for (the host test holds `dispatch` against the names)
CASES = (
    [Case("rows", f, 32, n, OP_TYPES, 32, _named(f, OP_TYPES), _fast(_named(f, OP_TYPES), 32)) for f in FORMS for n in ROW_COUNTS]
    + [Case("types", f, 32, TYPE_ROWS, T, 32, TYPE_COUNTS[T][f], _fast(TYPE_COUNTS[T][f], 32)) for f in FORMS for T in TYPE_COUNTS]
    + [Case("magnitudes", f, 32, n, OP_TYPES, 32, _named(f, OP_TYPES), _fast(_named(f, OP_TYPES), 32)) for f in FORMS for n in MAGNITUDE_ROWS]
    + [Case("strides", "cols", 32, n, T, ldh, k, False) for ldh in STRIDES for n, T, k in ((65, 10, COLS8), (1254, 10, COLS8),
                                                                                         (65, 13, COLS16), (1254, 13, COLS16))]
    + [Case("strides", "csr", 32, n, T, ldh, k, None) for ldh in STRIDES for n, T, k in ((65, 13, LDS), (1254, 13, LDS), (1254, 31, GENERIC))]
    + [Case("guard", f, 32, n, OP_TYPES, 32, _named(f, OP_TYPES), _fast(_named(f, OP_TYPES), 32)) for f in FORMS for n in GUARD_ROWS]
    + [Case("halo", f, 32, n, OP_TYPES, 32, _named(f, OP_TYPES), _fast(_named(f, OP_TYPES), 32)) for f in ("cols", "cols_f16", "csr")
       for n in (65, 1254)]
    + [Case("repeat", f, 32, n, OP_TYPES, 32, _named(f, OP_TYPES), _fast(_named(f, OP_TYPES), 32)) for f in FORMS for n in REPEAT_ROWS]
    + [Case("caps", f, 32, CAP_ROWS, T, 32, k, _fast(k, 32)) for f, T, k in (("cols", 10, COLS8), ("cols", 13, COLS16), ("cols_f16", 13, COLS16F),
                                                                    ("eg", 13, EG))]
    + [Case("widths", "csr", c, n, 3 if c == 256 else OP_TYPES, c, GENERIC, None) for c in GENERIC_WIDTHS for n in GENERIC_ROWS]
)


# ---------------------------------------------------------------------------------------------- the graph
Graph = namedtuple("Graph", "n n_src T src dst typ deg rows attr")
# row class -> in-degree (None: depends on n / T); small layouts take them in this order while rows last
_CLASSES = (("deg17", 17), ("deg15", 15), ("deg16", 16), ("deg1", 1), ("deg14", 14), ("deg33", 33), ("hub", None),
            ("distinct", None), ("dup", 3), ("self", 3), ("from_first", 5), ("from_last", 5), ("from_halo", 4))


def hub_degree(n):
    return min(700, n // 2)


@functools.lru_cache(maxsize=None)
def graph(n, T, seed, halo=0, hub=None):
    """A directed multigraph on n destination rows (sources: n + halo rows), CPU int64 tensors in destination order, whose
    in-degrees are PRESCRIBED: the seed draws sources only.  Row classes, each present when a row is left for it (rows: class ->
    row), types cycling 0, 1, ... within a row unless said otherwise:
      deg0_tile    rows 16 .. 31 without in-edges (n >= 48): a tile with the root column only;   deg0_last: row n - 1 (n >= 2)
      deg1, deg14, deg15, deg16, deg17, deg33: that many in-edges (nnconv32_lds_kernel pipelines 15 and loops over the rest)
      hub          min(700, n // 2) in-edges (or `hub`) of ONE type, in row n - 3 from 64 rows on: a long tile at the end of the stream
      distinct     min(T, 12) in-edges of distinct types;     dup: the same (source, type) edge stored twice, and one more
      self         two self loops of different types and one more edge (NNConv keeps them)
      from_first / from_last: five in-edges each, all from row 0 / all from row n - 1;   from_halo: four from the halo rows
    Every other row v has (5 v + 3) mod 8 in-edges from random sources (halo rows included), their types running through
    0 .. T - 1 edge after edge: every type is used once there are T such edges or a class row covers it.  T = 0: no edge at all.
    attr: [E, 4] attribute rows, row t of a table of T distinct rows for an edge of type t."""
    gen = torch.Generator().manual_seed(seed)
    n_src = n + halo
    deg = (torch.arange(n) * 5 + 3) % 8
    rows = {}
    if T == 0:
        e0 = torch.zeros(0, dtype=torch.int64)
        return Graph(n, n_src, 0, e0, e0, e0, torch.zeros(n, dtype=torch.int64), {"deg0_last": n - 1}, torch.zeros(0, 4))
    first, end = 0, n
    if n >= 48:
        deg[16:32] = 0
        rows["deg0_tile"] = 16
        first = 32
    if n >= 2:
        deg[n - 1] = 0
        rows["deg0_last"] = n - 1
        end = n - 1
    r = first
    for name, d in _CLASSES:
        if name == "hub":
            d = hub if hub is not None else hub_degree(n)
            if d < 1:
                continue
            if n >= 64:
                rows[name] = n - 3
                deg[n - 3] = d
                continue
        if name == "distinct":
            d = min(T, 12)
        if name == "from_halo" and not halo:
            continue
        if r >= end:
            break
        rows[name] = r
        deg[r] = d
        r += 1
    e = int(deg.sum())
    dst = torch.repeat_interleave(torch.arange(n), deg)
    src = torch.randint(0, n_src, (e,), generator=gen)
    rowptr = torch.cat([torch.zeros(1, dtype=torch.int64), torch.cumsum(deg, 0)])
    filler = torch.ones(e, dtype=torch.bool)
    typ = torch.zeros(e, dtype=torch.int64)
    for name, v in rows.items():
        if name.startswith("deg0"):
            continue
        b, d = int(rowptr[v]), int(deg[v])
        filler[b:b + d] = False
        typ[b:b + d] = torch.arange(d) % T
        if name == "hub":
            typ[b:b + d] = T - 1
        elif name == "dup":
            src[b + 1] = src[b]
            typ[b:b + d] = torch.tensor([0, 0, 1 % T])
        elif name == "self":
            src[b:b + 2] = v
        elif name == "from_first":
            src[b:b + d] = 0
        elif name == "from_last":
            src[b:b + d] = n - 1
        elif name == "from_halo":
            src[b:b + d] = n + torch.arange(d) % halo
    typ[filler] = torch.arange(int(filler.sum())) % T
    table = torch.rand(T, 4, generator=torch.Generator().manual_seed(1000 + T)) + torch.arange(T, dtype=torch.float32).unsqueeze(1)
    return Graph(n, n_src, T, src, dst, typ, deg.clone(), rows, table[typ].contiguous())


def row_class(g, v):
    """the name of row v's class ("" for the other rows)"""
    for name, r in g.rows.items():
        if r == v or (name == "deg0_tile" and r <= v < r + 16):
            return name
    return ""


# ---------------------------------------------------------------------------------------------- operands
Operands = namedtuple("Operands", "h wtab root bias")


def operands(g, c=32, magnitude=1.0, root_scale=0.3, table="rand", seed=1):
    """h [n + halo, c]: a product of two normals (heavy tails) times `magnitude`; wtab [T, c, c] in (0, 1) -- the fp16 forms are
    built for sigmoid outputs -- or every entry exactly 0.0 / exactly 1.0f; root = root_scale * normal; bias at h's magnitude."""
    gen = torch.Generator().manual_seed(seed + 7 * g.n + g.T)
    h = torch.randn(g.n_src, c, generator=gen) * torch.randn(g.n_src, c, generator=gen) * magnitude
    w = torch.rand(g.T, c, c, generator=gen) * (1 - 2.0 ** -10) + 2.0 ** -11
    if table == "zeros":
        w = torch.zeros_like(w)
    elif table == "ones":
        w = torch.ones_like(w)
    else:
        assert table == "rand"
    root = torch.randn(c, c, generator=gen) * root_scale
    bias = torch.randn(c, generator=gen) * magnitude
    return Operands(h, w, root, bias)


# ---------------------------------------------------------------------------------------------- reference and gates
Ref = namedtuple("Ref", "y mag deg a1 b1 c h_max root_max")


def reference(g, op, leaky=False, dtype=torch.float64):
    """The op in `dtype` (fp64: the expectation; fp32: the host test's plain-fp32 implementation), type by type -- index_add_ of
    h[src[e_t]] @ W[t], no [E, c, c] gather --, the mean by max(deg, 1), the root term, the bias, LeakyReLU; with it (always
    fp64) the magnitude sum `mag`, the in-degrees, and the L1 sums A1 [n], B1 [n, c] of the fp16 floors (module docstring)."""
    n, c = g.n, int(op.h.shape[1])
    x, w, root, bias = op.h.to(dtype), op.wtab.to(dtype), op.root.to(dtype), op.bias.to(dtype)
    ax, aw = op.h.double().abs(), op.wtab.double().abs()
    agg = torch.zeros(n, c, dtype=dtype)
    mag = torch.zeros(n, c, dtype=torch.float64)
    b1 = torch.zeros(n, c, dtype=torch.float64)
    order = torch.argsort(g.typ, stable=True)
    counts = torch.bincount(g.typ, minlength=max(g.T, 1)).tolist()
    at = 0
    for t in range(g.T):
        sel = order[at:at + counts[t]]
        at += counts[t]
        if sel.numel() == 0:
            continue
        s, d = g.src[sel], g.dst[sel]
        agg.index_add_(0, d, x[s] @ w[t])
        mag.index_add_(0, d, ax[s] @ aw[t])
        b1.index_add_(0, d, aw[t].sum(0).expand(sel.numel(), c))
    deg = torch.bincount(g.dst, minlength=n)[:n]
    dm = deg.clamp(min=1)
    y = agg / dm.to(dtype).unsqueeze(1) + x[:n] @ root + bias
    if leaky:
        y = orc.leaky_relu(y)
    dm64 = dm.double().unsqueeze(1)
    mag = mag / dm64 + ax[:n] @ op.root.double().abs() + op.bias.double().abs()
    l1 = ax.sum(1)
    a1 = torch.zeros(n, dtype=torch.float64).index_add_(0, g.dst, l1[g.src]) / dm.double() + l1[:n]
    b1 = b1 / dm64 + op.root.double().abs().sum(0)
    return Ref(y, mag, deg, a1, b1, c, float(op.h.abs().max()), float(op.root.abs().max()))


def pow2_scale_for(bound, extra_log2):
    """tgnn_common.h: the power of two s with s * bound * 2^extra_log2 < 2^15, from the bound's fp32 exponent (0, inf, nan -> 1)"""
    e = (int(np.float32(bound).view(np.uint32)) >> 23) & 0xff
    if e in (0, 255):
        return 1.0
    se = min(max(127 + 15 - (e - 126) - extra_log2, 1), 254)
    return 2.0 ** (se - 127)


def nnconv_weight_scale(root_max):
    return pow2_scale_for(max(root_max, 1.0), 0)


def f16_scales(ref, form, degree_bound):
    """(sx, sw) of the module docstring"""
    sw = nnconv_weight_scale(ref.root_max)
    if form == "eg":
        e = (int(np.float32(ref.h_max).view(np.uint32)) >> 23) & 0xff
        return (1.0 if 130 <= e <= 136 else pow2_scale_for(ref.h_max, 5)), sw * 2.0 ** -15
    return pow2_scale_for(ref.h_max, max(int(math.ceil(math.log2(max(degree_bound, 1)))), 0)), sw


def bound(ref, form, degree_bound=None):
    """[n, c] fp64.  degree_bound: what cols_f16 was handed as max_in_degree (default: the graph's largest in-degree)."""
    gamma = (ref.c * (ref.deg.double() + 1) + C0[form]) * U32
    b = gamma.unsqueeze(1) * ref.mag
    if form in ("cols_f16", "eg"):
        sx, sw = f16_scales(ref, form, int(ref.deg.max()) if degree_bound is None else degree_bound)
        b = b + 2.0 ** -25 * (ref.b1 / sx + ref.a1.unsqueeze(1) / sw)
        if form == "eg":
            b = b + 2 * 2.0 ** -25 / (sx * sw)
    return b


def measure(got, ref, form, degree_bound=None):
    """(max-norm relative error, worst error / bound over all elements); NaN where `got` holds one"""
    err = (got.double() - ref.y).abs()
    bnd = bound(ref, form, degree_bound)
    ratio = torch.where((err == 0) & (bnd == 0), torch.zeros_like(err), err / bnd.clamp(min=1e-300))
    return orc.rel_max_err(got, ref.y), float(ratio.max())


def gate_failures(got, ref, form, g=None, degree_bound=None):
    """[] or what failed, as text; written so that a NaN fails.  g: the graph -- the rows over the bound are reported by class."""
    if tuple(got.shape) != tuple(ref.y.shape):
        return ["shape %s, want %s" % (tuple(got.shape), tuple(ref.y.shape))]
    rel, ratio = measure(got, ref, form, degree_bound)
    bad = []
    if not rel < REL_MAX_TOL:
        bad.append("max-norm error %.3e (gate %.0e)" % (rel, REL_MAX_TOL))
    if not ratio <= 1.0:
        err = (got.double() - ref.y).abs()
        over = ~(err <= bound(ref, form, degree_bound))
        rows = torch.nonzero(over.any(1)).squeeze(1).tolist()
        r, c = (int(v) for v in torch.nonzero(over)[0])
        text = "element-wise: %d elements in %d rows over the bound, worst %.3g x; first at row %d column %d: got %.9g want %.9g" % (
            int(over.sum()), len(rows), ratio, r, c, float(got[r, c]), float(ref.y[r, c]))
        if g is not None:
            named = sorted({row_class(g, v) or "other" for v in rows})
            degs = sorted({int(ref.deg[v]) for v in rows})
            text += "; row classes %s; in-degrees %s" % (", ".join(named), degs[:12] + (["..."] if len(degs) > 12 else []))
        bad.append(text)
    return bad


Problem = namedtuple("Problem", "g op ref")


@functools.lru_cache(maxsize=None)
def problem(n, T=OP_TYPES, halo=0, c=32, magnitude=1.0, root_scale=0.3, table="rand", hub=None):
    """One case's graph, operands and fp64 reference WITHOUT LeakyReLU (leaky_ref adds it), computed once per process and shared
    by the tests: treat as read-only."""
    g = graph(n, T, n + T, halo, hub)
    op = operands(g, c, magnitude, root_scale, table)
    return Problem(g, op, reference(g, op))


def leaky_ref(ref):
    return ref._replace(y=orc.leaky_relu(ref.y))


# ---------------------------------------------------------------------------------------------- the edge MLP's table
EW_TYPES = (1, 15, 16, 17, 33, 300)                    # the chunk kernel walks 16 types at a time
EW_FE = (1, 4, 15, 64, 65)                             # 65: beyond the chunk kernel's 64 attribute columns, one block per type
EW_WIDTHS = (32, 64, 8)                                # 8: 64 outputs are no multiple of 256, one block per type


def edge_table_kernel(fe, c):
    return "edge_weight_table_chunks_kernel" if fe <= 64 and (c * c) % 256 == 0 else "edge_weight_table_kernel"


def edge_mlp_problem(T, fe, c, seed=0):
    """Attribute rows [E, fe] with E = 3 T + 2 edges whose representatives are NOT in type order, the edge MLP's weights as a state
    dict (prefix "g.mlp"), the representative edge of every type.  Type 0's attribute row is 400 in every column (type 1's, where
    there is one, -400): layer 1's pre-activations are 400 x N(0, 1), so some of its sigmoids are exactly 0 in fp32 (z < -104:
    below the smallest subnormal) and some exactly 1.0f (z > 17.4) -- edge_mlp_saturation counts them from the fp64 values.  W2 and W3
    are N(0, 1) x 0.5 = 4 / sqrt(64): over 64 inputs in (0, 1) the last pre-activations have a standard deviation of ~2.3, so the
    table spans the sigmoid's unsaturated range, where an error in a hidden layer shows.  Wider weights only saturate the table
    and multiply layer 2's rounding by sum|W3| / 4 (the kernels' sigmoid is the hardware exp2 and reciprocal: 2 u |z| from the
    argument's rounding): at sigma 2 no fp32 evaluation with that sigmoid holds the max-norm gate (measured 2.3e-6 at 17 types)."""
    gen = torch.Generator().manual_seed(seed + 31 * T + 7 * fe + c)
    table = torch.randn(T, fe, generator=gen)
    table[0] = 400.0
    if T > 1:
        table[1] = -400.0
    e = 3 * T + 2
    typ = torch.cat([torch.randperm(T, generator=gen), torch.randint(0, T, (e - T,), generator=gen)])
    rep = torch.stack([torch.nonzero(typ == t)[0, 0] for t in range(T)]).to(torch.int32)
    sd = {"g.mlp.mlp.0.linear.weight": torch.randn(32, fe, generator=gen) * (1.0 / math.sqrt(fe)),
          "g.mlp.mlp.0.linear.bias": torch.randn(32, generator=gen) * 0.3,
          "g.mlp.mlp.1.linear.weight": torch.randn(64, 32, generator=gen) * 0.5,
          "g.mlp.mlp.1.linear.bias": torch.randn(64, generator=gen) * 0.3,
          "g.mlp.mlp.2.linear.weight": torch.randn(c * c, 64, generator=gen) * 0.5,
          "g.mlp.mlp.2.linear.bias": torch.randn(c * c, generator=gen) * 0.3}
    return table, table[typ].contiguous(), rep, sd


def edge_mlp_saturation(table, sd):
    """(layer-1 sigmoids of type 0 that are exactly 0 in fp32, exactly 1.0f) from the fp64 pre-activations"""
    z = table[0].double() @ sd["g.mlp.mlp.0.linear.weight"].double().t() + sd["g.mlp.mlp.0.linear.bias"].double()
    return int((z < -104).sum()), int((z > 17.4).sum())


def edge_mlp_reference(table, sd, c):
    """-> (fp64 table [T, c, c] through oracle.edge_weight_matrices, element-wise bound [T, c, c]).  The bound is dense_oracle's
    sigmoid bound composed over the three layers: a layer's pre-activation carries (K + 8) u (|in| @ |W|^T + |b|) of its own plus
    the previous layer's output error e through |W|; sigmoid's slope falls with |z|, so over [z - e, z + e] it is Lipschitz with
    sigmoid'(max(|z| - e, 0)) <= 1/4 (a saturated unit passes nothing on), and it adds SIGMOID_ULPS ulp of its result, plus 2^-126:
    below fp32's normal range a result may come back as 0 (1 + exp(-z) overflows from z < -88.7; the hardware's exp2 and
    reciprocal flush subnormals)."""
    sd64 = orc.cast_sd(sd, torch.float64)
    with torch.no_grad():
        want = orc.edge_weight_matrices(table.double(), sd64, "g.mlp", c, c)
    x, ex = table.double(), torch.zeros_like(table, dtype=torch.float64)
    for i in range(3):
        w, b = sd64[f"g.mlp.mlp.{i}.linear.weight"], sd64[f"g.mlp.mlp.{i}.linear.bias"]
        z = x @ w.t() + b
        ez = (w.shape[1] + 8) * U32 * (x.abs() @ w.abs().t() + b.abs()) + ex @ w.abs().t()
        x = orc.sigmoid(z)
        near = orc.sigmoid(-(z.abs() - ez).clamp(min=0))          # (the small one of sigmoid(+-t): 1 - it does not cancel)
        ex = ez * near * (1 - near) + do.SIGMOID_ULPS * do.ulp32(x) + 2.0 ** -126
    return want, ex.view(-1, c, c)
