"""Cases of the eval-mode forward (TilinGNN.eval(): BatchNorm on the running buffers, tgnn_forward with use_running_stats) and the
gate that holds it against the fp64 oracle through the whole depth.  Importable without a GPU: everything here is CPU torch.

Why eval mode can be gated 20 layers deep when train mode cannot: batch statistics of near-constant columns amplify the last
bit (tests/test_small_layout.py: 4x per layer), running statistics with a floor under every variance do not.  The running buffers
of a freshly made state dict (mean 0, var 1) would not tell one BatchNorm's buffers from another's, so the cases carry
statistics worth reading:

* `conditioned_state_dict`: the batch statistics of ONE train-mode fp64 oracle pass (momentum 1) over a fixed 1 000-node source
  layout, `ridge` added to every running_var, rounded to fp32 (the network holds fp32; the fp64 oracle reads the rounded values);
* `jittered_state_dict`: the same from another source layout, every entry then moved by a seeded draw of its own (mean by
  0.3 standard deviations, var by a factor in [0.5, 1.5]): buffers that are no layout's statistics.  (Draws unrelated to the
  activations -- `independent_state_dict` -- leave the network unscaled and every probability saturated: measured there.)

The gate of a case's tap is taken from the oracle alone (`gate`): 8 x the distance of the oracle's own fp32 run from its fp64 run,
floored at 2e-6 (max-normalised, orc.rel_max_err); probabilities: 8 x the same distance, absolute, floored at 5e-7.  Why 8: the
matrix-core kernels carry three roundings per product (bf16 x 3 split) where torch's fp32 carries one, and 20 layers compound.
tests/test_eval_cases_host.py holds what makes these gates meaningful (the oracle's pins, conditioning, observability,
sensitivity to the mistakes restated in `MISTAKES`); tests/test_eval_forward.py holds the HIP forward to them."""
import contextlib
import functools
from dataclasses import dataclass
from typing import Dict, Optional, Tuple

import numpy as np
import torch

from oracle import tilingnn_oracle as orc
from tests.golden_util import graph_tensors, load_labyrinth_graph
from tilingnn_amd.synth import make_super_graph
from tilingnn_amd.weights import make_state_dict

RIDGE = 0.01                                   # added to every running_var (the labyrinth case: 0.02, see LAYOUT_CASES)
SOURCE_LAYOUT = (1000, 8000, 10000, 3)         # make_super_graph(n, ea, ec, seed=...) behind the conditioned statistics
GATE_FACTOR, GATE_FLOOR, PROBS_FLOOR = 8.0, 2e-6, 5e-7
CONDITIONING = 2e-5                            # the oracle's fp32 run within this of its fp64 run, every gated tap of every case


# ------------------------------------------------------------------------------------------------------------------ statistics
def _rounded_to_fp32(sd):
    return {k: (v.float() if v.is_floating_point() else v.clone()) for k, v in sd.items()}


@functools.lru_cache(maxsize=None)
def _conditioned(fe, depth, width, out_dim, fx, seed, ridge, source=SOURCE_LAYOUT):
    sd64 = orc.cast_sd(make_state_dict(fe, depth, width, out_dim, fx, seed=seed), torch.float64)
    n, ea, ec, src_seed = source
    sg = make_super_graph(n, ea, ec, tile_count=fx - 1, n_edge_types=fe - 2, seed=src_seed)
    src = _fp32_values(sg.node_feature, sg.align_edge_index, sg.align_edge_features, sg.collide_edge_index)
    saved = orc.BN_MOMENTUM
    orc.BN_MOMENTUM = 1.0                      # running buffers := this pass's batch mean / unbiased variance
    try:
        with torch.no_grad():
            orc.tilingnn_forward(sd64, *src, update_running=True)
    finally:
        orc.BN_MOMENTUM = saved
    for k in sd64:
        if k.endswith("running_var"):
            sd64[k] = sd64[k] + ridge
        elif k.endswith("num_batches_tracked"):
            sd64[k] = torch.ones((), dtype=torch.int64)
    return _rounded_to_fp32(sd64)


def conditioned_state_dict(fe, depth, width, out_dim, fx, seed, ridge=RIDGE) -> Dict[str, torch.Tensor]:
    """fp32 state dict (a fresh copy) whose running buffers are the source layout's batch statistics + `ridge` on the variances."""
    return {k: v.clone() for k, v in _conditioned(fe, depth, width, out_dim, fx, seed, ridge).items()}


def independent_state_dict(fe, depth, width, out_dim, fx, seed) -> Dict[str, torch.Tensor]:
    """fp32 state dict whose running buffers are seeded draws: mean ~ 0.3 N(0, 1), var ~ U[0.05, 1.5], num_batches_tracked 1.
    NOT a recipe of any gated case: buffers unrelated to the activations leave no BatchNorm a normaliser.  Measured with the
    fp64 oracle: max |middle| 6e3 at depth 3, 5e5 at depth 5 and 7e23 at depth 20 (the adjacency branch is linear in its input
    and the residual adds), the collision columns vary by 0.02 ... 0.3 % of their magnitude over the rows (observability asks for
    1 %) and every probability saturates (spread 0 on the labyrinth graph): a test on it would gate nothing.  Kept for
    tests/test_eval_cases_host.py, which holds those figures; `jittered_state_dict` is the second recipe of the cases."""
    sd = {k: v.clone() for k, v in make_state_dict(fe, depth, width, out_dim, fx, seed=seed).items()}
    g = torch.Generator().manual_seed(1000 + seed)
    for k in sd:                               # (insertion order of the state dict: the draw sequence is part of the recipe)
        if k.endswith("running_mean"):
            sd[k] = (0.3 * torch.randn(sd[k].shape, generator=g, dtype=torch.float64)).float()
        elif k.endswith("running_var"):
            sd[k] = (0.05 + 1.45 * torch.rand(sd[k].shape, generator=g, dtype=torch.float64)).float()
        elif k.endswith("num_batches_tracked"):
            sd[k] = torch.ones((), dtype=torch.int64)
    return sd


JITTER_SOURCE = (300, 1500, 1800, 11)          # another source layout than SOURCE_LAYOUT: smaller, sparser


def jittered_state_dict(fe, depth, width, out_dim, fx, seed, ridge=RIDGE) -> Dict[str, torch.Tensor]:
    """The second recipe: no buffer is any layout's statistic.  The conditioned buffers of ANOTHER source layout (JITTER_SOURCE),
    every entry then moved by a seeded draw of its own, relative to the entry's scale so that the BatchNorms still normalise:
    mean += 0.3 sqrt(var) N(0, 1), var *= U[0.5, 1.5] (var with the ridge in it).  A kernel that reads the right buffer at the
    right place is as close to the oracle as on the first recipe; nothing else of the first recipe is shared."""
    sd = {k: v.double() if v.is_floating_point() else v.clone()
          for k, v in _conditioned(fe, depth, width, out_dim, fx, seed, ridge, JITTER_SOURCE).items()}
    g = torch.Generator().manual_seed(1000 + seed)
    for k in list(sd):                         # (insertion order of the state dict: the draw sequence is part of the recipe)
        if k.endswith("running_mean"):
            var = sd[k[:-len("running_mean")] + "running_var"]
            sd[k] = sd[k] + 0.3 * var.sqrt() * torch.randn(sd[k].shape, generator=g, dtype=torch.float64)
    for k in list(sd):
        if k.endswith("running_var"):
            sd[k] = sd[k] * (0.5 + torch.rand(sd[k].shape, generator=g, dtype=torch.float64))
    return _rounded_to_fp32(sd)


# --------------------------------------------------------------------------------------------------------------------- layouts
def _fp32_values(x, adj, attr, col):
    """(x, adj, attr, col) as fp64 / int64 CPU tensors holding fp32-representable values: what the network is fed, .float(), is
    then exactly what the fp64 oracle reads."""
    f = lambda a: torch.from_numpy(np.ascontiguousarray(a)).float().double()
    i = lambda a: torch.from_numpy(np.ascontiguousarray(a)).long().reshape(2, -1)
    return f(x), i(adj), f(attr), i(col)


def _one_hot_attr(types, n_types):
    attr = np.zeros((len(types), 2 + n_types))
    attr[:, 1] = np.where(np.asarray(types) % 2 == 0, 0.57735, 1.0)
    attr[np.arange(len(types)), 2 + np.asarray(types)] = 1.0
    return attr


def _node_rows(n, tile_count):
    x = np.zeros((n, tile_count + 1))
    t = np.arange(n) % tile_count
    x[np.arange(n), t] = 1.0
    x[:, -1] = np.linspace(1.0, 0.5, tile_count)[t] if tile_count > 1 else 1.0
    return x


@functools.lru_cache(maxsize=None)
def layout(kind: str, n: int, n_types: int = 13, tile_count: int = 2):
    """(x, adj_e_index, adj_e_features, col_e_idx) of a named layout, CPU, fp64 / int64, fp32-representable values.
    one: one row, no edge.  two: two rows, one adjacency pair and one collision pair.  syn: make_super_graph with 8 n / 10 n
    edges (4 n / 3 n below 100 rows; 4 n / 5 n from 1 000 and 2 n / 3 n from 2 000 rows on: the oracle materialises [Ea, C, C] per
    layer, and every case costs its test two oracle runs).  sparse: 4 n / 2 n edges, and the last five rows cut out of both sets (rows without an
    in-edge in either).  no_adj / no_col: `syn` with that set empty.  hub: 400 rows, row 5 with exactly 300 adjacency in-edges.
    labyrinth: the committed real graph."""
    if kind == "labyrinth":
        return _fp32_values(*[t.numpy() for t in graph_tensors(load_labyrinth_graph(), torch.float64)[:4]])
    empty = np.zeros((2, 0), dtype=np.int64)
    if kind == "one":
        return _fp32_values(_node_rows(1, tile_count), empty, np.zeros((0, 2 + n_types)), empty)
    if kind == "two":
        pair = np.array([[0, 1], [1, 0]])
        return _fp32_values(_node_rows(2, tile_count), pair, _one_hot_attr([0, 0], n_types), pair)
    ea, ec = (4 * n, 2 * n) if kind == "sparse" else (2 * n, 3 * n) if n >= 2000 else (4 * n, 5 * n) if n >= 1000 else \
        (8 * n, 10 * n) if n >= 100 else (4 * n, 3 * n)
    sg = make_super_graph(n, ea, ec, tile_count=tile_count, n_edge_types=n_types, seed=n % 97 + 1)
    x, adj, attr, col = sg.node_feature, sg.align_edge_index, sg.align_edge_features, sg.collide_edge_index
    if kind == "sparse":
        keep = (adj < n - 5).all(axis=0)
        adj, attr = adj[:, keep], attr[keep]
        col = col[:, (col < n - 5).all(axis=0)]
    elif kind == "no_adj":
        adj, attr = empty, attr[:0]
    elif kind == "no_col":
        col = empty
    elif kind == "hub":
        keep = adj[1] != 5
        src = np.arange(50, 350)
        adj = np.concatenate([adj[:, keep], np.stack([src, np.full(300, 5)])], axis=1)
        attr = np.concatenate([attr[keep], _one_hot_attr(src % n_types, n_types)], axis=0)
    elif kind != "syn":
        raise ValueError(kind)
    return _fp32_values(x, adj, attr, col)


# ----------------------------------------------------------------------------------------------------------------------- cases
@dataclass(frozen=True)
class Case:
    name: str
    kind: str
    n: int
    depth: int = 20
    width: int = 32
    out_dim: int = 1
    tile_count: int = 2
    n_types: int = 13
    stats: str = "conditioned"             # or "jittered"
    seed: int = 0
    ridge: float = RIDGE

    @property
    def fe(self):
        return 2 + self.n_types

    @property
    def fx(self):
        return self.tile_count + 1

    def inputs(self):
        return layout(self.kind, self.n, self.n_types, self.tile_count)

    def state_dict(self):
        a = (self.fe, self.depth, self.width, self.out_dim, self.fx, self.seed, self.ridge)
        return conditioned_state_dict(*a) if self.stats == "conditioned" else jittered_state_dict(*a)

    def taps(self):
        return ["mid.%d" % k for k in range(self.depth + 1)] + ["f1", "f2", "f3", "probs"]


# ridge: 0.01 wherever it conditions the case (at 0.02 `no-eps` moves the one- and two-row layouts by less than their gates).  The
# labyrinth graph's activations are 3 x the source layout's (max |middle| 4.95 against 1.5): at 0.01 the oracle's fp32 run is
# 2.5e-5 off its fp64 run in middle[2], above CONDITIONING; at 0.02 7.5e-6, and `no-eps` still moves every tap by 8.8 gates.
LABYRINTH = Case("labyrinth", "labyrinth", 1254, ridge=0.02)
LAYOUT_CASES = (
    Case("one-row", "one", 1),
    Case("two-rows", "two", 2),
    Case("16-rows", "syn", 16),
    Case("17-rows", "syn", 17),
    Case("300-sparse", "sparse", 300),
    Case("300-no-adjacency", "no_adj", 300),
    Case("300-no-collision", "no_col", 300),
    LABYRINTH,
    # (seed 1: every skip slot varies by >= 3.5 % of its magnitude over the rows; the jitter of seed 2 leaves one at 0.9 %)
    Case("labyrinth-jittered", "labyrinth", 1254, stats="jittered", seed=1),
    Case("4097-rows", "syn", 4097),
    Case("1000-one-type", "syn", 1000, n_types=1),
    Case("1000-fifty-types", "syn", 1000, n_types=50),
    Case("hub-300", "hub", 400),
)
MODEL_CASES = (
    Case("depth-1", "syn", 300, depth=1),
    Case("depth-2", "syn", 300, depth=2),
    Case("depth-3", "syn", 300, depth=3),
    Case("depth-23", "syn", 300, depth=23),
    Case("three-maps", "syn", 300, out_dim=3, stats="jittered", seed=4),
    Case("four-tiles", "syn", 300, tile_count=4),
    Case("width-64", "syn", 300, width=64, stats="jittered", seed=6),
    Case("width-96", "sparse", 300, width=96, stats="jittered", seed=5),
)
# the general schedule at 3 000 rows on a graph prepared with edge groups only; five layouts side by side (forward_many)
ROUTING_CASES = (Case("3000-rows", "syn", 3000),)
# held on the CPU only (the reference's own width-64 run on the real graph pins the oracle; its two oracle runs take ~8 s)
HOST_CASES = (Case("width-64-labyrinth", "labyrinth", 1254, width=64),)
MANY_CASES = (Case("one-row", "one", 1), Case("many-640", "syn", 640), LABYRINTH,
              Case("many-900", "syn", 900), Case("17-rows", "syn", 17))
CASES = {c.name: c for c in LAYOUT_CASES + MODEL_CASES + ROUTING_CASES + MANY_CASES + HOST_CASES}
# the cases the committed outputs of the reference's own modules in .eval() cover (tests/golden/generate_eval_golden.py)
GOLDEN_CASES = ("labyrinth", "width-64-labyrinth", "17-rows", "one-row")


# ---------------------------------------------------------------------------------------------------------------- oracle runs
@contextlib.contextmanager
def _batch_norm_as(fn):
    saved = orc.batch_norm_train
    orc.batch_norm_train = fn
    try:
        yield
    finally:
        orc.batch_norm_train = saved


def _finish(sd, cap, depth):
    """The taps of one captured forward: middle[k], the final MLP's three hidden activations BEFORE their BatchNorm (the
    workspace's F1 F2 F3), the probabilities.  Runs inside the caller's BatchNorm context."""
    out = {"mid.0": cap["init"], "probs": cap["probs"]}
    for k in range(1, depth + 1):
        out["mid.%d" % k] = cap["mid.%d" % k]
    v = cap["cat"]
    for l in range(3):
        p = "final_mlp.0.mlp.%d" % l
        out["f%d" % (l + 1)] = orc.leaky_relu(orc.linear(v, sd, p + ".linear"))
        v = orc.batch_norm_train(out["f%d" % (l + 1)], sd, p + ".batch_norm")
    return out


def oracle_taps(sd, inputs, dtype, batch_norm=None) -> Dict[str, torch.Tensor]:
    """Every tap of the eval-mode oracle forward in `dtype`.  batch_norm: another BatchNorm in place of orc.batch_norm_eval (the
    restated mistakes)."""
    sdd = orc.cast_sd(sd, dtype)
    ins = tuple(t.to(dtype) if t.is_floating_point() else t for t in inputs)
    cap = {}
    with torch.no_grad(), _batch_norm_as(batch_norm or orc.batch_norm_eval):
        orc.tilingnn_forward(sdd, *ins, capture=cap)
        return _finish(sdd, cap, orc.network_depth_of(sdd))


@functools.lru_cache(maxsize=None)
def reference(case: Case) -> Tuple[Dict[str, torch.Tensor], Dict[str, torch.Tensor]]:
    """(fp64 taps, fp32 taps) of the oracle on the case; computed once, shared, never written to."""
    sd, inputs = case.state_dict(), case.inputs()
    return oracle_taps(sd, inputs, torch.float64), oracle_taps(sd, inputs, torch.float32)


def tap_error(tap: str, got: torch.Tensor, want: torch.Tensor) -> float:
    """The measure the gate is stated in: max-normalised for activations, absolute for probabilities."""
    if tap == "probs":
        return float((got.double() - want.double()).abs().max())
    return orc.rel_max_err(got, want)


def oracle_floor(case: Case, tap: str) -> float:
    t64, t32 = reference(case)
    return tap_error(tap, t32[tap], t64[tap])


def gate(case: Case, tap: str) -> float:
    return max(GATE_FACTOR * oracle_floor(case, tap), PROBS_FLOOR if tap == "probs" else GATE_FLOOR)


def probs_gate(sd, inputs) -> Tuple[torch.Tensor, float]:
    """(fp64 probabilities, their gate) of the eval-mode forward of ANY state dict on a layout: tests of other files that run one
    eval forward hold it to the oracle with this instead of asking for finite numbers."""
    inputs = tuple(t.detach().cpu().double() if t.is_floating_point() else t.detach().cpu() for t in inputs)
    sd = {k: v.detach().cpu() for k, v in sd.items()}
    p64, p32 = oracle_taps(sd, inputs, torch.float64)["probs"], oracle_taps(sd, inputs, torch.float32)["probs"]
    return p64, max(GATE_FACTOR * tap_error("probs", p32, p64), PROBS_FLOOR)


# -------------------------------------------------------------------------------------------------------------------- mistakes
def _residual_from(sd, inputs, skip):
    """tilingnn_forward's layer loop with the residual taken from middle[i - skip] (the network: skip = 2; pinned equal to
    orc.tilingnn_forward at skip = 2 by tests/test_eval_cases_host.py).  Runs inside the caller's BatchNorm context."""
    x, adj, attr, col = inputs
    depth = orc.network_depth_of(sd)
    h1 = orc.init_node_feature_trans(x, sd)
    h2 = h1
    middle = [h1]
    for i in range(depth):
        g1 = orc.graph_conv(h1, adj, attr, sd, "brch_1_graph_conv_layers.%d" % i)
        h2 = orc.coll_conv(h2, col, sd, "brch_2_coll_conv_layers.%d" % i)
        h1 = g1 * h2
        if i - skip >= 0:
            h1 = h1 + middle[i - skip]
        middle.append(h1)
    cap = {"init": middle[0], "cat": torch.cat(middle, dim=1)}
    cap.update({"mid.%d" % k: middle[k] for k in range(1, depth + 1)})
    cap["probs"] = orc.final_mlp(cap["cat"], sd)
    return _finish(sd, cap, depth)


def residual_taps(sd, inputs, skip) -> Dict[str, torch.Tensor]:
    sdd = orc.cast_sd(sd, torch.float64)
    with torch.no_grad(), _batch_norm_as(orc.batch_norm_eval):
        return _residual_from(sdd, inputs, skip)


def _bn_no_eps(v, sd, prefix, update_running=False):
    return (v - sd[prefix + ".running_mean"]) / torch.sqrt(sd[prefix + ".running_var"]) * sd[prefix + ".weight"] + sd[prefix + ".bias"]


def _bn_unbiased(v, sd, prefix, update_running=False):
    n = v.shape[0]
    var = sd[prefix + ".running_var"] * (n / (n - 1))
    return (v - sd[prefix + ".running_mean"]) / torch.sqrt(var + orc.BN_EPS) * sd[prefix + ".weight"] + sd[prefix + ".bias"]


_BN_TRAIN = orc.batch_norm_train


def _bn_last_final_train(v, sd, prefix, update_running=False):
    return (_BN_TRAIN if prefix == "final_mlp.0.mlp.3.batch_norm" else orc.batch_norm_eval)(v, sd, prefix)


# name -> (first tap behind the point of action, smallest depth, smallest row count at which the mistake is one)
MISTAKES = {
    "no-eps": ("mid.0", 1, 1),
    "collision-bn-7-8-swapped": ("mid.8", 9, 1),
    "residual-from-i-1": ("mid.2", 2, 1),
    "last-final-bn-on-batch-statistics": ("probs", 1, 2),
    "unbiased-running-var": ("mid.0", 1, 2),
}


def mistake_applies(case: Case, name: str) -> bool:
    _, depth, rows = MISTAKES[name]
    return case.depth >= depth and case.n >= rows


def taps_behind(case: Case, name: str):
    taps = case.taps()
    return taps[taps.index(MISTAKES[name][0]):]


def mistaken_taps(case: Case, name: str) -> Optional[Dict[str, torch.Tensor]]:
    """The fp64 taps of the oracle with the named mistake restated in it; None where the mistake does not apply to the case."""
    if not mistake_applies(case, name):
        return None
    sd, inputs = case.state_dict(), case.inputs()
    if name == "no-eps":
        return oracle_taps(sd, inputs, torch.float64, _bn_no_eps)
    if name == "unbiased-running-var":
        return oracle_taps(sd, inputs, torch.float64, _bn_unbiased)
    if name == "last-final-bn-on-batch-statistics":
        return oracle_taps(sd, inputs, torch.float64, _bn_last_final_train)
    if name == "residual-from-i-1":
        return residual_taps(sd, inputs, 1)
    a, b = "brch_2_coll_conv_layers.7.batch_norm", "brch_2_coll_conv_layers.8.batch_norm"
    for s in (".running_mean", ".running_var"):
        sd[a + s], sd[b + s] = sd[b + s], sd[a + s]
    return oracle_taps(sd, inputs, torch.float64)
