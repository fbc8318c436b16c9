"""What makes the gates of tests/test_eval_forward.py meaningful, on the CPU (no GPU, no HIP code):

* the eval-mode oracle (oracle/tilingnn_oracle.py: running_statistics) is torch's eval-mode BatchNorm, on one Linear_trans and
  through the whole forward, and equals the REFERENCE's own modules in .eval() (tests/golden/ref_forward_eval.npz);
* every case of tests/eval_cases.py is conditioned (the oracle's fp32 run within 2e-5 of its fp64 run at every gated tap),
  observable (the taps vary over the rows, the probabilities spread) and sensitive: each mistake of eval_cases.MISTAKES, restated
  inside the fp64 oracle, moves every gated tap behind its point of action by at least two gates."""
import numpy as np
import pytest
import torch
import torch.nn.functional as F

from oracle import tilingnn_oracle as orc
from tests import eval_cases as ec
from tests.golden_util import load_npz

ALL = sorted(ec.CASES)


def _torch_bn_module(v, sd, prefix, update_running=False):
    bn = torch.nn.BatchNorm1d(v.shape[1]).to(v.dtype)
    bn.load_state_dict({k: sd[f"{prefix}.{k}"] for k in ("weight", "bias", "running_mean", "running_var", "num_batches_tracked")})
    return bn.eval()(v)


def _torch_bn_functional(v, sd, prefix, update_running=False):
    return F.batch_norm(v, sd[prefix + ".running_mean"], sd[prefix + ".running_var"], sd[prefix + ".weight"], sd[prefix + ".bias"],
                        False, orc.BN_MOMENTUM, orc.BN_EPS)


# ------------------------------------------------------------------------------------------------------------ the oracle's pins
@pytest.mark.parametrize("torch_bn", [_torch_bn_module, _torch_bn_functional])
def test_eval_oracle_is_torch_on_one_linear_trans(torch_bn):
    case = ec.CASES["17-rows"]
    sd = orc.cast_sd(case.state_dict(), torch.float64)
    x = case.inputs()[0]
    p = "init_node_feature_trans.mlp.0"
    with orc.running_statistics():
        got = orc.linear_trans(x, sd, p, orc.leaky_relu, bn=True)
    lin = torch.nn.Linear(case.fx, case.width).double()
    lin.load_state_dict({"weight": sd[p + ".linear.weight"], "bias": sd[p + ".linear.bias"]})
    with torch.no_grad():
        want = torch_bn(F.leaky_relu(lin(x), orc.LEAKY_SLOPE), sd, p + ".batch_norm")
    assert orc.rel_max_err(got, want) <= 1e-14
    assert not torch.equal(got, orc.linear_trans(x, sd, p, orc.leaky_relu, bn=True))      # (outside the context: train mode again)


@pytest.mark.parametrize("name", ["one-row", "two-rows", "17-rows", "300-sparse", "depth-3", "labyrinth"])
@pytest.mark.parametrize("torch_bn", [_torch_bn_module, _torch_bn_functional])
def test_eval_oracle_is_torch_through_the_whole_forward(name, torch_bn):
    """The whole forward built from torch.nn.BatchNorm1d(...).double().eval() / F.batch_norm(training=False) fed the same buffers.

    1e-14 in units of what torch's BatchNorm itself rounds: ATen evaluates eval mode as x w + b with w = gamma / sqrt(var + eps),
    b = beta - mean w (batch_norm_cpu_transform_input), so its own rounding error is 2^-53 (|x w| + |b|) -- on the collision
    branch (sigmoid columns near 0.5 over a standard deviation of 0.1) ten times the result.  Held at every one of the 2 D + 6
    BatchNorm calls of the free-running forward in that unit, and on the final MLP's hidden activations and the probabilities
    free running in the taps' own unit.  The skip slots free running sit at 1.2e-14 ... 2.2e-14 of their max-norm on these cases
    (measured; the same at depth 3 and 20: one collision BatchNorm's cancellation inside torch, not a drift) and are
    not asserted in that unit."""
    case = ec.CASES[name]
    calls = []

    def both(v, sd, prefix, update_running=False):
        got, want = orc.batch_norm_eval(v, sd, prefix), torch_bn(v, sd, prefix)
        w = sd[prefix + ".weight"] / torch.sqrt(sd[prefix + ".running_var"] + orc.BN_EPS)
        unit = float(((v * w).abs() + (sd[prefix + ".bias"] - sd[prefix + ".running_mean"] * w).abs()).max())
        calls.append(prefix)
        assert float((got - want).abs().max()) <= 1e-14 * unit, (prefix, float((got - want).abs().max()), unit)
        return want                                               # (the forward goes on with torch's values)
    want = ec.oracle_taps(case.state_dict(), case.inputs(), torch.float64, both)
    assert len(set(calls)) == 2 * case.depth + 6
    got = ec.reference(case)[0]
    for tap in ("f1", "f2", "f3", "probs"):
        assert ec.tap_error(tap, got[tap], want[tap]) <= 1e-14, tap
    print(name, "skip slots free running:", max(ec.tap_error(t, got[t], want[t]) for t in case.taps() if t.startswith("mid")))


def test_eval_oracle_writes_no_buffer_and_takes_one_row():
    case = ec.CASES["one-row"]
    sd = orc.cast_sd(case.state_dict(), torch.float64)
    before = {k: v.clone() for k, v in sd.items()}
    with orc.running_statistics(), torch.no_grad():
        probs, _ = orc.tilingnn_forward(sd, *case.inputs(), update_running=True)
    assert probs.shape == (1, 1) and bool(torch.isfinite(probs).all())
    assert all(torch.equal(before[k], sd[k]) for k in before)
    assert orc.batch_norm_train is not orc.batch_norm_eval                                 # (the context has left)


@pytest.mark.parametrize("name", ec.GOLDEN_CASES)
def test_eval_oracle_is_the_reference_in_eval(name):
    """The reference's own network modules after .eval(), float64 (tests/golden/generate_eval_golden.py): 1e-9."""
    z = load_npz("ref_forward_eval.npz")
    case = ec.CASES[name]
    sd = case.state_dict()
    for leaf in ("mean", "var"):                                  # the recipe reproduces the generator's buffers bit for bit
        mine = np.concatenate([v.numpy().ravel() for k, v in sd.items() if k.endswith("running_" + leaf)])
        assert mine.dtype == np.float32 and np.array_equal(mine, z[f"{name}/bn_{leaf}"]), leaf
    t64 = ec.reference(case)[0]
    assert float(np.abs(t64["probs"].numpy() - z[f"{name}/probs"]).max()) <= 1e-9
    rows, cols = z[f"{name}/rows"], z[f"{name}/cols"]
    assert len(rows) == min(case.n, 64) and z[f"{name}/middle"].shape == (case.depth + 1, len(rows), len(cols))
    for k in range(case.depth + 1):
        mid = t64["mid.%d" % k].numpy()
        assert np.abs(mid[rows][:, cols] - z[f"{name}/middle"][k]).max() <= 1e-9 * np.abs(mid).max(), k
        want_sum = z[f"{name}/middle_colsum"][k]
        assert np.abs(mid.sum(axis=0) - want_sum).max() <= 1e-9 * max(np.abs(want_sum).max(), np.abs(mid).max()), k


def test_residual_restatement_is_the_oracle_at_skip_two():
    case = ec.CASES["17-rows"]
    mine, want = ec.residual_taps(case.state_dict(), case.inputs(), 2), ec.reference(case)[0]
    for tap in case.taps():
        assert torch.equal(mine[tap], want[tap]), tap


# ------------------------------------------------------------------------------------------------------------------- the cases
def test_the_layouts_are_what_their_names_say():
    _, adj, attr, col = ec.layout("sparse", 300)
    touched = set(adj[1].tolist()) | set(col[1].tolist())
    assert 0 < len(set(range(300)) - touched) and all(r not in touched for r in range(295, 300))
    assert ec.layout("no_adj", 300)[1].shape == (2, 0) and ec.layout("no_adj", 300)[2].shape == (0, 15)
    assert ec.layout("no_col", 300)[3].shape == (2, 0) and ec.layout("no_col", 300)[1].shape[1] > 0
    hub = ec.layout("hub", 400)
    assert int((hub[1][1] == 5).sum()) == 300 and hub[2].shape[0] == hub[1].shape[1]
    assert int(torch.unique(ec.layout("syn", 1000, 50)[2], dim=0).shape[0]) == 50
    assert int(torch.unique(ec.layout("syn", 1000, 1)[2], dim=0).shape[0]) == 1
    x, adj, attr, col = ec.layout("one", 1)
    assert x.shape == (1, 3) and adj.shape == col.shape == (2, 0) and attr.shape == (0, 15)
    for case in ec.CASES.values():
        x, adj, attr, col = case.inputs()
        assert x.shape == (case.n, case.fx) and attr.shape == (adj.shape[1], case.fe) and case.n <= 5000
        assert torch.equal(x, x.float().double()) and torch.equal(attr, attr.float().double())
        assert adj.numel() == 0 or (0 <= int(adj.min()) and int(adj.max()) < case.n)
        assert col.numel() == 0 or (0 <= int(col.min()) and int(col.max()) < case.n)


def test_both_recipes_give_fp32_buffers_above_the_ridge():
    for case in (ec.CASES["17-rows"], ec.CASES["labyrinth"], ec.CASES["labyrinth-jittered"]):
        sd, plain = case.state_dict(), ec.make_state_dict(case.fe, case.depth, case.width, case.out_dim, case.fx, seed=case.seed)
        floor = case.ridge * (0.5 if case.stats == "jittered" else 1.0)
        for k, v in sd.items():
            if k.endswith("running_var"):
                assert v.dtype == torch.float32 and float(v.min()) >= floor * (1 - 1e-6), k
            elif k.endswith("running_mean"):
                assert v.dtype == torch.float32 and float(v.abs().max()) > 0, k
            elif k.endswith("num_batches_tracked"):
                assert int(v) == 1
            else:
                assert torch.equal(v, plain[k]), k               # (the parameters are make_state_dict's)
    a, b = ec.CASES["labyrinth-jittered"].state_dict(), ec.CASES["labyrinth-jittered"].state_dict()
    assert all(torch.equal(a[k], b[k]) for k in a)               # seeded
    k = "brch_2_coll_conv_layers.7.batch_norm.running_var"
    assert not torch.equal(a[k], a[k.replace(".7.", ".8.")])


def test_statistics_unrelated_to_the_activations_gate_nothing():
    """Why the second recipe jitters a layout's statistics instead of drawing them outright (mean ~ 0.3 N(0, 1), var ~
    U[0.05, 1.5]): with such buffers the activations grow layer by layer, the skip slots stop varying over the rows and the
    probabilities saturate."""
    inputs = ec.layout("syn", 300)
    sd = ec.independent_state_dict(15, 5, 32, 1, 3, seed=4)
    t = ec.oracle_taps(sd, inputs, torch.float64)
    assert float(t["mid.5"].abs().max()) > 1e4
    assert all(float(p) in (0.0, 1.0) or min(float(p), 1 - float(p)) < 1e-6 for p in t["probs"].flatten())


@pytest.mark.parametrize("name", ALL)
def test_case_is_conditioned_and_observable(name):
    case = ec.CASES[name]
    t64, _ = ec.reference(case)
    for tap in case.taps():
        floor = ec.oracle_floor(case, tap)
        assert floor <= ec.CONDITIONING, (tap, floor)
        assert ec.gate(case, tap) >= (ec.PROBS_FLOOR if tap == "probs" else ec.GATE_FLOOR)
        assert ec.gate(case, tap) <= ec.GATE_FACTOR * ec.CONDITIONING
    assert bool(((t64["probs"] > 0) & (t64["probs"] < 1)).all())
    if case.n >= 17:
        for k in range(case.depth + 1):
            w = t64["mid.%d" % k]
            rms = float((w - w.mean(dim=0, keepdim=True)).pow(2).mean().sqrt())
            assert rms >= 0.01 * float(w.abs().max()), (k, rms)
        assert float(t64["probs"].max() - t64["probs"].min()) >= 1e-3


@pytest.mark.parametrize("mistake", sorted(ec.MISTAKES))
@pytest.mark.parametrize("name", ALL)
def test_case_is_sensitive_to(name, mistake):
    case = ec.CASES[name]
    wrong = ec.mistaken_taps(case, mistake)
    if wrong is None:                                             # (the mistake is none on this case: see eval_cases.MISTAKES)
        assert not ec.mistake_applies(case, mistake)
        return
    t64, _ = ec.reference(case)
    for tap in ec.taps_behind(case, mistake):
        moved = ec.tap_error(tap, wrong[tap], t64[tap])
        assert moved >= 2 * ec.gate(case, tap), (tap, moved, ec.gate(case, tap))


def test_every_mistake_applies_somewhere_and_most_everywhere():
    for mistake in ec.MISTAKES:
        hit = [n for n in ALL if ec.mistake_applies(ec.CASES[n], mistake)]
        assert len(hit) >= len(ALL) - 4, (mistake, hit)           # (depth 1 ... 3 have no layers 7 / 8; one row has no batch statistics)
