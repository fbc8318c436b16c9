"""tilingnn_amd.optim.Adam on the GPU (csrc/adam.hip: tgnn_adam_step): every step teacher forced against the fp64
evaluation of torch's Adam formulas on the same fp32 inputs, under the gates of tests/adam_cases.py (which
tests/test_adam_plan_host.py first points at torch's own CPU Adam); the two ways the gradients are addressed, bit for bit; the
interchange of checkpoints with torch.optim.Adam; the whole depth-20 network behind one real backward; the refusals."""
import functools
import io
import types

import numpy as np
import pytest
import torch

from tests import adam_cases as ac
from tests.golden_util import graph_tensors, load_npz

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
SENTINEL = 12345.678
NO_GRAD = (5, 9)                       # parameters (63 and CHUNK elements) that get no gradient in the single-step runs


def _adam(*a, **k):
    from tilingnn_amd.optim import Adam
    return Adam(*a, **k)


def _bits(t):
    return t.detach().contiguous().view(torch.int32).cpu().numpy().copy()


def _arena(ps):
    """The parameters as views of ONE buffer, a guard band of sentinels around each; every parameter starts on a 256-byte boundary
    but the one at OFFSET_ONE, which starts one float behind one.  -> (buffer, parameters, [(start, numel)])"""
    spans, off = [], ac.GUARD
    for k, p in enumerate(ps):
        start = off + (1 if k == ac.OFFSET_ONE else 0)
        spans.append((start, p.size))
        off = (start + p.size + ac.GUARD + 63) // 64 * 64
    host = np.full(off, SENTINEL, dtype=np.float32)
    for (a, n), p in zip(spans, ps):
        host[a:a + n] = p.reshape(-1)
    buf = torch.from_numpy(host).to(DEV)
    params = [torch.nn.Parameter(buf[a:a + n].view(p.shape)) for (a, n), p in zip(spans, ps)]
    assert all(q.data_ptr() % 256 == (4 if k == ac.OFFSET_ONE else 0) for k, q in enumerate(params))
    return buf, params, spans


def _set_grads(params, gs, layout, skip=()):
    """layout "flat": slices of one buffer at 64-float steps (what tgnn_backward leaves); "separate": one allocation each."""
    keep = [k for k in range(len(params)) if k not in skip]
    for k in skip:
        params[k].grad = None
    if layout == "flat":
        offs, off = {}, 0
        for k in keep:
            offs[k] = off
            off += (gs[k].size + 63) // 64 * 64
        host = np.full(max(off, 1), SENTINEL, dtype=np.float32)
        for k in keep:
            host[offs[k]:offs[k] + gs[k].size] = gs[k].reshape(-1)
        flat = torch.from_numpy(host).to(DEV)
        for k in keep:
            params[k].grad = flat[offs[k]:offs[k] + gs[k].size].view(gs[k].shape)
    else:
        for k in keep:
            params[k].grad = torch.from_numpy(np.array(gs[k])).to(DEV)


def _load_state(opt, params, t, ms, vs, only=None):
    """State as torch.optim.Adam keeps it after t - 1 steps, handed over through torch's own state_dict()."""
    ref = torch.optim.Adam(params, lr=1e-3)
    for k, q in enumerate(params):
        if only is None or k in only:
            ref.state[q] = ac.torch_state(t, ms[k], vs[k], DEV)
    sd = ref.state_dict()
    sd["param_groups"] = opt.state_dict()["param_groups"]
    opt.load_state_dict(sd)


def _outside(total, spans, touched):
    mask = np.ones(total, dtype=bool)
    for k in touched:
        a, n = spans[k]
        mask[a:a + n] = False
    return mask


@functools.lru_cache(maxsize=None)
def _case(t, lr, weight_decay=0.0):
    """Inputs and fp64 expectation of one single-step case: computed once, shared by the runs that need them, never written to."""
    ps, gs, ms, vs = ac.make_inputs(seed=11 + t % 5, t=t)
    want = [ac.adam64(ps[k], gs[k], ms[k], vs[k], t, lr, weight_decay) for k in range(len(ps))]
    for arr in (*ps, *gs, *ms, *vs):
        arr.setflags(write=False)
    return ps, gs, ms, vs, want


def _single_step(t, lr, layout, weight_decay=0.0):
    """One step of ours from the case's state -> (p', m', v') per stepped tensor, after the untouched bytes were checked."""
    ps, gs, ms, vs, _ = _case(t, lr, weight_decay)
    buf, params, spans = _arena(ps)
    opt = _adam(params, lr=lr, betas=ac.BETAS, eps=ac.EPS, weight_decay=weight_decay)
    if t > 1:
        _load_state(opt, params, t, ms, vs)
    ea, es, mspans = opt.flat_moments(0)
    assert all(a % 64 == 0 for a, _ in mspans) and [n for _, n in mspans] == [p.size for p in ps]
    assert ea.data_ptr() != es.data_ptr() and ea.numel() == es.numel() >= mspans[-1][0] + mspans[-1][1]
    pad = torch.from_numpy(_outside(ea.numel(), mspans, range(len(ps)))).to(DEV)
    ea[pad] = SENTINEL                                       # what lies between the moment slices must come back bit for bit
    es[pad] = SENTINEL
    _set_grads(params, gs, layout, skip=NO_GRAD)
    stepped = [k for k in range(len(ps)) if k not in NO_GRAD]
    before = _bits(buf), _bits(ea), _bits(es)
    steps_before = {k: float(opt.state[params[k]]["step"]) for k in range(len(ps)) if params[k] in opt.state}
    opt.step()
    torch.cuda.synchronize()
    assert opt.launches == 1 and opt.table_uploads == 1
    after = _bits(buf), _bits(ea), _bits(es)
    keep_p, keep_m = _outside(buf.numel(), spans, stepped), _outside(ea.numel(), mspans, stepped)
    assert np.array_equal(before[0][keep_p], after[0][keep_p]), "a byte outside the stepped parameters changed"
    assert np.array_equal(before[1][keep_m], after[1][keep_m]) and np.array_equal(before[2][keep_m], after[2][keep_m]), \
        "a byte outside the stepped moment slices changed"
    for k in NO_GRAD:                                        # skipped as torch skips them: no state appears, none advances
        if t == 1:
            assert params[k] not in opt.state
        else:
            assert float(opt.state[params[k]]["step"]) == steps_before[k] == t - 1
    out = {}
    for k in stepped:
        st = opt.state[params[k]]
        assert float(st["step"]) == t and st["step"].device.type == "cpu"
        a, n = mspans[k]
        if n:                                                # views into the flat buffers
            assert st["exp_avg"].data_ptr() == ea.data_ptr() + 4 * a and st["exp_avg_sq"].data_ptr() == es.data_ptr() + 4 * a
        assert st["exp_avg"].shape == params[k].shape == st["exp_avg_sq"].shape
        out[k] = tuple(x.detach().cpu().numpy() for x in (params[k], st["exp_avg"], st["exp_avg_sq"]))
    return out


@pytest.mark.parametrize("layout", ["flat", "separate"])
@pytest.mark.parametrize("lr", ac.LRS)
@pytest.mark.parametrize("t", ac.STEPS)
def test_single_step_against_fp64(t, lr, layout):
    from tilingnn_amd._lib import lib
    assert lib.tgnn_adam_chunk_elems() == ac.CHUNK
    want = _case(t, lr)[4]
    got = _single_step(t, lr, layout)
    worst = np.zeros(3)
    for k, (p, m, v) in got.items():
        rp, rm, rv = ac.gate_ratios(p, m, v, want[k])
        worst = np.maximum(worst, (rp, rm, rv))
    print(f"t {t}, lr {lr}, {layout}: worst error / gate = p {worst[0]:.3f}, m {worst[1]:.3f}, v {worst[2]:.3f}")
    for k, (p, m, v) in got.items():
        ac.assert_within_gates(p, m, v, want[k], f"tensor {k} {ac.SHAPES[k]}, t {t}, lr {lr}, {layout}")


@pytest.mark.parametrize("lr", ac.LRS)
@pytest.mark.parametrize("t", ac.STEPS)
def test_single_step_with_weight_decay_against_torch_on_the_device(t, lr):
    """weight_decay 1e-2: per tensor our largest error against fp64 is at most 4 x that of torch.optim.Adam(foreach=False) on the
    device for the same inputs, plus one ulp of the largest expected magnitude (another fused-multiply-add contraction, no more)."""
    wd = 1e-2
    ps, gs, ms, vs, want = _case(t, lr, wd)
    got = _single_step(t, lr, "flat", wd)
    ref_p, ref_m, ref_v = ac.torch_adam_step(ps, gs, ms, vs, t, lr, wd, device=DEV)
    for k, ours in got.items():
        if ps[k].size == 0:
            continue
        for name, mine, theirs in zip("pmv", ours, (ref_p[k], ref_m[k], ref_v[k])):
            w = want[k][name]
            e_ours = float(np.abs(mine.astype(np.float64) - w).max())
            e_torch = float(np.abs(theirs.astype(np.float64) - w).max())
            ulp = float(np.spacing(np.float32(np.abs(w).max())))
            print(f"t {t}, lr {lr}, tensor {k} {name}: ours {e_ours:.3e}, torch {e_torch:.3e}, ulp {ulp:.3e}")
            assert e_ours <= 4.0 * e_torch + ulp, (k, name, e_ours, e_torch, ulp)


# ---------------------------------------------------------------------------------------------- several steps
def _state_of(opt, q):
    st = opt.state.get(q)
    if not st:
        z = np.zeros(tuple(q.shape), np.float32)
        return 0, z, z
    return int(float(st["step"])), st["exp_avg"].detach().cpu().numpy(), st["exp_avg_sq"].detach().cpu().numpy()


def _forced_step(opt, params, gs, layout, skip=(), lrs=None, what=""):
    """One step of `opt`, every stepped tensor teacher forced from ITS OWN state before the step against fp64 (each at its own
    step count and its group's lr).  -> worst error / gate."""
    group_of = {id(q): g for g in opt.param_groups for q in g["params"]}
    prev = [(q.detach().cpu().numpy(), *_state_of(opt, q)) for q in params]
    _set_grads(params, gs, layout, skip=skip)
    opt.step()
    torch.cuda.synchronize()
    worst = np.zeros(3)
    for k, q in enumerate(params):
        p0, t0, m0, v0 = prev[k]
        t1, m1, v1 = _state_of(opt, q)
        if k in skip:
            assert t1 == t0 and np.array_equal(q.detach().cpu().numpy(), p0) and np.array_equal(m1, m0) and np.array_equal(v1, v0)
            continue
        assert t1 == t0 + 1
        group = group_of[id(q)]
        want = ac.adam64(p0, gs[k], m0, v0, t1, group["lr"] if lrs is None else lrs[k], group["weight_decay"], group["betas"], group["eps"])
        worst = np.maximum(worst, ac.assert_within_gates(q.detach().cpu().numpy(), m1, v1, want, f"{what} tensor {k}, step {t1}"))
    return worst


def _grad_sequence(n_steps, seed):
    return [ac.make_inputs(seed=seed + 13 * s, t=1)[1] for s in range(n_steps)]


def test_twenty_steps_walk_the_bias_corrections():
    ps = ac.make_inputs(seed=2, t=1)[0]
    _, params, _ = _arena(ps)
    twin = [torch.nn.Parameter(q.detach().clone()) for q in params]
    opt = _adam(params, lr=1e-2, betas=ac.BETAS, eps=ac.EPS)
    ref = torch.optim.Adam(twin, lr=1e-2, betas=ac.BETAS, eps=ac.EPS)
    worst = np.zeros(3)
    for s, gs in enumerate(_grad_sequence(20, seed=40)):
        worst = np.maximum(worst, _forced_step(opt, params, gs, "flat", what=f"step {s + 1}:"))
        _set_grads(twin, gs, "separate")
        ref.step()
        for q, r in zip(params, twin):                       # the step counts in `state` equal torch's after every step
            assert float(opt.state[q]["step"]) == float(ref.state[r]["step"]) == s + 1
            assert opt.state[q]["step"].dtype == ref.state[r]["step"].dtype
    print(f"20 steps: worst error / gate = p {worst[0]:.3f}, m {worst[1]:.3f}, v {worst[2]:.3f}")
    # a new flat gradient buffer at every step, the same distances inside it: ONE table for all twenty launches
    assert opt.launches == 20 and opt.table_uploads == 1


def _snapshot(opt, params):
    return [(_bits(q), *[_bits(opt.state[q][key]) if q in opt.state else None for key in ("exp_avg", "exp_avg_sq")]) for q in params]


def _same_bits(a, b):
    return all((x is None and y is None) or (x is not None and y is not None and np.array_equal(x, y))
               for ra, rb in zip(a, b) for x, y in zip(ra, rb))


def test_flat_and_uploaded_paths_give_the_same_bits_and_may_alternate():
    ps = ac.make_inputs(seed=5, t=1)[0]
    grads = _grad_sequence(7, seed=70)
    # (layout of the gradients, parameters without one) per step: both paths, switching, a changing set of Nones
    plan = [("flat", ()), ("flat", ()), ("separate", ()), ("flat", (3, 7)), ("separate", (5,)), ("flat", (3,)), ("flat", ())]
    opts, pars = [], []
    for _ in range(3):
        _, params, _ = _arena(ps)
        pars.append(params)
        opts.append(_adam(params, lr=1e-2, betas=ac.BETAS, eps=ac.EPS))
    mixed, always_flat, always_separate = opts
    for s, (layout, skip) in enumerate(plan):
        _forced_step(mixed, pars[0], grads[s], layout, skip=skip, what=f"mixed, step {s + 1}:")
        _set_grads(pars[1], grads[s], "flat", skip=skip)
        always_flat.step()
        _set_grads(pars[2], grads[s], "separate", skip=skip)
        always_separate.step()
        torch.cuda.synchronize()
        a, b, c = (_snapshot(o, p) for o, p in zip(opts, pars))
        assert _same_bits(a, b) and _same_bits(a, c), f"step {s + 1}: the paths differ"
    # after the Nones the step counts differ: one launch per distinct count (two at steps 5 and 6, three at step 7)
    counts = sorted({int(float(mixed.state[q]["step"])) for q in pars[0]})
    assert counts == [5, 6, 7]
    assert always_flat.table_uploads < always_flat.launches and mixed.launches == always_flat.launches == always_separate.launches
    assert mixed.launches == 1 + 1 + 1 + 1 + 2 + 2 + 3
    # a parameter that moved: the table follows it
    before = mixed.table_uploads
    _forced_step(mixed, pars[0], grads[0], "flat", what="before the move:")
    assert mixed.table_uploads == before                     # (same tables as the step before)
    q = pars[0][2]
    q.data = q.data.clone()
    _forced_step(mixed, pars[0], grads[1], "flat", what="after the move:")
    assert mixed.table_uploads == before + 1


def test_two_parameter_groups_follow_their_own_learning_rates():
    ps = ac.make_inputs(seed=6, t=1)[0]
    _, params, _ = _arena(ps)
    first = [k for k in range(len(params)) if k % 2 == 0]
    opt = _adam([{"params": [params[k] for k in first], "lr": 1e-2},
                 {"params": [params[k] for k in range(len(params)) if k % 2], "weight_decay": 0.0}], lr=1e-4, betas=ac.BETAS, eps=ac.EPS)
    grads = _grad_sequence(3, seed=90)
    lrs = [1e-2 if k in first else 1e-4 for k in range(len(params))]
    _forced_step(opt, params, grads[0], "flat", lrs=lrs, what="groups, step 1:")
    assert opt.launches == 2
    opt.param_groups[0]["lr"] *= 0.5                         # what a scheduler does: read at every step
    lrs = [5e-3 if k in first else 1e-4 for k in range(len(params))]
    _forced_step(opt, params, grads[1], "separate", lrs=lrs, what="groups, step 2:")
    _forced_step(opt, params, grads[2], "flat", lrs=lrs, what="groups, step 3:")
    assert opt.launches == 6
    sched_opt = _adam([torch.nn.Parameter(torch.ones(8, device=DEV))], lr=1e-2)
    sched = torch.optim.lr_scheduler.StepLR(sched_opt, step_size=1, gamma=0.5)
    sched_opt.param_groups[0]["params"][0].grad = torch.ones(8, device=DEV)
    sched_opt.step()
    sched.step()
    assert sched_opt.param_groups[0]["lr"] == 5e-3


# ---------------------------------------------------------------------------------------------- checkpoints
def _round_trip(sd):
    f = io.BytesIO()
    torch.save(sd, f)
    size = f.tell()
    f.seek(0)
    return torch.load(f), size


def _describe(sd):
    return {i: {k: (tuple(v.shape), v.dtype, v.device.type) for k, v in st.items()} for i, st in sd["state"].items()}


@pytest.mark.parametrize("direction", ["torch_to_ours", "ours_to_torch"])
def test_checkpoints_interchange_with_torch_adam(direction):
    ps = ac.make_inputs(seed=8, t=1)[0]
    grads = _grad_sequence(4, seed=120)
    make = {"ours": lambda par: _adam(par, lr=1e-2, betas=ac.BETAS, eps=ac.EPS),
            "torch": lambda par: torch.optim.Adam(par, lr=1e-2, betas=ac.BETAS, eps=ac.EPS)}
    src_kind, dst_kind = ("torch", "ours") if direction == "torch_to_ours" else ("ours", "torch")
    _, src_params, _ = _arena(ps)
    src = make[src_kind](src_params)
    for s in range(3):
        _set_grads(src_params, grads[s], "flat")
        src.step()
    loaded, src_size = _round_trip(src.state_dict())
    _, dst_params, _ = _arena([q.detach().cpu().numpy() for q in src_params])
    dst = make[dst_kind](dst_params)
    dst.load_state_dict(loaded)
    # the two state_dict()s describe the same thing: keys, shapes, dtypes, devices, group options
    a, b = src.state_dict(), dst.state_dict()
    assert _describe(a) == _describe(b) and len(a["state"]) == len(ps)
    assert [sorted(g) for g in a["param_groups"]] == [sorted(g) for g in b["param_groups"]]
    assert all(float(st["step"]) == 3 for st in b["state"].values())
    if dst_kind == "ours":
        ea, _, mspans = dst.flat_moments(0)
        assert all(dst.state[q]["exp_avg"].data_ptr() == ea.data_ptr() + 4 * a_ for q, (a_, n_) in zip(dst_params, mspans) if n_)
    # a checkpoint of ours is no larger than torch's: the flat buffers are written once, not once per view
    _, dst_size = _round_trip(b)
    ours_size, torch_size = (dst_size, src_size) if dst_kind == "ours" else (src_size, dst_size)
    print(f"{direction}: checkpoint of ours {ours_size} bytes, of torch.optim.Adam {torch_size} bytes")
    assert ours_size <= 1.05 * torch_size
    # one more step of each on the same gradients, both teacher forced from the state they share
    prev = [(q.detach().cpu().numpy(), *_state_of(src, q)) for q in src_params]
    for opt, params in ((src, src_params), (dst, dst_params)):
        _set_grads(params, grads[3], "separate")
        opt.step()
    torch.cuda.synchronize()
    for k in range(len(ps)):
        p0, t0, m0, v0 = prev[k]
        want = ac.adam64(p0, grads[3][k], m0, v0, t0 + 1, 1e-2)
        for opt, params, name in ((src, src_params, src_kind), (dst, dst_params, dst_kind)):
            t1, m1, v1 = _state_of(opt, params[k])
            assert t1 == 4
            ac.assert_within_gates(params[k].detach().cpu().numpy(), m1, v1, want, f"{direction}, {name}, tensor {k}")


# ---------------------------------------------------------------------------------------------- the whole network
def _tiny_network():
    from tilingnn_amd.graph_networks.networks.TilinGNN import TilinGNN
    from tilingnn_amd.weights import make_state_dict
    z = load_npz("tiny_graph.npz")
    g = dict(x=z["x"], adj=z["adj"], adj_attr=z["adj_attr"], col=z["col"], col_attr=z["col_attr"])
    fe = int(g["adj_attr"].shape[1])
    net = TilinGNN(adj_edge_features_dim=fe, network_depth=20, network_width=32, node_features_dim=3)
    net.load_state_dict(make_state_dict(fe, 20, 32, 1, 3, seed=3))
    return net.to(DEV).train(), graph_tensors(g, torch.float32, DEV)


def test_whole_network_step_takes_the_flat_path(tmp_path):
    from tilingnn_amd.solver.ml_solver.losses import Losses
    from tilingnn_amd.solver.ml_solver.trainer import Trainer
    net, (x, adj, attr, col, _) = _tiny_network()
    net.autograd = True
    params = list(net.parameters())
    # the depth-20 network's table of 544 tensors: 386 of them trainable parameters (the rest are BatchNorm buffers)
    from tilingnn_amd import _lib
    assert len(_lib.param_names(net._dims())) == 544 and len(params) == 386
    opt = _adam(params, lr=1e-3)

    def backward():
        opt.zero_grad()
        probs, _ = net(x, adj, attr, col)
        loss, *_ = Losses.calculate_unsupervised_loss(probs, x, col, adj_edges_index=adj, adj_edge_features=attr)
        loss.backward()
        return probs.detach().clone()

    probs0 = backward()
    # every gradient is a slice of the backward's ONE buffer (no clone by autograd)
    assert all(q.grad is not None for q in params) and len({q.grad.untyped_storage().data_ptr() for q in params}) == 1
    twin_params = [torch.nn.Parameter(q.detach().clone()) for q in params]      # (a copy of the network's parameters: it never runs)
    for q, r in zip(params, twin_params):
        r.grad = q.grad.detach().clone()
    ref = torch.optim.Adam(twin_params, lr=1e-3, foreach=False)
    prev = [(q.detach().cpu().numpy(), q.grad.detach().cpu().numpy()) for q in params]
    opt.step()
    ref.step()
    torch.cuda.synchronize()
    assert opt.launches == 1 and opt.table_uploads == 1
    worst = np.zeros(3)
    for k, (q, r) in enumerate(zip(params, twin_params)):
        p0, g0 = prev[k]
        zero = np.zeros_like(p0)
        want = ac.adam64(p0, g0, zero, zero, 1, 1e-3)
        worst = np.maximum(worst, ac.assert_within_gates(q.detach().cpu().numpy(), *_state_of(opt, q)[1:], want, f"ours, parameter {k}"))
        ac.assert_within_gates(r.detach().cpu().numpy(), *_state_of(ref, r)[1:], want, f"torch, parameter {k}")
    print(f"{len(params)} parameters: worst error / gate = p {worst[0]:.3f}, m {worst[1]:.3f}, v {worst[2]:.3f}")
    # the next backward writes into a new buffer at the same distances: a new base pointer, no new table
    probs1 = backward()
    assert torch.isfinite(probs1).all() and not torch.equal(probs1, probs0)
    opt.step()
    assert opt.launches == 2 and opt.table_uploads == 1
    # a checkpoint of the network's moments is no larger than torch's
    assert _round_trip(opt.state_dict())[1] <= 1.05 * _round_trip(ref.state_dict())[1]
    # Trainer.train_step takes it like any optimizer
    layout = types.SimpleNamespace(node_feature=x, align_edge_index=adj, align_edge_features=attr, collide_edge_index=col)
    loss = Trainer(None, None, DEV, net, str(tmp_path)).train_step(layout, opt)
    assert loss is not None and torch.isfinite(loss) and opt.launches == 3 and opt.table_uploads == 1


# ---------------------------------------------------------------------------------------------- refusals
def test_refusals_name_the_cause_and_change_nothing():
    good = torch.nn.Parameter(torch.ones(4, 6, device=DEV))
    with pytest.raises(TypeError, match="parameter 1 .*float16"):
        _adam([good, torch.nn.Parameter(torch.ones(4, device=DEV, dtype=torch.float16))])
    with pytest.raises(ValueError, match="parameter 1 .*cpu"):
        _adam([good, torch.nn.Parameter(torch.ones(4))])
    with pytest.raises(ValueError, match="parameter 2 .*contiguous"):
        _adam([good, torch.nn.Parameter(torch.ones(3, device=DEV)), torch.nn.Parameter(torch.ones(6, 4, device=DEV).t())])
    with pytest.raises(NotImplementedError, match="amsgrad"):
        _adam([good], amsgrad=True)
    with pytest.raises(NotImplementedError, match="maximize"):
        _adam([good], maximize=True)
    with pytest.raises(NotImplementedError, match="tensor lr"):
        _adam([good], lr=torch.tensor(1e-3))
    with pytest.raises(NotImplementedError, match="amsgrad"):
        _adam([{"params": [good], "amsgrad": True}])

    ps = ac.make_inputs(seed=9, t=1)[0][:6]
    grads = _grad_sequence(2, seed=150)
    buf, params, _ = _arena(ps)
    opt = _adam(params, lr=1e-2)
    extra = torch.nn.Parameter(torch.ones(5, device=DEV))
    probe = _adam(params[:2], lr=1e-2)
    probe.add_param_group({"params": [extra], "lr": 1e-3})   # before the first step: fine
    assert len(probe.param_groups) == 2
    _set_grads(params, [g for g in grads[0][:6]], "flat")
    opt.step()
    torch.cuda.synchronize()

    def frozen():
        ea, es, _ = opt.flat_moments(0)
        return _bits(buf), _bits(ea), _bits(es), [float(opt.state[q]["step"]) for q in params], len(opt.param_groups)

    def unchanged(was):
        torch.cuda.synchronize()
        now = frozen()
        return all(np.array_equal(a, b) for a, b in zip(was[:3], now[:3])) and was[3:] == now[3:]

    was = frozen()
    _set_grads(params, [g for g in grads[1][:6]], "separate")
    idx = torch.tensor([[0, 2]], device=DEV)
    params[3].grad = torch.sparse_coo_tensor(idx, torch.ones(2, device=DEV), size=tuple(params[3].shape))
    with pytest.raises(RuntimeError, match="sparse"):
        opt.step()
    assert unchanged(was)
    with pytest.raises(NotImplementedError, match="add_param_group"):
        opt.add_param_group({"params": [extra]})
    assert unchanged(was)
    opt.param_groups[0]["amsgrad"] = True
    params[3].grad = torch.ones_like(params[3])
    with pytest.raises(NotImplementedError, match="amsgrad"):
        opt.step()
    opt.param_groups[0]["amsgrad"] = False
    assert unchanged(was)
    opt.step()                                               # ... and the optimizer is still usable
    assert not unchanged(was) and [float(opt.state[q]["step"]) for q in params] == [2.0] * 6
