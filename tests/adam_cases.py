"""Inputs, fp64 expectation and gates of the fused Adam step's tests (tests/test_adam_fused.py on the GPU; tests/test_adam_plan_host.py
points the same gates at torch's own CPU Adam first, so that they are known to be passable by the reference).

The expectation is the fp64 evaluation of

    g  = grad (+ weight_decay p)        m' = b1 m + (1 - b1) g        v' = b2 v + (1 - b2) g g
    p' = p - step_size m' / (sqrt(v') rsqrt_bc2 + eps),   step_size = lr / (1 - b1^t),  rsqrt_bc2 = 1 / sqrt(1 - b2^t)

on the SAME fp32 inputs (teacher forced: one step from given state).  Gates, U = 2^-24, weight_decay 0:

    |m' - m'64| <= 6 U (|b1 m| + |(1 - b1) g|) =: tau_m
    |v' - v'64| <= 6 U (b2 v + (1 - b2) g^2)
    |p' - p'64| <= 2 U |p'64| + 8 U |upd64| + 4 step_size tau_m / den64

The constants count roundings (the fp32 hyper-parameters, the products, the sum; the square root, the scaling, the eps, the
quotient, the step size, the final subtraction); the last term is the cancellation in m' carried through the quotient.
"""
import math

import numpy as np
import torch

U = 2.0 ** -24
CHUNK = 4096                                   # kAdamChunk of tilingnn_amd/csrc/adam_plan.h (the GPU test checks the library's value)
SIZES = [(0,), (1,), (3,), (4,), (5,), (63,), (64,), (65,), (CHUNK - 1,), (CHUNK,), (CHUNK + 1,), (2 * CHUNK + 7,), (256, 672)]
OFFSET_ONE = len(SIZES)                        # index of the extra tensor that sits one float off a 16-byte boundary
SHAPES = SIZES + [(65,)]
STEPS = (1, 2, 10, 1000, 100000)               # 1 = fresh state; the others = loaded state that has seen t - 1 steps
LRS = (1e-4, 1e-2)
BETAS, EPS = (0.9, 0.999), 1e-8
GRAD_SCALES = 10.0 ** np.linspace(-8, 2, len(SHAPES))
GUARD = 64                                     # floats of guard band on each side of a parameter


def numel(shape):
    return int(np.prod(shape))


def make_inputs(seed, t):
    """-> (p, g, m, v): lists of fp32 arrays, one per SHAPES entry.  Gradient scales from 1e-8 to 1e2, every fifth gradient
    element exactly zero; t == 1: zero moments, else moments of the size t - 1 steps on such gradients leave."""
    rng = np.random.default_rng(seed)
    ps, gs, ms, vs = [], [], [], []
    for k, shape in enumerate(SHAPES):
        n, s = numel(shape), GRAD_SCALES[(k + seed) % len(SHAPES)]
        p = (0.1 * rng.standard_normal(n)).astype(np.float32)
        g = (s * rng.standard_normal(n)).astype(np.float32)
        g[::5] = 0.0
        if t == 1:
            m, v = np.zeros(n, np.float32), np.zeros(n, np.float32)
        else:
            m = (0.5 * s * rng.standard_normal(n)).astype(np.float32)
            v = ((s * s) * (0.05 + rng.random(n))).astype(np.float32)
            v[1::7] = 0.0                      # (a second moment that has seen only zero gradients)
        ps.append(p.reshape(shape)), gs.append(g.reshape(shape)), ms.append(m.reshape(shape)), vs.append(v.reshape(shape))
    return ps, gs, ms, vs


def adam64(p, g, m, v, t, lr, weight_decay=0.0, betas=BETAS, eps=EPS):
    """One step in fp64 -> dict(p, m, v, tau_p, tau_m, tau_v)."""
    b1, b2 = betas
    p, g, m, v = (np.asarray(a, dtype=np.float64) for a in (p, g, m, v))
    if weight_decay:
        g = g + weight_decay * p
    m2 = b1 * m + (1.0 - b1) * g
    v2 = b2 * v + (1.0 - b2) * g * g
    step_size = lr / (1.0 - b1 ** t)
    den = np.sqrt(v2) * (1.0 / math.sqrt(1.0 - b2 ** t)) + eps
    upd = step_size * m2 / den
    p2 = p - upd
    tau_m = 6 * U * (np.abs(b1 * m) + np.abs((1.0 - b1) * g))
    tau_v = 6 * U * (b2 * v + (1.0 - b2) * g * g)
    tau_p = 2 * U * np.abs(p2) + 8 * U * np.abs(upd) + 4 * step_size * tau_m / den
    return dict(p=p2, m=m2, v=v2, tau_p=tau_p, tau_m=tau_m, tau_v=tau_v)


def gate_ratios(got_p, got_m, got_v, want):
    """Largest |got - want| / tau over the tensor for (p, m, v); an error where tau == 0 must be 0 and counts as inf."""
    out = []
    for key, got in (("p", got_p), ("m", got_m), ("v", got_v)):
        err = np.abs(np.asarray(got, dtype=np.float64) - want[key])
        tau = want["tau_" + key]
        if err.size == 0:
            out.append(0.0)
            continue
        r = np.where(err == 0.0, 0.0, err / np.where(tau > 0.0, tau, 1.0))
        r = np.where((tau == 0.0) & (err > 0.0), np.inf, r)
        out.append(float(r.max()))
    return tuple(out)


def assert_within_gates(got_p, got_m, got_v, want, what):
    rp, rm, rv = gate_ratios(got_p, got_m, got_v, want)
    assert rp <= 1.0 and rm <= 1.0 and rv <= 1.0, f"{what}: error / gate = p {rp:.3f}, m {rm:.3f}, v {rv:.3f}"
    return rp, rm, rv


def torch_state(t, m, v, device="cpu"):
    """What torch.optim.Adam (non-capturable, non-fused) keeps for a parameter that has seen t - 1 steps."""
    return {"step": torch.tensor(float(t - 1)), "exp_avg": torch.from_numpy(np.array(m)).to(device),
            "exp_avg_sq": torch.from_numpy(np.array(v)).to(device)}


def torch_adam_step(ps, gs, ms, vs, t, lr, weight_decay=0.0, device="cpu"):
    """One step of torch.optim.Adam(foreach=False) from the given state on `device` -> lists (p', m', v') of numpy arrays."""
    params = [torch.nn.Parameter(torch.from_numpy(np.array(p)).to(device)) for p in ps]
    opt = torch.optim.Adam(params, lr=lr, betas=BETAS, eps=EPS, weight_decay=weight_decay, foreach=False)
    for q, g, m, v in zip(params, gs, ms, vs):
        q.grad = torch.from_numpy(np.array(g)).to(device)
        if t > 1:
            opt.state[q] = torch_state(t, m, v, device)
    opt.step()
    out = ([q.detach().cpu().numpy() for q in params], [opt.state[q]["exp_avg"].cpu().numpy() for q in params],
           [opt.state[q]["exp_avg_sq"].cpu().numpy() for q in params])
    assert all(float(opt.state[q]["step"]) == t for q in params)
    return out
