"""Fused Adam: `torch.optim.Adam`'s update of a whole parameter group in ONE kernel launch (csrc/adam.hip).

    optimizer = tilingnn_amd.optim.Adam(network.parameters(), lr=1e-3)          # network_train.py:27

The arithmetic is torch's non-capturable single-tensor Adam in fp32; `state_dict()` / `load_state_dict()` interchange with
`torch.optim.Adam` in both directions.  The moments of a group live in two flat buffers (`state[p]["exp_avg"]` and
`state[p]["exp_avg_sq"]` are views into them), the kernel reads a device-resident table of (parameter, gradient offset, moment
offset, size) segments cut into equal chunks of work.  The table is built once: a step whose gradients sit at the same distances
from each other as at the step before -- always the case behind `tgnn_backward`, which writes every gradient into one flat
buffer -- passes a new base pointer and nothing else: no upload, no copy, no host synchronisation.  Otherwise (gradients from
torch's autograd, hand-assigned `.grad`, another set of `None`s, parameters that moved) the table is rebuilt and uploaded on the
stream.  Not supported, refused by name: amsgrad, maximize, a tensor `lr`, decoupled weight decay, capturable / graph-captured
steps, sparse gradients, parameters that are not contiguous fp32 on a GPU.
"""
from __future__ import annotations

import ctypes as C
import math

import torch

from . import _lib
from ._lib import check, lib

try:
    from torch.optim.optimizer import _get_scalar_dtype
except ImportError:                                  # pragma: no cover
    def _get_scalar_dtype():
        return torch.float64 if torch.get_default_dtype() == torch.float64 else torch.float32

__all__ = ["Adam"]

MOMENT_ALIGN = 64            # floats: kAdamMomentAlign of csrc/adam_plan.h
_MAX_TABLES = 32             # cached tables per group (one per set of parameters stepped together)


class _Table:
    """One uploaded segment + chunk table: the parameters' and gradients' addresses it was built for."""
    __slots__ = ("pptrs", "goffs", "host", "dev", "n_segments", "n_chunks")


class _GroupState:
    """Flat moments and step counts of one parameter group."""

    def __init__(self, params):
        self.params = list(params)
        self.device = self.params[0].device if self.params else None
        self.numel = [int(p.numel()) for p in self.params]
        self.moment_off, off = [], 0
        for n in self.numel:
            self.moment_off.append(off)
            off += (n + MOMENT_ALIGN - 1) // MOMENT_ALIGN * MOMENT_ALIGN
        self.moment_floats = off
        self.exp_avg = torch.zeros(max(off, 1), dtype=torch.float32, device=self.device)
        self.exp_avg_sq = torch.zeros(max(off, 1), dtype=torch.float32, device=self.device)
        self.steps = torch.zeros(max(len(self.params), 1), dtype=_get_scalar_dtype())     # host, as torch keeps `step`
        self.steps_np = self.steps.numpy()
        self.has_state = [False] * len(self.params)
        self.tables = {}

    def views(self, i):
        a, n, shape = self.moment_off[i], self.numel[i], self.params[i].shape
        return self.steps[i], self.exp_avg[a:a + n].view(shape), self.exp_avg_sq[a:a + n].view(shape)


def _refuse_options(group) -> None:
    for key in ("amsgrad", "maximize"):
        if group.get(key):
            raise NotImplementedError(f"tilingnn_amd.optim.Adam does not implement {key}=True")
    if isinstance(group.get("lr"), torch.Tensor):
        raise NotImplementedError("tilingnn_amd.optim.Adam does not implement a tensor lr (pass a float)")
    if group.get("decoupled_weight_decay"):
        raise NotImplementedError("tilingnn_amd.optim.Adam does not implement decoupled_weight_decay=True (AdamW)")
    if group.get("capturable") or group.get("differentiable"):
        raise NotImplementedError("tilingnn_amd.optim.Adam does not implement capturable=True / differentiable=True")


def _check_param(p, index) -> None:
    if p.dtype is not torch.float32:
        raise TypeError(f"tilingnn_amd.optim.Adam: parameter {index} is {p.dtype}, only torch.float32 is supported")
    if not p.is_cuda:
        raise ValueError(f"tilingnn_amd.optim.Adam: parameter {index} is on {p.device}, not on a GPU")
    if not p.is_contiguous():
        raise ValueError(f"tilingnn_amd.optim.Adam: parameter {index} is not contiguous")


class Adam(torch.optim.Optimizer):
    """Drop-in for `torch.optim.Adam(params, lr, betas, eps, weight_decay)`; see the module's docstring.

    `table_uploads` counts the segment tables built and uploaded so far, `launches` the kernel launches."""

    def __init__(self, params, lr=1e-3, betas=(0.9, 0.999), eps=1e-8, weight_decay=0, amsgrad=False, *, maximize=False):
        if not isinstance(lr, torch.Tensor) and lr < 0.0:
            raise ValueError(f"Invalid learning rate: {lr}")
        if eps < 0.0:
            raise ValueError(f"Invalid epsilon value: {eps}")
        if not 0.0 <= betas[0] < 1.0:
            raise ValueError(f"Invalid beta parameter at index 0: {betas[0]}")
        if not 0.0 <= betas[1] < 1.0:
            raise ValueError(f"Invalid beta parameter at index 1: {betas[1]}")
        if weight_decay < 0.0:
            raise ValueError(f"Invalid weight_decay value: {weight_decay}")
        # (the keys torch.optim.Adam keeps in a group, so that the two state_dict()s interchange; the last five are fixed)
        defaults = dict(lr=lr, betas=betas, eps=eps, weight_decay=weight_decay, amsgrad=amsgrad, maximize=maximize, foreach=None,
                        capturable=False, differentiable=False, fused=None, decoupled_weight_decay=False)
        _refuse_options(defaults)
        self._groups = {}            # index of the group -> _GroupState, made at the group's first step (or on load)
        self.table_uploads = 0
        self.launches = 0
        super().__init__(params, defaults)

    # ------------------------------------------------------------------------------------------ groups
    def add_param_group(self, param_group):
        if self.__dict__.get("_groups") or len(self.state):
            raise NotImplementedError("tilingnn_amd.optim.Adam: add_param_group after the first step (the flat moment buffers "
                                      "are laid out): build a new optimizer and load_state_dict into it")
        first = sum(len(g["params"]) for g in self.param_groups)
        super().add_param_group(param_group)
        group = self.param_groups[-1]
        try:
            _refuse_options(group)
            for j, p in enumerate(group["params"]):
                _check_param(p, first + j)
            if len({p.device for p in group["params"]}) > 1:
                raise ValueError("tilingnn_amd.optim.Adam: the parameters of one group must be on one device")
        except Exception:
            self.param_groups.pop()
            raise

    def __setstate__(self, state):
        super().__setstate__(state)
        self._groups = {}            # (unpickled / loaded state: adopted into fresh flat buffers on first use)
        self.__dict__.setdefault("table_uploads", 0)
        self.__dict__.setdefault("launches", 0)

    def _group_state(self, gi, group) -> _GroupState:
        gs = self._groups.get(gi)
        if gs is not None and len(gs.params) == len(group["params"]) and all(a is b for a, b in zip(gs.params, group["params"])):
            return gs
        first = sum(len(g["params"]) for g in self.param_groups[:gi])
        for j, p in enumerate(group["params"]):
            _check_param(p, first + j)
        gs = _GroupState(group["params"])
        # state that is already there (load_state_dict, unpickling): moved into the flat buffers, the entries become views
        for i, p in enumerate(gs.params):
            st = self.state.get(p)
            if not st:
                continue
            step, m, v = gs.views(i)
            m.copy_(st["exp_avg"])
            v.copy_(st["exp_avg_sq"])
            gs.steps_np[i] = float(st["step"])
            st["step"], st["exp_avg"], st["exp_avg_sq"] = step, m, v
            gs.has_state[i] = True
        self._groups[gi] = gs
        return gs

    def flat_moments(self, group=0):
        """(exp_avg, exp_avg_sq, spans) of a parameter group: the two flat moment buffers and, per parameter of the group, the
        (offset, numel) of its slice in both (slices start on 64-float boundaries; what lies between them is never touched)."""
        gs = self._group_state(group, self.param_groups[group])
        return gs.exp_avg, gs.exp_avg_sq, list(zip(gs.moment_off, gs.numel))

    def load_state_dict(self, state_dict):
        for group in state_dict["param_groups"]:
            _refuse_options(group)
        for st in state_dict["state"].values():
            if "max_exp_avg_sq" in st:
                raise NotImplementedError("tilingnn_amd.optim.Adam does not implement amsgrad=True (state has max_exp_avg_sq)")
        super().load_state_dict(state_dict)
        self._groups = {}
        with torch.no_grad():
            for gi, group in enumerate(self.param_groups):
                group["foreach"], group["fused"] = None, None                    # (torch's choice of loop: not ours to keep)
                self._group_state(gi, group)

    # ------------------------------------------------------------------------------------------ the step
    @torch.no_grad()
    def step(self, closure=None):
        loss = None
        if closure is not None:
            with torch.enable_grad():
                loss = closure()
        # first everything that can refuse, then the launches: a refused step changes nothing
        work = []
        for gi, group in enumerate(self.param_groups):
            _refuse_options(group)
            params = group["params"]
            grads = [p.grad for p in params]
            idx = [i for i, g in enumerate(grads) if g is not None]
            if not idx:
                continue
            for i in idx:
                g = grads[i]
                if g.layout is not torch.strided:
                    raise RuntimeError("tilingnn_amd.optim.Adam does not support sparse gradients")
                if g.dtype is not torch.float32:
                    raise TypeError(f"tilingnn_amd.optim.Adam: a gradient of group {gi} is {g.dtype}, only torch.float32 is supported")
                if not g.is_contiguous():
                    grads[i] = g.contiguous()
            work.append((gi, group, grads, idx))
        for gi, group, grads, idx in work:
            gs = self._group_state(gi, group)
            for i in idx:
                if not gs.has_state[i]:
                    step, m, v = gs.views(i)
                    self.state[gs.params[i]] = {"step": step, "exp_avg": m, "exp_avg_sq": v}
                    gs.has_state[i] = True
            whole = len(idx) == len(gs.params)
            counts = gs.steps_np[:len(gs.params)] if whole else gs.steps_np[idx]
            first = counts[0]
            if (counts == first).all():
                self._launch(group, gs, idx, grads, int(first) + 1)
            else:
                for t in sorted(set(counts.tolist())):
                    self._launch(group, gs, [i for i, c in zip(idx, counts) if c == t], grads, int(t) + 1)
            if whole:
                gs.steps_np[:len(gs.params)] += 1
            else:
                gs.steps_np[idx] += 1
        return loss

    def _launch(self, group, gs, sub, grads, t) -> None:
        sub = [i for i in sub if gs.numel[i]]
        if not sub:
            return
        key = tuple(sub)
        params = gs.params
        pptrs = tuple([params[i].data_ptr() for i in sub])
        gptrs = [grads[i].data_ptr() for i in sub]
        base = gptrs[0]
        goffs = tuple([q - base for q in gptrs])
        tab = gs.tables.get(key)
        if tab is None or tab.pptrs != pptrs or tab.goffs != goffs:
            tab = self._build_table(gs, sub, pptrs, goffs)
            if len(gs.tables) >= _MAX_TABLES:
                gs.tables.clear()
            gs.tables[key] = tab
        lr = group["lr"]
        beta1, beta2 = group["betas"]
        step_size = lr / (1.0 - beta1 ** t)
        rsqrt_bc2 = 1.0 / math.sqrt(1.0 - beta2 ** t)
        check(lib.tgnn_adam_step(tab.host.data_ptr(), tab.dev.data_ptr(), tab.n_segments, tab.n_chunks, base,
                                 gs.exp_avg.data_ptr(), gs.exp_avg_sq.data_ptr(), gs.moment_floats, step_size, rsqrt_bc2,
                                 float(beta1), float(beta2), float(group["eps"]), float(group["weight_decay"]),
                                 _lib.current_stream(gs.device)))
        self.launches += 1

    def _build_table(self, gs, sub, pptrs, goffs) -> _Table:
        n = len(sub)
        for i in sub:                                        # (a parameter that moved may have changed in kind as well)
            p = gs.params[i]
            _check_param(p, i)
            if p.device != gs.device:
                raise RuntimeError(f"tilingnn_amd.optim.Adam: parameter {i} of its group moved to {p.device}; the moments are on "
                                   f"{gs.device} (build a new optimizer and load_state_dict into it)")
        i64n = C.c_int64 * n
        numel = i64n(*[gs.numel[i] for i in sub])
        n_chunks = int(lib.tgnn_adam_chunk_count(numel, n))
        if n_chunks < 0:
            raise ValueError("tilingnn_amd.optim.Adam: more chunks of work than one launch holds")
        nbytes = int(lib.tgnn_adam_table_bytes(n, n_chunks))
        tab = _Table()
        tab.pptrs, tab.goffs, tab.n_segments = pptrs, goffs, n
        # a fresh pinned image per table: the copy below is stream-ordered, nothing may overwrite its source while it is in flight
        tab.host = torch.empty(nbytes, dtype=torch.uint8, pin_memory=True)
        out = C.c_int64(0)
        check(lib.tgnn_adam_table_build((C.c_void_p * n)(*pptrs), i64n(*goffs), i64n(*[gs.moment_off[i] for i in sub]), numel, n,
                                        gs.moment_floats, tab.host.data_ptr(), nbytes, C.byref(out)))
        tab.n_chunks = int(out.value)
        tab.dev = torch.empty(nbytes, dtype=torch.uint8, device=gs.device)
        tab.dev.copy_(tab.host, non_blocking=True)
        self.table_uploads += 1
        return tab
