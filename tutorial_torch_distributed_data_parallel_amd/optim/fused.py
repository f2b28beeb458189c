"""Fused SGD / Adam / AdamW (torch.optim-compatible).

The reference steps ``torch.optim.Adam(ddp_model.parameters(), lr=0.001)``
(REF/multi-GPU-training-torch.py:249, REF/multi-GPU-training-accelerate.py:126); the north star
adds a fused SGD. All are ``torch.optim.Optimizer`` subclasses (param_groups, state_dict,
load_state_dict, LR schedulers all work) whose ``step`` is:
  * FLAT  -- when the group's parameters are exactly one ParamArena (every DDP model, or any model
             passed through ``flatten_module``) and each .grad is its arena view: ONE kernel over
             the whole arena, optimizer state kept in arena-shaped flat buffers
             (state[p][...] are views into them);
  * MULTI -- otherwise: one launch over a device-side chunk table of the individual tensors;
  * CPU   -- torch's own single-tensor implementation (reference path for the CPU tests).
Semantics are torch's (TORCH/optim/sgd.py, TORCH/optim/adam.py): momentum buffer initialised to
the first gradient, dampening, nesterov, maximize, L2 vs decoupled weight decay, amsgrad,
bias-corrected Adam with a per-parameter step counter.

LAMB and LARS (torch has neither; their docstrings are the specification) keep the same three
paths, but a step is three launches: their update is not elementwise (``_LayerwiseBase``).
``_FusedBase`` owns the host state machine around the kernel calls, shared by all of them.
"""
from __future__ import annotations

import functools
import weakref

import torch
from torch.optim import Optimizer
from torch.optim.optimizer import _global_optimizer_post_hooks, _global_optimizer_pre_hooks

from .._native import native
from ..parallel.arena import arena_of


def _flat_arena(group, ps):
    """The arena a FLAT step of ``group`` runs over: every parameter has a gradient (``ps``, the
    ones that do, is all of them), they are exactly one arena, each .grad is its arena view."""
    params = group["params"]
    if len(ps) != len(params):
        return None
    a = arena_of(params)
    if a is None:
        return None
    for i in range(len(a.params)):
        if not a.is_arena_grad(i):
            return None
    return a


def _hooks_or_profiler(opt) -> bool:
    return bool(_global_optimizer_pre_hooks or _global_optimizer_post_hooks or
                opt._optimizer_step_pre_hooks or opt._optimizer_step_post_hooks or
                torch.autograd.profiler._is_profiler_enabled)


def _lean_step_hook(func):
    """torch wraps ``step`` (TORCH/optim/optimizer.py ``profile_hook_step``) in a record_function
    range plus the hook dispatch on EVERY call: ~10 us of host time per training step, and the
    eager toy-MLP step is host-bound right after the loss (profiles/host_overhead.md). Same
    behaviour, paid only when a hook is registered or the profiler is on."""

    @functools.wraps(func)
    def wrapper(self, *args, **kwargs):
        if _hooks_or_profiler(self):
            return Optimizer.profile_hook_step(func)(self, *args, **kwargs)
        out = func(self, *args, **kwargs)
        self._optimizer_step_code()
        return out

    wrapper.hooked = True  # torch's _patch_step_function leaves a hooked step alone
    return wrapper


_LIVE = weakref.WeakSet()  # optimizers that own device hyper blocks (CapturedStep re-syncs them)


def hyper_slots() -> dict:
    """Slot indices of the device hyper block (csrc/kernels.h HyperSlot)."""
    global _SLOTS
    if _SLOTS is None:
        _SLOTS = dict(native().hyper_slots())
    return _SLOTS


_SLOTS = None


def sync_all_hyper() -> None:
    """Push host-side hyper-parameter changes (LR schedulers, ...) of every live optimizer into
    its device hyper block; called before each hipGraph replay (train/graph.py)."""
    for opt in list(_LIVE):
        opt.sync_hyper()


def _dense(t: torch.Tensor) -> torch.Tensor:
    """A 1-D view of ``t``'s memory in storage order (no copy): the elementwise optimizer kernels
    only need p, grad and state to share one element order. Dense row-major tensors and
    channels_last conv weights (the native convolutions' parameter layout) qualify."""
    if t.is_contiguous():
        return t.view(-1)
    if t.dim() == 4 and t.is_contiguous(memory_format=torch.channels_last):
        return t.permute(0, 2, 3, 1).view(-1)
    raise RuntimeError(f"optimizer tensor with unsupported strides {tuple(t.stride())}")


def _grad_like(p: torch.Tensor) -> torch.Tensor:
    """``p.grad`` flattened in ``p``'s element order (converted only if its layout differs)."""
    g = p.grad
    if p.is_contiguous():
        return g.contiguous().view(-1)
    return _dense(g.contiguous(memory_format=torch.channels_last))


def _closure_loss(closure):
    with torch.enable_grad():
        return closure()


def _step_of(st) -> int:
    """A parameter's host step count (a tensor, a plain number, or missing = 0)."""
    s = st.get("step")
    return int(s.item()) if torch.is_tensor(s) else int(s or 0)


def _adam_scalars(g) -> tuple:
    b1, b2 = g["betas"]
    return (float(g["lr"]), float(b1), float(b2), float(g["weight_decay"]), float(g["eps"]))


def _momentum_cpu(st, d, momentum, dampening, nesterov):
    """torch-SGD momentum on the CPU: the buffer starts as the first direction ``d``; returns
    the direction to apply."""
    buf = st.get("momentum_buffer")
    if buf is None:
        buf = d.clone()
        st["momentum_buffer"] = buf
    else:
        buf.mul_(momentum).add_(d, alpha=1 - dampening)
    return d.add(buf, alpha=momentum) if nesterov else buf


class _FusedBase(Optimizer):
    _state_keys: tuple = ()
    _kind = 0  # hyper-block kind: 1 first-step flag (SGD, LARS), 2 step count too (Adam, LAMB)

    def __init__(self, params, defaults):
        super().__init__(params, defaults)
        self._flat_bufs = {}  # id(arena) -> {key: flat tensor}
        self._flat_step = {}  # id(arena) -> int step shared by every arena parameter (Adam)
        self._blocks = {}     # group index -> [device hyper block, host copy of its scalars]

    def __init_subclass__(cls, **kwargs):
        super().__init_subclass__(**kwargs)
        if "step" in cls.__dict__ and not getattr(cls.__dict__["step"], "hooked", False):
            cls.step = _lean_step_hook(cls.__dict__["step"])

    # ------------------------------------------------------------------ device hyper block
    def _scalars(self, g) -> tuple:
        raise NotImplementedError

    def hyper_block(self, gi: int = 0, device=None, step: int = 0,
                    first: bool = False) -> torch.Tensor:
        """The device-resident hyper-parameter block of parameter group ``gi`` (created on first
        use with step count ``step``; ``first`` = the next step initialises the SGD momentum
        buffers). Kernels read lr / momentum / betas / bias corrections from it, so a captured
        hipGraph replays with the current values (csrc/kernels.h HyperSlot)."""
        ent = self._blocks.get(gi)
        if ent is not None:
            return ent[0]
        S = hyper_slots()
        g = self.param_groups[gi]
        dev = device if device is not None else g["params"][0].device
        vals = self._scalars(g)
        host = torch.zeros(S["size"], dtype=torch.float32)
        host[:len(vals)] = torch.tensor(vals, dtype=torch.float64).float()
        host[S["scale"]] = 1.0
        host[S["first_next"]] = 1.0 if first else 0.0
        host.view(torch.int32)[S["step"]] = int(step)
        blk = host.to(dev)
        self._blocks[gi] = [blk, vals]
        _LIVE.add(self)
        return blk

    def sync_hyper(self) -> None:
        """Stream-ordered write of changed scalars (lr, momentum / betas, weight decay, eps) into
        the device blocks. Nothing is issued when nothing changed."""
        for gi, ent in self._blocks.items():
            vals = self._scalars(self.param_groups[gi])
            if vals == ent[1]:
                continue
            blk = ent[0]
            if blk.is_cuda and torch.cuda.is_current_stream_capturing():
                raise RuntimeError("hyper-parameters changed while a hipGraph was being captured")
            src = torch.tensor(vals, dtype=torch.float64).float()
            if blk.is_cuda:
                blk[:len(vals)].copy_(src.pin_memory(), non_blocking=True)
            else:
                blk[:len(vals)].copy_(src)
            ent[1] = vals

    def device_step(self, gi: int = 0):
        """Step count held by the device block of group ``gi`` (None without a block). Reading
        it synchronises with the device."""
        ent = self._blocks.get(gi)
        if ent is None:
            return None
        return int(ent[0].view(torch.int32)[hyper_slots()["step"]].item())

    def _request_first(self, blk) -> None:
        blk[hyper_slots()["first_next"]] = 1.0

    def _step_block(self, gi: int, *, device=None, step: int = 0, fresh: bool = False):
        """Group ``gi``'s block, ready for the step about to be issued: created with step count
        ``step``, or brought up to date with the host's scalars; ``fresh`` (the momentum buffers
        were just created) makes that step the one that initialises them."""
        ent = self._blocks.get(gi)
        if ent is None:
            return self.hyper_block(gi, device=device, step=step, first=fresh)
        self.sync_hyper()
        if fresh:
            self._request_first(ent[0])
        return ent[0]

    # ------------------------------------------------------------------ torch API
    def zero_grad(self, set_to_none: bool = True) -> None:
        """torch's zero_grad, without its per-call record_function range / dynamo guard when
        gradients are simply dropped (the default) and the profiler is off."""
        if not set_to_none or torch.autograd.profiler._is_profiler_enabled:
            return super().zero_grad(set_to_none)
        for g in self.param_groups:
            for p in g["params"]:
                p.grad = None

    def _flat_state(self, arena, keys):
        """Arena-shaped state buffers; adopts values already in self.state (load_state_dict)."""
        bufs = self._flat_bufs.get(id(arena))
        if bufs is not None and all(k in bufs for k in keys):
            return bufs, False  # steady state: no per-parameter Python work
        fresh = False
        if bufs is None:
            bufs = {k: arena.new_state() for k in keys}
            self._flat_bufs[id(arena)] = bufs
            fresh = True
            arena.attach_optimizer(self)  # a DDP bucket rebuild re-lays the state out too
        for i, p in enumerate(arena.params):
            st = self.state[p]
            for k in keys:
                view = arena.state_view(bufs[k], i)
                cur = st.get(k)
                if cur is None:
                    st[k] = view
                elif cur.data_ptr() != view.data_ptr():
                    view.copy_(cur)
                    st[k] = view
                    fresh = False
        return bufs, fresh

    def _relayout(self, arena, remap) -> None:
        """The arena was re-laid out (DDP bucket rebuild): move the flat state buffers the same
        way and re-point the per-parameter state views."""
        bufs = self._flat_bufs.get(id(arena))
        if not bufs:
            return
        for k in list(bufs):
            bufs[k] = remap(bufs[k])
        for i, p in enumerate(arena.params):
            st = self.state[p]
            for k, buf in bufs.items():
                st[k] = arena.state_view(buf, i)

    def load_state_dict(self, state_dict):
        super().load_state_dict(state_dict)
        self._flat_bufs = {}  # re-adopted into flat buffers on the next step
        self._flat_step = {}
        self._blocks = {}     # re-created with the loaded step count
        ddp = getattr(self, "_fused_ddp", None)
        if ddp is not None:
            ddp.push_fused_hyper(self, initial=True)

    def _fused_step(self) -> bool:
        """When a DDP model applies this optimizer inside its reduction the update already
        happened during backward, so step() has nothing left to do (the DDP forward hands the
        current hyper-parameters, e.g. after an LR-scheduler step, to the fused update)."""
        return getattr(self, "_fused_ddp", None) is not None

    # ------------------------------------------------------------------ flat step counter
    # One count for the whole arena, held by the device block (graph replays advance it without
    # the host) and mirrored in _flat_step; state[p]["step"] is written when somebody looks.
    def _host_steps(self, arena) -> set:
        return {_step_of(self.state[p]) for p in arena.params}

    def _enter_flat(self, arena) -> bool:
        """Whether ``arena`` steps flat: it does already, or its parameters agree on a step
        count, which becomes the flat one. Mixed counts keep the group on MULTI."""
        if id(arena) in self._flat_step:
            return True
        steps = self._host_steps(arena)
        if len(steps) != 1:
            return False
        self._flat_step[id(arena)] = steps.pop()
        return True

    def _current_flat_step(self, arena) -> int:
        if id(arena) in self._flat_step:
            return self._flat_step[id(arena)]
        return max(self._host_steps(arena), default=0)

    def _store_flat_step(self, arena) -> None:
        t = torch.tensor(float(self._flat_step[id(arena)]))
        for p in arena.params:
            self.state[p]["step"] = t.clone()

    def _leave_flat(self, gi: int, g) -> None:
        """Group ``gi`` steps MULTI from here on: if it was flat, its count (the device's, when
        there is a block) goes back into state[p]["step"] and the block is dropped."""
        a = arena_of(g["params"])
        if a is None or id(a) not in self._flat_step:
            return
        dstep = self.device_step(gi)
        self._blocks.pop(gi, None)
        if dstep is not None:
            self._flat_step[id(a)] = dstep
        self._store_flat_step(a)
        del self._flat_step[id(a)]

    def state_dict(self):
        for gi, g in enumerate(self.param_groups):
            a = arena_of(g["params"])
            if a is None:
                continue
            dstep = self.device_step(gi) if self._kind == 2 else None
            if dstep is not None:
                self._flat_step[id(a)] = dstep
            if id(a) in self._flat_step:
                self._store_flat_step(a)
        return super().state_dict()

    # ------------------------------------------------------------------ MULTI bookkeeping
    def _momentum_split(self, ps, mom: bool):
        """``(parameters, first_step)``: those whose buffer this step creates, and the rest."""
        new, old = [], []
        for p in ps:
            st = self.state[p]
            if mom and st.get("momentum_buffer") is None:
                st["momentum_buffer"] = torch.empty_like(p)
                new.append(p)
            else:
                old.append(p)
        return (new, True), (old, False)

    def _bump_step(self, ps):
        steps = set()
        for p in ps:
            st = self.state[p]
            s = st.get("step")
            s = torch.tensor(0.0) if s is None else s
            s = s + 1 if torch.is_tensor(s) else torch.tensor(float(s) + 1)
            st["step"] = s
            steps.add(int(s.item()) if torch.is_tensor(s) else int(s))
        return steps

    def _by_step(self, ps, keys) -> dict:
        """Missing state of ``ps`` zero-filled, their step counts advanced: the new count ->
        the parameters at it (one launch each: the bias corrections go by value)."""
        for p in ps:
            st = self.state[p]
            for k in keys:
                if st.get(k) is None:
                    st[k] = torch.zeros_like(p)
        self._bump_step(ps)
        by_step = {}
        for p in ps:
            by_step.setdefault(_step_of(self.state[p]), []).append(p)
        return by_step


class SGD(_FusedBase):
    def __init__(self, params, lr: float = 1e-3, momentum: float = 0.0, dampening: float = 0.0,
                 weight_decay: float = 0.0, nesterov: bool = False, *, maximize: bool = False,
                 grad_scale: float = 1.0):
        if lr < 0 or momentum < 0 or weight_decay < 0:
            raise ValueError("invalid SGD hyper-parameter")
        if nesterov and (momentum <= 0 or dampening != 0):
            raise ValueError("Nesterov momentum requires a momentum and zero dampening")
        super().__init__(params, dict(lr=lr, momentum=momentum, dampening=dampening,
                                      weight_decay=weight_decay, nesterov=nesterov,
                                      maximize=maximize, grad_scale=grad_scale))

    _kind = 1

    def _scalars(self, g) -> tuple:
        return (float(g["lr"]), float(g["momentum"]), float(g["dampening"]),
                float(g["weight_decay"]), 0.0)

    @torch.no_grad()
    def step(self, closure=None):
        loss = None if closure is None else _closure_loss(closure)
        if self._fused_step():
            return loss
        tp = getattr(self, "_fused_tp", None)
        tp = tp() if tp is not None else None
        if tp is not None:
            # tensor-sharded wrapper with the shards' update in their GEMM epilogues: the rest
            tp._fused_step(self)
            return loss
        for gi, g in enumerate(self.param_groups):
            ps = [p for p in g["params"] if p.grad is not None]
            if not ps:
                continue
            if not ps[0].is_cuda:
                self._cpu_step(g, ps)
                continue
            C = native()
            hyper = (g["lr"], g["momentum"], g["dampening"], g["weight_decay"], g["nesterov"],
                     g["maximize"])
            mom = g["momentum"] != 0
            arena = _flat_arena(g, ps)
            if arena is not None:
                buf, fresh = None, False
                if mom:
                    # fresh == the buffers were just created (torch: buf = clone(grad))
                    bufs, fresh = self._flat_state(arena, ("momentum_buffer",))
                    buf = bufs["momentum_buffer"]
                # scalars and the first-step flag come from the device block (graph-safe)
                blk = self._step_block(gi, fresh=fresh)
                C.opt_step_begin(blk, 1)
                C.sgd_flat(arena.data, arena.grad, buf, *hyper, False, g["grad_scale"],
                           hyper=blk)
                continue
            for lst, first in self._momentum_split(ps, mom):
                if lst:
                    bufs = [self.state[p]["momentum_buffer"] for p in lst] if mom else []
                    C.sgd_multi([_dense(p.data) for p in lst], [_grad_like(p) for p in lst],
                                [_dense(b) for b in bufs], *hyper, first, g["grad_scale"])
        return loss

    def _cpu_step(self, g, ps):
        for p in ps:
            d = p.grad * g["grad_scale"]
            if g["maximize"]:
                d = -d
            if g["weight_decay"]:
                d = d.add(p, alpha=g["weight_decay"])
            if g["momentum"]:
                d = _momentum_cpu(self.state[p], d, g["momentum"], g["dampening"], g["nesterov"])
            p.add_(d, alpha=-g["lr"])


class Adam(_FusedBase):
    _decoupled = False

    def __init__(self, params, lr: float = 1e-3, betas=(0.9, 0.999), eps: float = 1e-8,
                 weight_decay: float = 0.0, amsgrad: bool = False, *, maximize: bool = False,
                 grad_scale: float = 1.0):
        if not 0.0 <= betas[0] < 1.0 or not 0.0 <= betas[1] < 1.0:
            raise ValueError(f"invalid betas {betas}")
        super().__init__(params, dict(lr=lr, betas=tuple(betas), eps=eps,
                                      weight_decay=weight_decay, amsgrad=amsgrad,
                                      maximize=maximize, grad_scale=grad_scale))

    _kind = 2

    def _scalars(self, g) -> tuple:
        return _adam_scalars(g)

    def _keys(self, g):
        return ("exp_avg", "exp_avg_sq") + (("max_exp_avg_sq",) if g["amsgrad"] else ())

    @torch.no_grad()
    def step(self, closure=None):
        loss = None if closure is None else _closure_loss(closure)
        if self._fused_step():
            return loss
        for gi, g in enumerate(self.param_groups):
            ps = [p for p in g["params"] if p.grad is not None]
            if not ps:
                continue
            if not ps[0].is_cuda:
                self._cpu_step(g, ps)
                continue
            C = native()
            b1, b2 = g["betas"]
            keys = self._keys(g)
            args = (g["lr"], b1, b2, g["eps"], g["weight_decay"], g["amsgrad"], g["maximize"],
                    self._decoupled)
            arena = _flat_arena(g, ps)
            if arena is not None and self._enter_flat(arena):
                bufs, _ = self._flat_state(arena, keys)
                # the step count and bias corrections advance ON THE DEVICE (opt_step_begin),
                # so a captured step replays correctly; the host count mirrors it eagerly
                blk = self._step_block(gi, step=self._flat_step[id(arena)])
                self._flat_step[id(arena)] += 1
                C.opt_step_begin(blk, 2)
                C.adam_flat(arena.data, arena.grad, bufs["exp_avg"], bufs["exp_avg_sq"],
                            bufs.get("max_exp_avg_sq"), *args, self._flat_step[id(arena)],
                            g["grad_scale"], hyper=blk)
                continue
            self._leave_flat(gi, g)
            for step, lst in self._by_step(ps, keys).items():
                st = [self.state[p] for p in lst]
                C.adam_multi([_dense(p.data) for p in lst], [_grad_like(p) for p in lst],
                             [_dense(s["exp_avg"]) for s in st], [_dense(s["exp_avg_sq"]) for s in st],
                             [_dense(s["max_exp_avg_sq"]) for s in st] if g["amsgrad"] else [],
                             *args, step, g["grad_scale"])
        return loss

    def _cpu_step(self, g, ps):
        b1, b2 = g["betas"]
        for p in ps:
            st = self.state[p]
            if st.get("exp_avg") is None:
                st["exp_avg"] = torch.zeros_like(p)
                st["exp_avg_sq"] = torch.zeros_like(p)
                if g["amsgrad"]:
                    st["max_exp_avg_sq"] = torch.zeros_like(p)
            self._bump_step([p])
            t = int(st["step"].item())
            grad = p.grad * g["grad_scale"]
            if g["maximize"]:
                grad = -grad
            if g["weight_decay"]:
                if self._decoupled:
                    p.mul_(1 - g["lr"] * g["weight_decay"])
                else:
                    grad = grad.add(p, alpha=g["weight_decay"])
            m, v = st["exp_avg"], st["exp_avg_sq"]
            m.lerp_(grad, 1 - b1)
            v.mul_(b2).addcmul_(grad, grad, value=1 - b2)
            bc1 = 1 - b1 ** t
            bc2s = (1 - b2 ** t) ** 0.5
            vv = v
            if g["amsgrad"]:
                torch.maximum(st["max_exp_avg_sq"], v, out=st["max_exp_avg_sq"])
                vv = st["max_exp_avg_sq"]
            denom = (vv.sqrt() / bc2s).add_(g["eps"])
            p.addcdiv_(m, denom, value=-g["lr"] / bc1)


def _f32(x) -> float:
    """A hyper-parameter as the kernels hold it: rounded to fp32, widened back to a double."""
    return float(torch.tensor(float(x), dtype=torch.float32))


class _LayerwiseBase(_FusedBase):
    """What LAMB and LARS share: each tensor's update is scaled by a trust ratio formed from
    whole-tensor L2 norms, so a GPU step is three launches over a device work table
    (csrc/optim_layerwise.hip): chunk partial sums, one finish per tensor, the update. FLAT runs
    them over the arena, MULTI over the individual tensors; both build the table with the same
    partition, so both give the same bits. The table is cached per layout; norms and ratios of
    the last step stay in a per-optimizer workspace (``trust_ratios``).

    Limits, on purpose: the norms are plain fp32 sums of squares, so a tensor whose sum of
    squares overflows gets a non-finite ratio and update, as the same formula would in torch --
    there is no clamp. The update cannot run inside DDP's gradient reduction
    (``DDP.register_fused_optimizer`` raises TypeError): sharded there, a rank sees 1/W of each
    tensor and the norms need all of it. Use ``loss.backward(); opt.step()``. ``skip_1d`` and
    LARS's ``trust_coefficient`` are passed by value: they are fixed once a step is captured."""

    def __init__(self, params, defaults):
        super().__init__(params, defaults)
        for g in self.param_groups:
            for p in g["params"]:
                if p.dtype != torch.float32:
                    raise TypeError(f"{type(self).__name__} takes fp32 parameters, got {p.dtype}")
        self._tables = {}    # layout key -> (work table, workspace)
        self._last_ws = {}   # group index -> (workspace [3, T], the T parameters in its order)
        self._flat_gi = {}   # id(arena) -> the group that steps it

    @staticmethod
    def _skip(g, p) -> bool:
        return bool(g["skip_1d"]) and p.dim() <= 1

    def trust_ratios(self, gi: int = 0):
        """``(ws, params)`` of group ``gi``'s last step: ``ws[0]`` = ||p||, ``ws[1]`` = ||u||
        (LARS: ||g'||), ``ws[2]`` = the trust ratio applied, one column per entry of ``params``.
        On the GPU this is the kernels' own workspace (reading it synchronises). When a step
        needed several launches (MULTI with mixed step counts) it is the last one's."""
        return self._last_ws.get(gi)

    def _table(self, gi, params, ps, gs, s0, s1, skip):
        key = (tuple(t.data_ptr() for t in ps), tuple(t.data_ptr() for t in gs),
               tuple(t.data_ptr() for t in s0), tuple(t.data_ptr() for t in s1),
               tuple(t.numel() for t in ps), tuple(skip))
        ent = self._tables.get(key)
        if ent is None:
            if len(self._tables) >= 8:  # MULTI: gradients move every step
                self._tables.clear()
            tab = native().layerwise_table(ps, gs, s0, s1, list(skip))
            ent = (tab, torch.zeros(3, len(ps), device=ps[0].device, dtype=torch.float32))
            self._tables[key] = ent
        self._last_ws[gi] = (ent[1], list(params))
        return ent

    def _flat_table(self, gi, g, arena, bufs):
        """The arena's table: rebuilt only when the layout (any base pointer) changes."""
        key = (id(arena), arena.data.data_ptr(), arena.grad.data_ptr(),
               tuple(b.data_ptr() for b in bufs), bool(g["skip_1d"]))
        ent = self._tables.get(key)
        if ent is None:
            self._tables.clear()
            sl = [slice(o, o + n) for o, n in zip(arena.offsets, arena.numels)]
            tab = native().layerwise_table(
                [arena.data[s] for s in sl], [arena.grad[s] for s in sl],
                [bufs[0][s] for s in sl] if len(bufs) > 0 else [],
                [bufs[1][s] for s in sl] if len(bufs) > 1 else [],
                [self._skip(g, p) for p in arena.params])
            ent = (tab, torch.zeros(3, len(sl), device=arena.data.device, dtype=torch.float32))
            self._tables[key] = ent
            self._flat_gi[id(arena)] = gi
            arena.attach_optimizer(self)  # a DDP bucket rebuild calls _relayout
        self._last_ws[gi] = (ent[1], list(arena.params))
        return ent

    def _relayout(self, arena, remap) -> None:
        super()._relayout(arena, remap)
        self._tables.clear()  # the chunk table holds the old arena's addresses
        gi = self._flat_gi.get(id(arena))
        if gi is not None:
            # rebuilt now, eagerly: the next step may be the one a hipGraph records, and
            # building the table copies from the host
            bufs = self._flat_bufs.get(id(arena), {})
            self._flat_table(gi, self.param_groups[gi], arena,
                             tuple(bufs[k] for k in self._state_keys if k in bufs))

    def load_state_dict(self, state_dict):
        super().load_state_dict(state_dict)
        self._tables.clear()
        self._last_ws = {}

    def _cpu_ws(self, gi, ps):
        ws = torch.zeros(3, len(ps), dtype=torch.float32)
        self._last_ws[gi] = (ws, list(ps))
        return ws


class LAMB(_LayerwiseBase):
    """LAMB (You et al., "Large Batch Optimization for Deep Learning", 2019): Adam with a trust
    ratio per tensor. With ``g' = grad_scale * g`` (negated if ``maximize``)::

        m <- m + (1 - beta1)(g' - m);  v <- beta2 v + (1 - beta2) g'^2
        u = (m / bc1) / (sqrt(v) / bc2_sqrt + eps) + wd * p
        r = ||p|| / ||u||  if both norms are positive, else 1
        p <- p - lr * r * u

    ``skip_1d``: a tensor with ``ndim <= 1`` (biases, norm scales) takes r = 1 and wd = 0; it is
    a per-tensor flag inside one group, so a whole model stays one flat step. The betas are held
    as fp32 and the bias corrections formed from those, on every path. State: ``exp_avg``,
    ``exp_avg_sq``, ``step``. See ``_LayerwiseBase`` for the limits."""
    _kind = 2
    _state_keys = ("exp_avg", "exp_avg_sq")

    def __init__(self, params, lr: float = 1e-3, betas=(0.9, 0.999), eps: float = 1e-6,
                 weight_decay: float = 0.01, *, skip_1d: bool = True, maximize: bool = False,
                 grad_scale: float = 1.0):
        if lr < 0 or eps < 0 or weight_decay < 0:
            raise ValueError("invalid LAMB hyper-parameter")
        if not 0.0 <= betas[0] < 1.0 or not 0.0 <= betas[1] < 1.0:
            raise ValueError(f"invalid betas {betas}")
        super().__init__(params, dict(lr=lr, betas=tuple(betas), eps=eps,
                                      weight_decay=weight_decay, skip_1d=skip_1d,
                                      maximize=maximize, grad_scale=grad_scale))

    def _scalars(self, g) -> tuple:
        return _adam_scalars(g)

    @torch.no_grad()
    def step(self, closure=None):
        loss = None if closure is None else _closure_loss(closure)
        for gi, g in enumerate(self.param_groups):
            ps = [p for p in g["params"] if p.grad is not None]
            if not ps:
                continue
            if not ps[0].is_cuda:
                self._cpu_step(gi, g, ps)
                continue
            C = native()
            b1, b2 = g["betas"]
            args = (g["lr"], b1, b2, g["eps"], g["weight_decay"], g["maximize"])
            arena = _flat_arena(g, ps)
            if arena is not None and self._enter_flat(arena):
                bufs, _ = self._flat_state(arena, self._state_keys)
                tab, ws = self._flat_table(gi, g, arena, (bufs["exp_avg"], bufs["exp_avg_sq"]))
                # step count and bias corrections advance on the device (graph-safe)
                blk = self._step_block(gi, step=self._flat_step[id(arena)])
                self._flat_step[id(arena)] += 1
                C.opt_step_begin(blk, 2)
                C.lamb_layerwise(tab, ws, *args, self._flat_step[id(arena)], g["grad_scale"],
                                 hyper=blk)
                continue
            self._leave_flat(gi, g)
            for step, lst in self._by_step(ps, self._state_keys).items():
                st = [self.state[p] for p in lst]
                tab, ws = self._table(
                    gi, lst, [_dense(p.data) for p in lst], [_grad_like(p) for p in lst],
                    [_dense(s["exp_avg"]) for s in st], [_dense(s["exp_avg_sq"]) for s in st],
                    [self._skip(g, p) for p in lst])
                C.lamb_layerwise(tab, ws, *args, step, g["grad_scale"])
        return loss

    def _cpu_step(self, gi, g, ps):
        """Plain torch code of the formulas; hyper-parameters rounded to fp32 as on the GPU."""
        lr, eps, wd = _f32(g["lr"]), _f32(g["eps"]), _f32(g["weight_decay"])
        b1, b2, gs = _f32(g["betas"][0]), _f32(g["betas"][1]), _f32(g["grad_scale"])
        ws = self._cpu_ws(gi, ps)
        one = torch.ones((), dtype=torch.float32)
        for i, p in enumerate(ps):
            st = self.state[p]
            if st.get("exp_avg") is None:
                st["exp_avg"] = torch.zeros_like(p)
                st["exp_avg_sq"] = torch.zeros_like(p)
            self._bump_step([p])
            t = int(st["step"].item())
            bc1, bc2s = _f32(1 - b1 ** t), _f32((1 - b2 ** t) ** 0.5)
            grad = p.grad * gs
            if g["maximize"]:
                grad = -grad
            m, v = st["exp_avg"], st["exp_avg_sq"]
            m.add_((grad - m) * (1 - b1))
            v.mul_(b2).add_(grad.mul(1 - b2).mul_(grad))
            u = (m / bc1) / (v.sqrt() / bc2s + eps)
            skip = self._skip(g, p)
            if wd and not skip:
                u = u.add(p, alpha=wd)
            norm_p, norm_u = p.norm(), u.norm()
            ratio = norm_p / norm_u if (not skip and norm_p > 0 and norm_u > 0) else one
            ws[0, i], ws[1, i], ws[2, i] = norm_p, norm_u, ratio
            p.addcmul_(u, ratio * torch.tensor(lr, dtype=torch.float32), value=-1.0)


class LARS(_LayerwiseBase):
    """LARS (You et al., "Large Batch Training of Convolutional Networks", 2017): SGD with a
    trust ratio per tensor. With ``g' = grad_scale * g`` (negated if ``maximize``)::

        q = trust_coefficient * ||p|| / (||g'|| + wd * ||p|| + eps)  if both norms are positive,
            else 1
        d = q * (g' + wd * p)

    then torch-SGD momentum, dampening and nesterov on ``d`` (the buffer is initialised to the
    first ``d``) and ``p <- p - lr * d``. ``skip_1d`` as for LAMB: q = 1 and wd = 0 for tensors
    with ``ndim <= 1``. State: ``momentum_buffer``. See ``_LayerwiseBase`` for the limits."""
    _kind = 1
    _state_keys = ("momentum_buffer",)

    def __init__(self, params, lr: float, momentum: float = 0.9, dampening: float = 0.0,
                 weight_decay: float = 0.0, nesterov: bool = False,
                 trust_coefficient: float = 1e-3, eps: float = 1e-8, *, skip_1d: bool = True,
                 maximize: bool = False, grad_scale: float = 1.0):
        if lr < 0 or momentum < 0 or weight_decay < 0 or eps < 0 or trust_coefficient <= 0:
            raise ValueError("invalid LARS hyper-parameter")
        if nesterov and (momentum <= 0 or dampening != 0):
            raise ValueError("Nesterov momentum requires a momentum and zero dampening")
        super().__init__(params, dict(lr=lr, momentum=momentum, dampening=dampening,
                                      weight_decay=weight_decay, nesterov=nesterov,
                                      trust_coefficient=trust_coefficient, eps=eps,
                                      skip_1d=skip_1d, maximize=maximize,
                                      grad_scale=grad_scale))

    def _scalars(self, g) -> tuple:
        return (float(g["lr"]), float(g["momentum"]), float(g["dampening"]),
                float(g["weight_decay"]), float(g["eps"]))  # eps takes the kHEps slot

    @torch.no_grad()
    def step(self, closure=None):
        loss = None if closure is None else _closure_loss(closure)
        for gi, g in enumerate(self.param_groups):
            ps = [p for p in g["params"] if p.grad is not None]
            if not ps:
                continue
            if not ps[0].is_cuda:
                self._cpu_step(gi, g, ps)
                continue
            C = native()
            mom = g["momentum"] != 0
            head = (g["lr"], g["momentum"], g["dampening"], g["weight_decay"], g["nesterov"],
                    g["maximize"])
            tail = (g["trust_coefficient"], g["eps"], g["grad_scale"])
            arena = _flat_arena(g, ps)
            if arena is not None:
                bufs, fresh = (), False
                if mom:
                    st, fresh = self._flat_state(arena, self._state_keys)
                    bufs = (st["momentum_buffer"],)
                tab, ws = self._flat_table(gi, g, arena, bufs)
                blk = self._step_block(gi, fresh=fresh)
                C.opt_step_begin(blk, 1)
                C.lars_layerwise(tab, ws, *head, False, *tail, hyper=blk)
                continue
            for lst, first in self._momentum_split(ps, mom):
                if lst:
                    tab, ws = self._table(
                        gi, lst, [_dense(p.data) for p in lst], [_grad_like(p) for p in lst],
                        [_dense(self.state[p]["momentum_buffer"]) for p in lst] if mom else [],
                        [], [self._skip(g, p) for p in lst])
                    C.lars_layerwise(tab, ws, *head, first, *tail)
        return loss

    def _cpu_step(self, gi, g, ps):
        """Plain torch code of the formulas; hyper-parameters rounded to fp32 as on the GPU."""
        lr, mom, damp = _f32(g["lr"]), _f32(g["momentum"]), _f32(g["dampening"])
        wd0, eps, gs = _f32(g["weight_decay"]), _f32(g["eps"]), _f32(g["grad_scale"])
        trust = torch.tensor(g["trust_coefficient"], dtype=torch.float32)
        ws = self._cpu_ws(gi, ps)
        one = torch.ones((), dtype=torch.float32)
        for i, p in enumerate(ps):
            d = p.grad * gs
            if g["maximize"]:
                d = -d
            skip = self._skip(g, p)
            wd = 0.0 if skip else wd0
            norm_p, norm_g = p.norm(), d.norm()
            q = one
            if not skip and norm_p > 0 and norm_g > 0:
                q = (trust * norm_p) / (norm_g + wd * norm_p + eps)
            ws[0, i], ws[1, i], ws[2, i] = norm_p, norm_g, q
            if wd:
                d = d.add(p, alpha=wd)
            d = d * q
            if mom:
                d = _momentum_cpu(self.state[p], d, mom, damp, g["nesterov"])
            p.add_(d, alpha=-lr)


class AdamW(Adam):
    _decoupled = True

    def __init__(self, params, lr: float = 1e-3, betas=(0.9, 0.999), eps: float = 1e-8,
                 weight_decay: float = 1e-2, amsgrad: bool = False, *, maximize: bool = False,
                 grad_scale: float = 1.0):
        super().__init__(params, lr, betas, eps, weight_decay, amsgrad, maximize=maximize,
                         grad_scale=grad_scale)
