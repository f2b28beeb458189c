"""Float64 oracle of the optimizer element update, with a derived per-element error bound.

A helper for tests/test_optim_oracle_cpu.py and tests/test_optim_gpu.py, not a test.

``sgd_step`` and ``adam_step`` are plain torch float64 code written from torch/optim/sgd.py
(``_single_tensor_sgd``) and torch/optim/adam.py (``_single_tensor_adam``): one optimizer step of
one tensor. They know nothing of csrc/optim_elem.h except the contract below.

Contract (what the oracle is given)
-----------------------------------
* p, g and the state are the fp32 tensors the kernel saw, widened to double.
* Every hyper-parameter is rounded to fp32 first and then widened (``f32``): the kernels hold them
  as ``float``. ``1 - beta``, ``1 - dampening`` and ``1 - lr*wd`` are formed in double from those.
* ``bc1 = 1 - beta1^t`` and ``bc2_sqrt = sqrt(1 - beta2^t)`` are INPUTS: the fp32 values the kernel
  used (computed by the binding from the by-value betas, or read back from the hyper block).
* ``grad_scale`` multiplies the gradient before anything else (the 1/world_size of a sum-reduced
  gradient, times the clip coefficient of the hyper block). torch has no such argument: it is
  handed ``g * grad_scale``.

Contract difference to torch, not an error: torch keeps betas as Python doubles and forms
``1 - 0.999`` in double; the kernels hold ``beta2 = 0.999f = 0.999000012874...`` and form
``1.f - beta2`` in fp32, which is EXACT (Sterbenz: 0.5 <= beta <= 1) and equals the double
``1 - f32(beta2)``. Against torch's double ``1 - 0.999`` it differs by -1.29e-5 relative; in general
by at most half an ulp of beta over ``1 - beta``, ``2^-25 * beta / (1 - beta)`` = 3.0e-5 for 0.999
(5.9e-5 when a full ulp ``2^-24`` is allowed for). An oracle that took the double betas would have
to carry that as slack; this one takes the kernel's own fp32 scalars and carries none.
A second one: adam_flat / adam_multi form the bias corrections in double from their by-value
DOUBLE betas (as torch does) while the element update runs on ``(float)beta``; opt_step_begin
forms them from the hyper block's fp32 betas. The two are 1.3e-5 relative apart in
``1 - 0.999^t`` -- 3x to 8x this module's bound on p -- so ``bias_corrections`` takes
``fp32_betas`` and the tests pass what the path under test really used.

Error bound
-----------
``u = 2^-24`` is the unit roundoff of fp32 (round to nearest). Every fp32 operation of the kernel
returns ``x(1 + d)``, ``|d| <= u``, of the exact result x of its (already perturbed) inputs; an fma
rounds once. First-order propagation: each rounding adds ``u * |x|`` with x the float64 magnitude
of the value rounded there, and errors already carried by the inputs pass through multiplied by
the magnitude of the partial derivative. The roundings of optim_elem.h, in program order
(``[n]`` numbers them; a term in brackets only exists with that flag):

sgd_elem
  [1] g1 = g * grad_scale                      e(g1)  = u|g1|               (negation is exact)
  [2] g2 = fma(wd, p, g1)           [wd != 0]  e(g2)  = e(g1) + u|g2|
  first step: buf = g2                         e(buf) = e(g2)
  else [3] c = 1 - dampening                   e(c)   = u|c|
       [4] t = c * g2                          e(t)   = |g2| e(c) + |c| e(g2) + u|t|
       [5] buf = fma(buf0, momentum, t)        e(buf) = e(t) + u|buf|
  [6] g3 = fma(momentum, buf, g2)  [nesterov]  e(g3)  = momentum e(buf) + e(g2) + u|g3|
      g3 = buf                   [otherwise]   e(g3)  = e(buf)
  [7] p = fma(-lr, g3, p0)                     e(p)   = lr e(g3) + u|p|
  At most 7 roundings lie on the path to p and 5 on the path to buf.

adam_elem
  [1] g1 = g * grad_scale                      e(g1)  = u|g1|
  decoupled: [2] x = lr * wd, [3] c = 1 - x    e(c)   = u(|x| + |c|)
             [4] p1 = p0 * c                   e(p1)  = |p0| e(c) + u|p1|
  L2:        [2] g2 = fma(wd, p0, g1)          e(g2)  = e(g1) + u|g2|
  [5] a = 1 - beta1                            e(a)   = u|a|
  [6] d = g2 - m0                              e(d)   = e(g2) + u|d|
  [7] m = fma(a, d, m0)                        e(m)   = |d| e(a) + |a| e(d) + u|m|
  [8] b = 1 - beta2                            e(b)   = u|b|
  [9] t1 = b * g2                              e(t1)  = |g2| e(b) + |b| e(g2) + u|t1|
  [10] t2 = t1 * g2                            e(t2)  = |g2| e(t1) + |t1| e(g2) + u|t2|
  [11] v = fma(v0, beta2, t2)                  e(v)   = e(t2) + u|v|
  amsgrad: vv = vmax = max(vmax0, v)           e(vv)  = e(v)       (max is 1-Lipschitz, exact)
  [12] s = sqrt(vv)                            e(s)   = e(vv) / (2 s) + u|s|
  [13] q = s / bc2_sqrt                        e(q)   = e(s) / bc2_sqrt + u|q|
  [14] den = q + eps                           e(den) = e(q) + u|den|
  [15] r = m / den                             e(r)   = e(m)/den + |m| e(den)/den^2 + u|r|
  [16] ss = lr / bc1                           e(ss)  = u|ss|
  [17] p = fma(-ss, r, p1)                     e(p)   = e(p1) + |r| e(ss) + ss e(r) + u|p|
  At most 17 roundings lie on the path to p, 5 to m, 6 to v and vmax.

The bound returned for every output is TWICE the propagated e(.): ``sqrtf`` and ``/`` are not
guaranteed correctly rounded on the device (each may cost 2u instead of u), the compiler may
contract ``1 - lr*wd`` into one fma (fewer roundings, never more), and the second-order terms
dropped above are ``O(u)`` relative to the bound. Every rounding also adds ``2^-126`` (a subnormal
result flushed to zero), so the bound of an exactly-zero result is not zero. No number here was
tuned against kernel output.

Every comparison is ONE step from the kernel's own fp32 state (snapshot, run the kernel, run the
oracle on the snapshot, compare), so errors never compound and the bound stays this tight.
"""
from __future__ import annotations

import numpy as np
import torch

U = 2.0 ** -24       # fp32 unit roundoff
TINY = 2.0 ** -126   # smallest normal fp32: one flushed subnormal per rounding
SLACK = 2.0          # see "Error bound" above


def f32(x) -> float:
    """A hyper-parameter as the kernel holds it: rounded to fp32, widened to double."""
    return float(np.float32(x))


def _rnd(x: torch.Tensor) -> torch.Tensor:
    """The error one fp32 rounding adds to a result of float64 magnitude |x|."""
    return U * x.abs() + TINY


def sgd_hyper(lr=0.05, momentum=0.0, dampening=0.0, weight_decay=0.0, nesterov=False,
              maximize=False, grad_scale=1.0) -> dict:
    return dict(lr=lr, momentum=momentum, dampening=dampening, weight_decay=weight_decay,
                nesterov=nesterov, maximize=maximize, grad_scale=grad_scale)


def adam_hyper(lr=0.01, beta1=0.9, beta2=0.999, eps=1e-3, weight_decay=0.0, amsgrad=False,
               maximize=False, decoupled=False, grad_scale=1.0) -> dict:
    return dict(lr=lr, beta1=beta1, beta2=beta2, eps=eps, weight_decay=weight_decay,
                amsgrad=amsgrad, maximize=maximize, decoupled=decoupled, grad_scale=grad_scale)


def bias_corrections(beta1, beta2, t: int, fp32_betas: bool):
    """(bc1, bc2_sqrt) in double; the caller rounds them to fp32 (``f32``) when the kernel did.

    ``fp32_betas=True``: from the betas rounded to fp32 -- what opt_step_begin computes from the
    hyper block (and what torch computes when it is handed those betas).
    ``fp32_betas=False``: from the betas as given -- what adam_flat / adam_multi compute from
    their by-value double arguments, like torch, while the element update runs on the fp32 betas.
    The two differ by 1.3e-5 relative in ``1 - 0.999^t``; that is why they are inputs."""
    b1, b2 = (f32(beta1), f32(beta2)) if fp32_betas else (float(beta1), float(beta2))
    return 1.0 - b1 ** t, float(np.sqrt(1.0 - b2 ** t))


def sgd_step(p, g, buf, hyper: dict, first_step: bool, _mutant: str | None = None):
    """One torch.optim.SGD step of one tensor in float64.

    ``buf`` is the momentum buffer before the step (ignored when ``first_step`` or without
    momentum). Returns ``(out, bound)``, dicts over "p" and (with momentum) "buf".
    ``_mutant`` is for the mutant-rejection test only."""
    p0, g = p.double(), g.double()
    lr, mom, damp, wd = (f32(hyper[k]) for k in ("lr", "momentum", "dampening", "weight_decay"))
    gs = f32(hyper["grad_scale"])
    maximize = hyper["maximize"] and _mutant != "maximize_ignored"
    if _mutant == "dampening_ignored":
        damp = 0.0
    if _mutant == "grad_scale_after_wd":
        gs_late, gs = gs, 1.0
    grad = g * gs
    e_g = _rnd(grad)
    if maximize:
        grad = -grad
    if wd != 0.0:
        grad = grad + wd * p0
        e_g = e_g + _rnd(grad)
    if _mutant == "grad_scale_after_wd":
        grad = grad * gs_late
    out, bound = {}, {}
    if mom != 0.0:
        if first_step and _mutant != "buf_not_initialised":
            b, e_b = grad.clone(), e_g
        else:
            b0 = torch.zeros_like(grad) if first_step else buf.double()
            c = 1.0 - damp
            t = c * grad
            e_t = grad.abs() * _rnd(torch.tensor(c)) + abs(c) * e_g + _rnd(t)
            b = b0 * mom + t
            e_b = e_t + _rnd(b)
        if hyper["nesterov"] and _mutant != "nesterov_dropped":
            grad2 = grad + mom * b
            e_g = mom * e_b + e_g + _rnd(grad2)
            grad = grad2
        else:
            grad, e_g = b, e_b
        out["buf"], bound["buf"] = b, SLACK * e_b
    pn = p0 - lr * grad
    out["p"], bound["p"] = pn, SLACK * (lr * e_g + _rnd(pn))
    return out, bound


def adam_step(p, g, m, v, vmax, hyper: dict, bc1: float, bc2_sqrt: float,
              _mutant: str | None = None):
    """One torch.optim.Adam / AdamW (``decoupled``) step of one tensor in float64.

    ``bc1`` / ``bc2_sqrt`` are the bias corrections the kernel used. Returns ``(out, bound)``,
    dicts over "p", "m", "v" and (amsgrad) "vmax"."""
    p0, g, m0, v0 = p.double(), g.double(), m.double(), v.double()
    lr, b1, b2, eps, wd = (f32(hyper[k]) for k in ("lr", "beta1", "beta2", "eps", "weight_decay"))
    gs = f32(hyper["grad_scale"])
    maximize = hyper["maximize"] and _mutant != "maximize_ignored"
    decoupled = hyper["decoupled"] != (_mutant == "decay_swapped")
    if _mutant == "bc1_not_applied":
        bc1 = 1.0
    if _mutant == "bc2_not_applied":
        bc2_sqrt = 1.0
    if _mutant == "grad_scale_after_wd":
        gs_late, gs = gs, 1.0
    grad = g * gs
    e_g = _rnd(grad)
    if maximize:
        grad = -grad
    p1, e_p1 = p0, torch.zeros_like(p0)
    if wd != 0.0:
        if decoupled:
            x = lr * wd
            c = 1.0 - x
            p1 = p0 * c
            e_p1 = p0.abs() * (U * (abs(x) + abs(c)) + 2 * TINY) + _rnd(p1)
        else:
            grad = grad + wd * p0
            e_g = e_g + _rnd(grad)
    if _mutant == "grad_scale_after_wd":
        grad = grad * gs_late
    a = 1.0 - b1
    d = grad - m0
    e_d = e_g + _rnd(d)
    mn = m0 + a * d  # lerp(m0, grad, 1 - beta1)
    e_m = d.abs() * _rnd(torch.tensor(a)) + abs(a) * e_d + _rnd(mn)
    b = 1.0 - b2
    t1 = b * grad
    e_t1 = grad.abs() * _rnd(torch.tensor(b)) + abs(b) * e_g + _rnd(t1)
    t2 = t1 * grad
    e_t2 = grad.abs() * e_t1 + t1.abs() * e_g + _rnd(t2)
    vn = v0 * b2 + t2
    e_v = e_t2 + _rnd(vn)
    out = {"m": mn, "v": vn}
    bound = {"m": SLACK * e_m, "v": SLACK * e_v}
    vv = vn
    if hyper["amsgrad"]:
        vx = torch.maximum(vmax.double(), vn)
        out["vmax"], bound["vmax"] = vx, SLACK * e_v
        if _mutant != "amsgrad_uses_v":
            vv = vx
    if _mutant == "eps_inside_sqrt":
        den = (vv + eps).sqrt() / bc2_sqrt
        e_den = torch.zeros_like(den)
    else:
        s = vv.sqrt()
        e_s = torch.where(s > 0, e_v / (2 * s).clamp_min(TINY), e_v.sqrt()) + _rnd(s)
        q = s / bc2_sqrt
        e_q = e_s / abs(bc2_sqrt) + _rnd(q)
        den = q + eps
        e_den = e_q + _rnd(den)
    r = mn / den
    e_r = e_m / den + mn.abs() * e_den / (den * den) + _rnd(r)
    ss = lr / bc1
    pn = p1 - ss * r
    e_p = e_p1 + r.abs() * _rnd(torch.tensor(ss)) + abs(ss) * e_r + _rnd(pn)
    out["p"], bound["p"] = pn, SLACK * e_p
    return out, bound


def error_ratio(actual: torch.Tensor, expect: torch.Tensor, bound: torch.Tensor) -> float:
    """max |actual - expect| / bound over the tensor (NaN / inf in ``actual`` give inf)."""
    if actual.numel() == 0:
        return 0.0
    err = (actual.detach().double().cpu().reshape(-1) - expect.cpu().reshape(-1)).abs()
    ratio = err / bound.cpu().reshape(-1)
    ratio = torch.where(torch.isfinite(ratio), ratio, torch.full_like(ratio, float("inf")))
    return float(ratio.max())


# ------------------------------------------------------------------ shared inputs of both tests
# weight_decay ~ 0.1, dampening 0.25, grad_scale 0.25, eps 1e-3 with |g| in [1e-3, 1] and Adam
# step t >= 2 make every mutant of test_optim_oracle_cpu.py visible; the "maximize" sets carry a
# weight decay too so that the order of grad_scale and weight decay shows.
WD, DAMP, GSCALE, EPS = 0.1, 0.25, 0.25, 1e-3
SGD_FLAGS = {
    "plain": sgd_hyper(),
    "momentum": sgd_hyper(momentum=0.9),
    "momentum_dampening": sgd_hyper(momentum=0.9, dampening=DAMP),
    "nesterov_wd": sgd_hyper(momentum=0.9, nesterov=True, weight_decay=WD),
    "maximize_gscale": sgd_hyper(momentum=0.9, weight_decay=WD, maximize=True,
                                 grad_scale=GSCALE),
}
ADAM_FLAGS = {
    "plain": adam_hyper(eps=EPS),
    "l2": adam_hyper(eps=EPS, weight_decay=WD),
    "decoupled": adam_hyper(eps=EPS, weight_decay=WD, decoupled=True),
    "amsgrad": adam_hyper(eps=EPS, amsgrad=True),
    "amsgrad_maximize_gscale": adam_hyper(eps=EPS, weight_decay=WD, amsgrad=True, maximize=True,
                                          grad_scale=GSCALE),
}
# The GEMM optimizer epilogue takes every scalar from the hyper block (no grad_scale by value).
EPI_SGD_FLAGS = {
    "no_momentum_wd": sgd_hyper(weight_decay=WD),
    "momentum_dampening_wd": sgd_hyper(momentum=0.9, dampening=DAMP, weight_decay=WD),
    "nesterov_wd_maximize": sgd_hyper(momentum=0.9, nesterov=True, weight_decay=WD,
                                      maximize=True),
}
EPI_ADAM_FLAGS = {k: ADAM_FLAGS[k] for k in ("plain", "l2", "decoupled", "amsgrad")}
# The hyper-block tests: grad_scale is blk[scale] = 0.5 times the by-value 0.5.
HB_SGD = sgd_hyper(momentum=0.9, dampening=DAMP, weight_decay=WD, maximize=True,
                   grad_scale=GSCALE)
HB_ADAM = adam_hyper(eps=EPS, weight_decay=WD, amsgrad=True, maximize=True, grad_scale=GSCALE)
# Every flag set a GPU test uses, under one name each: what the CPU tests compare with torch.
ALL_SGD_FLAGS = {**SGD_FLAGS, **{"epi_" + k: h for k, h in EPI_SGD_FLAGS.items()},
                 "hyper_block": HB_SGD}
ALL_ADAM_FLAGS = {**ADAM_FLAGS, "hyper_block": HB_ADAM}  # EPI_ADAM_FLAGS is a subset
# Seeds of make_state / make_grad / make_operands that the GPU tests and the mutant test share.
HB_SGD_SEED, HB_ADAM_SEED = 40, 50
EPI_SGD_STATE_SEED, EPI_SGD_SEED = 60, 100
STEPS = 3
ADAM_T0 = 2 # the first Adam step of every test is t = 2 (seeded state): bc1, bc2 != trivial


def make_operands(M: int, N: int, K: int, seed: int):
    """A [K][M] and B [K][N] of the GEMM epilogue tests: integers in [-15, 15] times 2^-3. Every
    product is a multiple of 2^-6 below 4 and every partial sum below 2^9 (K <= 128), so A^T B is
    exact in fp32 in any summation order, and under the split-bf16 emulation too (4 significant
    bits per operand): the only rounding left is the element update."""
    gen = torch.Generator().manual_seed(seed)
    A = torch.randint(-15, 16, (K, M), generator=gen).float() / 8
    B = torch.randint(-15, 16, (K, N), generator=gen).float() / 8
    return A, B


def _log_uniform(n, gen):
    """sign * 10^(-3 U): magnitudes from 1e-3 to 1."""
    mag = torch.pow(10.0, -3.0 * torch.rand(n, generator=gen))
    sign = torch.where(torch.rand(n, generator=gen) < 0.5, -1.0, 1.0)
    return (mag * sign).float()


def make_grad(n: int, seed: int, step: int) -> torch.Tensor:
    gen = torch.Generator().manual_seed(1000 * seed + step)
    return _log_uniform(n, gen)


def make_state(n: int, seed: int) -> dict:
    """fp32 CPU tensors: p, a momentum buffer / exp_avg, exp_avg_sq = g0^2 of another gradient
    draw, and a max_exp_avg_sq at twice or half of it (a coin per element), which puts it above
    the next exp_avg_sq on about half of the elements and below on the rest."""
    gen = torch.Generator().manual_seed(seed)
    p = torch.randn(n, generator=gen)
    m = 0.1 * torch.randn(n, generator=gen)
    v = _log_uniform(n, gen) ** 2
    coin = torch.rand(n, generator=gen) < 0.5
    vmax = v * torch.where(coin, 2.0, 0.5)
    return {"p": p.float(), "m": m.float(), "v": v.float(), "vmax": vmax.float()}
