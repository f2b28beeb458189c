"""Float64 oracle of LAMB and LARS (one tensor, one step) with derived error bounds.

A helper for tests/test_layerwise_optim_cpu.py and tests/test_layerwise_optim_gpu.py, not a test.
torch has neither optimizer; ``lamb_step`` and ``lars_step`` are written from the formulas in the
class docstrings of ``tdp.optim.LAMB`` / ``LARS``. They follow the contract of
tests/optim_oracle.py (read that first): tensors are the fp32 values the kernel saw, widened;
every hyper-parameter is rounded to fp32 first; ``bc1`` / ``bc2_sqrt`` are INPUTS (the fp32 values
the kernel used) -- and so is the per-tensor trust ``ratio``, read back from the optimizer's
workspace. The ratio gets its own check (``lamb_ratio`` / ``lars_ratio``) against float64 norms.

Element bounds
--------------
As in optim_oracle.py: ``u = 2^-24``, every fp32 operation returns ``x(1 + d)``, ``|d| <= u``,
first-order propagation, TWICE the propagated value returned (sqrt and / may cost 2u on the
device, contraction removes roundings but never adds any, second-order terms), ``2^-126`` per
rounding for a flushed subnormal. The roundings of csrc/optim_elem.h in program order:

lamb_update_elem / lamb_u   (``wd`` is 0 for a skipped tensor)
  [1]  g1 = g * grad_scale                     e(g1)  = u|g1|            (negation is exact)
  [2]  a = 1 - beta1                           e(a)   = u|a|
  [3]  d = g1 - m0                             e(d)   = e(g1) + u|d|
  [4]  m = fma(a, d, m0)                       e(m)   = |d| e(a) + |a| e(d) + u|m|
  [5]  b = 1 - beta2                           e(b)   = u|b|
  [6]  t1 = b * g1                             e(t1)  = |g1| e(b) + |b| e(g1) + u|t1|
  [7]  t2 = t1 * g1                            e(t2)  = |g1| e(t1) + |t1| e(g1) + u|t2|
  [8]  v = fma(v0, beta2, t2)                  e(v)   = e(t2) + u|v|
  [9]  s = sqrt(v)                             e(s)   = e(v) / (2 s) + u|s|
  [10] q = s / bc2_sqrt                        e(q)   = e(s) / bc2_sqrt + u|q|
  [11] den = q + eps                           e(den) = e(q) + u|den|
  [12] mh = m / bc1                            e(mh)  = e(m) / bc1 + u|mh|
  [13] r = mh / den                            e(r)   = e(mh)/den + |mh| e(den)/den^2 + u|r|
  [14] uu = fma(wd, p0, r)        [wd != 0]    e(uu)  = e(r) + u|uu|
  stage 2 (the ratio is an input, exact):
  [15] c = lr * ratio                          e(c)   = u|c|
  [16] p = fma(-c, uu, p0)                     e(p)   = |uu| e(c) + |c| e(uu) + u|p|
  16 roundings at most on the path to p, 4 to m, 5 to v.

lars_grad / lars_elem   (``wd`` is 0 for a skipped tensor; the ratio is an input, exact)
  [1] g1 = g * grad_scale                      e(g1)  = u|g1|
  [2] g2 = fma(wd, p0, g1)        [wd != 0]    e(g2)  = e(g1) + u|g2|
  [3] d = g2 * ratio                           e(d)   = |ratio| e(g2) + u|d|
  first step: buf = d                          e(buf) = e(d)
  else [4] c = 1 - dampening                   e(c)   = u|c|
       [5] t = c * d                           e(t)   = |d| e(c) + |c| e(d) + u|t|
       [6] buf = fma(buf0, momentum, t)        e(buf) = e(t) + u|buf|
  [7] d2 = fma(momentum, buf, d)  [nesterov]   e(d2)  = momentum e(buf) + e(d) + u|d2|
      d2 = buf                  [otherwise]    e(d2)  = e(buf)
  [8] p = fma(-lr, d2, p0)                     e(p)   = lr e(d2) + u|p|

Norm bound
----------
The kernels' summation shape (csrc/optim_layerwise.hip) for a tensor of n elements cut into
K = ceil(n / C) chunks: inside a chunk of c elements each lane adds its own squares serially with
one fma each -- L = 4 ceil(c / 1024) of them when the workgroup takes the chunk (c > SMALL), or
4 ceil(c / 256) when one wave does -- then a 6-level butterfly adds the 64 lanes, and (workgroup
form) 3 more additions join the four waves. The finish adds the K chunk partials: each lane
ceil(K / 64) of them serially, then another 6-level butterfly. A square therefore passes through
at most

    D = L + 6 + 3 + ceil(K / 64) + 6

roundings (its own fma's included), and all terms are non-negative, so to first order
``|S^ - S| <= D u S``. Terms that carry an error e_i of their own (LAMB's u, LARS's g') add
``2 sum |x_i| e_i <= 2 ||x|| ||e||``. With the square root's own rounding,

    e(norm) = (D / 2) u norm + ||e||_2 + u norm,

and TWICE that is the bound (``norm_bound``), as for the elements. ``depth`` is an argument: the
CPU path sums with torch, whose order is not specified, so its tests pass the worst case n.

Ratio bounds, from the finish kernel's roundings with the norms' own errors as inputs:
  LAMB  r = np / nu                            e(r) = e(np)/nu + np e(nu)/nu^2 + u|r|
  LARS  [1] a = fma(wd, np, ng)                e(a) = wd e(np) + e(ng) + u|a|
        [2] den = a + eps                      e(den) = e(a) + u|den|
        [3] num = trust * np                   e(num) = trust e(np) + u|num|
        [4] q = num / den                      e(q) = e(num)/den + num e(den)/den^2 + u|q|
(e(np), e(nu) enter unslacked and the result is doubled once.) A norm that is exactly zero in
float64 must give the ratio exactly 1: a sum of squares of zeros is zero in any order.

No number here was tuned against kernel output.
"""
from __future__ import annotations

import math

import torch

from optim_oracle import SLACK, TINY, U, _rnd, error_ratio, f32  # noqa: F401  (re-exported)


def lamb_hyper(lr=0.01, beta1=0.9, beta2=0.999, eps=1e-3, weight_decay=0.1, maximize=False,
               grad_scale=1.0) -> dict:
    return dict(lr=lr, beta1=beta1, beta2=beta2, eps=eps, weight_decay=weight_decay,
                maximize=maximize, grad_scale=grad_scale)


def lars_hyper(lr=0.05, momentum=0.9, dampening=0.0, weight_decay=0.0, nesterov=False,
               trust_coefficient=1e-3, eps=1e-8, maximize=False, grad_scale=1.0) -> dict:
    return dict(lr=lr, momentum=momentum, dampening=dampening, weight_decay=weight_decay,
                nesterov=nesterov, trust_coefficient=trust_coefficient, eps=eps,
                maximize=maximize, grad_scale=grad_scale)


def lamb_step(p, g, m, v, hyper: dict, bc1: float, bc2_sqrt: float, ratio: float,
              skip: bool = False, e_in: dict | None = None):
    """One LAMB step of one tensor in float64, given the trust ratio the kernel applied.
    Returns ``(out, bound)`` over "p", "m", "v" and "u" (the direction whose norm the kernel
    reduces; its "bound" entry is the UNSLACKED e(u), an input of ``norm_bound``).
    ``e_in`` (multi-step twins): UNSLACKED errors the kernel's p, m, v already carry against
    the float64 inputs given here; they start the propagation instead of zero."""
    p0, g, m0, v0 = p.double(), g.double(), m.double(), v.double()
    lr, b1, b2, eps = (f32(hyper[k]) for k in ("lr", "beta1", "beta2", "eps"))
    wd = 0.0 if skip else f32(hyper["weight_decay"])
    grad = g * f32(hyper["grad_scale"])
    e_g = _rnd(grad)
    if hyper["maximize"]:
        grad = -grad
    zero = torch.zeros_like(p0)
    e_p0, e_m0, e_v0 = ((e_in or {}).get(k, zero) for k in ("p", "m", "v"))
    a = 1.0 - b1
    d = grad - m0
    e_d = e_g + e_m0 + _rnd(d)
    mn = m0 + a * d
    e_m = e_m0 + d.abs() * _rnd(torch.tensor(a)) + abs(a) * e_d + _rnd(mn)
    b = 1.0 - b2
    t1 = b * grad
    e_t1 = grad.abs() * _rnd(torch.tensor(b)) + abs(b) * e_g + _rnd(t1)
    t2 = t1 * grad
    e_t2 = grad.abs() * e_t1 + t1.abs() * e_g + _rnd(t2)
    vn = v0 * b2 + t2
    e_v = b2 * e_v0 + e_t2 + _rnd(vn)
    s = vn.sqrt()
    e_s = torch.where(s > 0, e_v / (2 * s).clamp_min(TINY), e_v.sqrt()) + _rnd(s)
    q = s / bc2_sqrt
    e_q = e_s / abs(bc2_sqrt) + _rnd(q)
    den = q + eps
    e_den = e_q + _rnd(den)
    mh = mn / bc1
    e_mh = e_m / abs(bc1) + _rnd(mh)
    r = mh / den
    e_r = e_mh / den + mh.abs() * e_den / (den * den) + _rnd(r)
    uu, e_u = r, e_r
    if wd != 0.0:
        uu = r + wd * p0
        e_u = e_r + wd * e_p0 + _rnd(uu)
    c = lr * float(ratio)
    pn = p0 - c * uu
    e_p = e_p0 + uu.abs() * _rnd(torch.tensor(c)) + abs(c) * e_u + _rnd(pn)
    out = {"p": pn, "m": mn, "v": vn, "u": uu}
    bound = {"p": SLACK * e_p, "m": SLACK * e_m, "v": SLACK * e_v, "u": e_u}
    return out, bound


def lars_step(p, g, buf, hyper: dict, ratio: float, first_step: bool, skip: bool = False,
              e_in: dict | None = None):
    """One LARS step of one tensor in float64, given the trust ratio the kernel applied.
    Returns ``(out, bound)`` over "p", "buf" (with momentum) and "gp" (g', whose norm the
    kernel reduces; its "bound" entry is the UNSLACKED e(g')). ``e_in`` as for ``lamb_step``
    (keys "p", "buf")."""
    p0, g = p.double(), g.double()
    lr, mom, damp = (f32(hyper[k]) for k in ("lr", "momentum", "dampening"))
    wd = 0.0 if skip else f32(hyper["weight_decay"])
    q = float(ratio)
    grad = g * f32(hyper["grad_scale"])
    e_g = _rnd(grad)
    if hyper["maximize"]:
        grad = -grad
    out, bound = {"gp": grad}, {"gp": e_g}
    zero = torch.zeros_like(p0)
    e_p0, e_b0 = ((e_in or {}).get(k, zero) for k in ("p", "buf"))
    if wd != 0.0:
        grad = grad + wd * p0
        e_g = e_g + wd * e_p0 + _rnd(grad)
    d = grad * q
    e_d = abs(q) * e_g + _rnd(d)
    if mom != 0.0:
        if first_step:
            b, e_b = d.clone(), e_d
        else:
            c = 1.0 - damp
            t = c * d
            e_t = d.abs() * _rnd(torch.tensor(c)) + abs(c) * e_d + _rnd(t)
            b = buf.double() * mom + t
            e_b = mom * e_b0 + e_t + _rnd(b)
        if hyper["nesterov"]:
            d2 = d + mom * b
            e_d = mom * e_b + e_d + _rnd(d2)
            d = d2
        else:
            d, e_d = b, e_b
        out["buf"], bound["buf"] = b, SLACK * e_b
    pn = p0 - lr * d
    out["p"], bound["p"] = pn, SLACK * (e_p0 + lr * e_d + _rnd(pn))
    return out, bound


# ---------------------------------------------------------------------------- norms and ratios
def kernel_depth(n: int, chunk: int, small: int) -> int:
    """D of the docstring for a tensor of n elements (the longest chunk decides L)."""
    if n <= 0:
        return 0
    K = -(-n // chunk)
    c = min(n, chunk)  # the longest chunk of the tensor
    L = 4 * (-(-c // 1024)) if c > small else 4 * (-(-c // 256))
    return L + 6 + 3 + -(-K // 64) + 6


def norm_e(x64: torch.Tensor, depth: int, e_elems=None):
    """``(norm, e(norm))`` in float64: the UNSLACKED propagated error of the docstring."""
    x64 = x64.double().reshape(-1)
    norm = float(torch.linalg.vector_norm(x64))
    e_in = 0.0 if e_elems is None else float(torch.linalg.vector_norm(e_elems.double()))
    return norm, (depth / 2.0) * U * norm + e_in + U * norm + TINY


def norm_bound(x64: torch.Tensor, depth: int, e_elems=None):
    norm, e = norm_e(x64, depth, e_elems)
    return norm, SLACK * e


def lamb_ratio(np_, e_np, nu, e_nu, skip: bool = False):
    """``(ratio, bound)``; bound 0 where the ratio must be exactly 1."""
    if skip or not (np_ > 0 and nu > 0):
        return 1.0, 0.0
    r = np_ / nu
    return r, SLACK * (e_np / nu + np_ * e_nu / (nu * nu) + U * abs(r) + TINY)


def lars_ratio(np_, e_np, ng, e_ng, hyper: dict, skip: bool = False):
    if skip or not (np_ > 0 and ng > 0):
        return 1.0, 0.0
    wd, eps, trust = (f32(hyper[k]) for k in ("weight_decay", "eps", "trust_coefficient"))
    a = wd * np_ + ng
    e_a = wd * e_np + e_ng + U * abs(a) + TINY
    den = a + eps
    e_den = e_a + U * abs(den) + TINY
    num = trust * np_
    e_num = trust * e_np + U * abs(num) + TINY
    q = num / den
    return q, SLACK * (e_num / den + num * e_den / (den * den) + U * abs(q) + TINY)


def scalar_ratio(actual: float, expect: float, bound: float) -> float:
    """|actual - expect| / bound for one number; an exact expectation (bound 0) gives 0 or inf."""
    err = abs(float(actual) - float(expect))
    if not math.isfinite(err):
        return float("inf")
    if bound == 0.0:
        return 0.0 if err == 0.0 else float("inf")
    return err / bound


def bias_corrections(beta1, beta2, t: int):
    """(bc1, bc2_sqrt) as every LAMB path forms them: in double from the fp32 betas, then
    rounded to fp32 (opt_step_begin; the by-value binding; the CPU path)."""
    b1, b2 = f32(beta1), f32(beta2)
    return f32(1.0 - b1 ** t), f32(math.sqrt(1.0 - b2 ** t))
