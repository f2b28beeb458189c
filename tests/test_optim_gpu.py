"""The optimizer element update (csrc/optim_elem.h) in every kernel that carries it, against the
float64 oracle of tests/optim_oracle.py and its derived error bound.

Every comparison is one step from the kernel's own fp32 state: snapshot p and the state, run the
kernel, run the oracle on the snapshot, require |kernel - oracle| <= bound element by element.
Every test prints its observed max(error / bound); a ratio above 1 fails.

Branch coverage of the flat kernels (csrc/optim.hip): ``grid_for`` gives ceil(n4 / 256) workgroups
up to the cap of 2048, so the unrolled body ``for (; i + (U-1)*stride < n4; ...)`` only runs for
n4 > U * 2048 * 256. BIG_N = 4 * (4 * 524288 + 777) + 3 has n4 = 2097929 float4, grid 2048,
stride 524288: every lane runs the unrolled body (once for SGD's U = 4, twice for Adam's U = 2),
lanes 0..776 then run the single-float4 loop at 2097152 + i, and 3 elements are left to the scalar
tail -- all three loops in one launch. Views ``alloc[1 : 1 + n]`` are 4-byte aligned only and take
the ``VEC = false`` instantiation.
"""
import numpy as np
import pytest
import torch

import optim_oracle as O

pytestmark = pytest.mark.gpu
DEV = "cuda"
SENT = -777.25           # fills the memory around every sliced operand
SMALL_N = [1, 3, 4, 5, 1027]
BIG_N = 4 * (4 * 524288 + 777) + 3
MULTI_SIZES = [1, 65535, 65536, 65537, 200001, (3, 5)]


@pytest.fixture(scope="module")
def C():
    from tutorial_torch_distributed_data_parallel_amd._native import native

    return native()


class Slot:
    """A device operand: a whole allocation, or a slice [off, off + n) of a sentinel-filled one."""

    def __init__(self, src, off=None, tail=13):
        src = src.reshape(-1)
        if off is None:
            self.alloc = None
            self.t = src.to(DEV)
        else:
            self.alloc = torch.full((off + src.numel() + tail,), SENT, device=DEV)
            self.off, self.n = off, src.numel()
            self.t = self.alloc[off:off + self.n]
            self.t.copy_(src)

    def intact(self):
        if self.alloc is None:
            return True
        return bool((self.alloc[:self.off] == SENT).all()) and \
            bool((self.alloc[self.off + self.n:] == SENT).all())


def _report(family, case, ratios):
    r = max(ratios) if ratios else 0.0
    print(f"[optim-oracle] {family} | {case} | max(error/bound) = {r:.4f}")
    assert r <= 1.0, f"{family} {case}: error exceeds the derived bound, ratio {r}"


def _ratios(actual, out, bound):
    return [O.error_ratio(actual[k], out[k], bound[k]) for k in out]


# ------------------------------------------------------------------------------ hyper block
def _block(C, kind, h, t0=0):
    S = C.hyper_slots()
    blk = torch.zeros(S["size"], device=DEV)
    blk[S["lr"]] = h["lr"]
    blk[S["wd"]] = h["weight_decay"]
    if kind == 1:
        blk[S["mom"]] = h["momentum"]
        blk[S["damp"]] = h["dampening"]
        blk[S["first_next"]] = 1.0
    else:
        blk[S["mom"]] = h["beta1"]
        blk[S["damp"]] = h["beta2"]
        blk[S["eps"]] = h["eps"]
    blk.view(torch.int32)[S["step"]] = t0
    return blk


def _ulp(x):
    return float(np.spacing(np.float32(abs(x))))


def _begin(C, blk, kind, t, first):
    """opt_step_begin + the read-back checks of the slots it owns. Returns the block on the host."""
    S = C.hyper_slots()
    blk[S["scale"]] = 0.125  # a stale clip coefficient: must be reset
    C.opt_step_begin(blk, kind)
    host = blk.cpu()
    assert int(host.view(torch.int32)[S["step"]]) == t
    assert float(host[S["first"]]) == (1.0 if first else 0.0)
    assert float(host[S["first_next"]]) == 0.0
    assert float(host[S["scale"]]) == 1.0
    if kind == 2:
        bc1, bc2s = O.bias_corrections(float(host[S["mom"]]), float(host[S["damp"]]), t, True)
        assert abs(float(host[S["bc1"]]) - bc1) <= _ulp(bc1)
        assert abs(float(host[S["bc2"]]) - bc2s) <= _ulp(bc2s)
    return host


def _sgd_from_block(host, S, h, scale=1.0):
    return O.sgd_hyper(lr=float(host[S["lr"]]),
                       momentum=float(host[S["mom"]]) if h["momentum"] else 0.0,
                       dampening=float(host[S["damp"]]), weight_decay=float(host[S["wd"]]),
                       nesterov=h["nesterov"], maximize=h["maximize"], grad_scale=scale)


def _adam_from_block(host, S, h, scale=1.0):
    return O.adam_hyper(lr=float(host[S["lr"]]), beta1=float(host[S["mom"]]),
                        beta2=float(host[S["damp"]]), eps=float(host[S["eps"]]),
                        weight_decay=float(host[S["wd"]]), amsgrad=h["amsgrad"],
                        maximize=h["maximize"], decoupled=h["decoupled"], grad_scale=scale)


# ------------------------------------------------------------------------------ flat kernels
def _sgd_flat_steps(C, family, case, h, n, off):
    mom = h["momentum"] != 0.0
    st = O.make_state(n, 11)
    p = Slot(st["p"], off)
    buf = Slot(torch.full((n,), float("nan")), off) if mom else None  # never read on step 0
    ratios = []
    for step in range(O.STEPS):
        g = Slot(O.make_grad(n, 11, step), off)
        p0, b0 = p.t.clone(), buf.t.clone() if mom else None
        C.sgd_flat(p.t, g.t, buf.t if mom else None, h["lr"], h["momentum"], h["dampening"],
                   h["weight_decay"], h["nesterov"], h["maximize"], step == 0, h["grad_scale"])
        torch.cuda.synchronize()
        out, bound = O.sgd_step(p0, g.t, b0, h, step == 0)
        ratios += _ratios({"p": p.t, "buf": buf.t if mom else None}, out, bound)
        assert p.intact() and g.intact() and (buf is None or buf.intact()), "sentinel overwritten"
        assert torch.equal(g.t.cpu(), O.make_grad(n, 11, step)), "the gradient was written"
    _report(family, case, ratios)


def _adam_flat_steps(C, family, case, h, n, off):
    st = O.make_state(n, 12)
    p, m, v, x = (Slot(st[k], off) for k in ("p", "m", "v", "vmax"))
    ratios = []
    for step in range(O.STEPS):
        t = O.ADAM_T0 + step
        g = Slot(O.make_grad(n, 12, step), off)
        snap = [s.t.clone() for s in (p, m, v, x)]
        C.adam_flat(p.t, g.t, m.t, v.t, x.t if h["amsgrad"] else None, h["lr"], h["beta1"],
                    h["beta2"], h["eps"], h["weight_decay"], h["amsgrad"], h["maximize"],
                    h["decoupled"], t, h["grad_scale"])
        torch.cuda.synchronize()
        bc1, bc2s = (O.f32(b) for b in O.bias_corrections(h["beta1"], h["beta2"], t, False))
        out, bound = O.adam_step(snap[0], g.t, snap[1], snap[2], snap[3], h, bc1, bc2s)
        ratios += _ratios({"p": p.t, "m": m.t, "v": v.t, "vmax": x.t}, out, bound)
        if not h["amsgrad"]:
            assert torch.equal(x.t, snap[3]), "vmax written without amsgrad"
        assert all(s.intact() for s in (p, g, m, v, x)), "sentinel overwritten"
    _report(family, case, ratios)


@pytest.mark.parametrize("off", [None, 1], ids=["aligned", "view"])
@pytest.mark.parametrize("n", SMALL_N)
@pytest.mark.parametrize("name", list(O.SGD_FLAGS))
def test_sgd_flat_small(C, name, n, off):
    _sgd_flat_steps(C, "sgd_flat " + ("VEC=false view" if off else "VEC"), f"{name} n={n}",
                    O.SGD_FLAGS[name], n, off)


@pytest.mark.parametrize("off", [None, 1], ids=["aligned", "view"])
@pytest.mark.parametrize("n", SMALL_N)
@pytest.mark.parametrize("name", list(O.ADAM_FLAGS))
def test_adam_flat_small(C, name, n, off):
    _adam_flat_steps(C, "adam_flat " + ("VEC=false view" if off else "VEC"), f"{name} n={n}",
                     O.ADAM_FLAGS[name], n, off)


@pytest.mark.parametrize("name", ["plain", "nesterov_wd"])
def test_sgd_flat_past_grid_cap(C, name):
    """Unrolled non-temporal body + single-float4 loop + scalar tail in one launch (see above)."""
    _sgd_flat_steps(C, "sgd_flat unrolled body", f"{name} n={BIG_N}", O.SGD_FLAGS[name], BIG_N,
                    None)


@pytest.mark.parametrize("name", ["l2", "amsgrad"])
def test_adam_flat_past_grid_cap(C, name):
    """Without amsgrad: the unrolled body (U = 2) twice per lane, then the two remainder loops;
    with amsgrad the kernel skips the unrolled body and grid-strides the float4 loop."""
    _adam_flat_steps(C, "adam_flat unrolled body", f"{name} n={BIG_N}", O.ADAM_FLAGS[name],
                     BIG_N, None)


# ------------------------------------------------------------------------------ multi kernels
def _numel(s):
    return int(np.prod(s))


@pytest.mark.parametrize("name", list(O.SGD_FLAGS))
def test_sgd_multi(C, name):
    h = O.SGD_FLAGS[name]
    mom = h["momentum"] != 0.0
    ps = [O.make_state(_numel(s), 20 + i)["p"].reshape(s).to(DEV)
          for i, s in enumerate(MULTI_SIZES)]
    bufs = [torch.full_like(p, float("nan")) for p in ps] if mom else []
    ratios = []
    for step in range(O.STEPS):
        gs = [O.make_grad(p.numel(), 20 + i, step).reshape(p.shape).to(DEV)
              for i, p in enumerate(ps)]
        p0 = [p.clone() for p in ps]
        b0 = [b.clone() for b in bufs]
        C.sgd_multi(ps, gs, bufs, h["lr"], h["momentum"], h["dampening"], h["weight_decay"],
                    h["nesterov"], h["maximize"], step == 0, h["grad_scale"])
        torch.cuda.synchronize()
        for i, p in enumerate(ps):
            out, bound = O.sgd_step(p0[i], gs[i], b0[i] if mom else None, h, step == 0)
            ratios += _ratios({"p": p, "buf": bufs[i] if mom else None}, out, bound)
    _report("sgd_multi", name, ratios)


@pytest.mark.parametrize("name", list(O.ADAM_FLAGS))
def test_adam_multi(C, name):
    h = O.ADAM_FLAGS[name]
    sts = [O.make_state(_numel(s), 30 + i) for i, s in enumerate(MULTI_SIZES)]
    ps, ms, vs, xs = ([st[k].reshape(s).to(DEV) for st, s in zip(sts, MULTI_SIZES)]
                      for k in ("p", "m", "v", "vmax"))
    ratios = []
    for step in range(O.STEPS):
        t = O.ADAM_T0 + step
        gs = [O.make_grad(p.numel(), 30 + i, step).reshape(p.shape).to(DEV)
              for i, p in enumerate(ps)]
        snap = [[q.clone() for q in qs] for qs in (ps, ms, vs, xs)]
        C.adam_multi(ps, gs, ms, vs, xs if h["amsgrad"] else [], h["lr"], h["beta1"], h["beta2"],
                     h["eps"], h["weight_decay"], h["amsgrad"], h["maximize"], h["decoupled"], t,
                     h["grad_scale"])
        torch.cuda.synchronize()
        bc1, bc2s = (O.f32(b) for b in O.bias_corrections(h["beta1"], h["beta2"], t, False))
        for i in range(len(ps)):
            out, bound = O.adam_step(snap[0][i], gs[i], snap[1][i], snap[2][i], snap[3][i], h,
                                     bc1, bc2s)
            ratios += _ratios({"p": ps[i], "m": ms[i], "v": vs[i], "vmax": xs[i]}, out, bound)
            if not h["amsgrad"]:
                assert torch.equal(xs[i], snap[3][i])
    _report("adam_multi", name, ratios)


# ------------------------------------------------------------------------------ hyper-block path
# O.HB_SGD / O.HB_ADAM carry grad_scale = 0.25: blk[scale] = 0.5 times the by-value 0.5.
HB_SCALE = 0.5
assert HB_SCALE * HB_SCALE == O.HB_SGD["grad_scale"] == O.HB_ADAM["grad_scale"]


@pytest.mark.parametrize("multi", [False, True], ids=["flat", "multi"])
def test_sgd_hyper_block(C, multi):
    """Scalars from the device block; the by-value ones are deliberately wrong (only momentum != 0
    is structural). lr changes before step 3; blk[scale] = 0.5 times by-value 0.5 is 0.25."""
    S, h = C.hyper_slots(), O.HB_SGD
    sizes = MULTI_SIZES if multi else [1027]
    ps = [O.make_state(_numel(s), O.HB_SGD_SEED + i)["p"].reshape(s).to(DEV)
          for i, s in enumerate(sizes)]
    bufs = [torch.full_like(p, float("nan")) for p in ps]
    blk = _block(C, 1, h)
    ratios = []
    for step in range(O.STEPS):
        if step == 2:
            blk[S["lr"]] = 0.5 * h["lr"]
        _begin(C, blk, 1, step + 1, first=step == 0)
        blk[S["scale"]] = HB_SCALE
        host = blk.cpu()
        gs = [O.make_grad(p.numel(), O.HB_SGD_SEED + i, step).reshape(p.shape).to(DEV)
              for i, p in enumerate(ps)]
        p0, b0 = [p.clone() for p in ps], [b.clone() for b in bufs]
        wrong = (123.0, 0.5, 0.875, 55.0, h["nesterov"], h["maximize"], step != 0, HB_SCALE)
        if multi:
            C.sgd_multi(ps, gs, bufs, *wrong, hyper=blk)
        else:
            C.sgd_flat(ps[0], gs[0], bufs[0], *wrong, hyper=blk)
        torch.cuda.synchronize()
        he = _sgd_from_block(host, S, h, scale=h["grad_scale"])
        assert he["lr"] == O.f32(h["lr"] * (0.5 if step == 2 else 1.0))
        for i, p in enumerate(ps):
            out, bound = O.sgd_step(p0[i], gs[i], b0[i], he, step == 0)
            ratios += _ratios({"p": p, "buf": bufs[i]}, out, bound)
    _report("hyper block", "sgd_multi" if multi else "sgd_flat", ratios)


@pytest.mark.parametrize("multi", [False, True], ids=["flat", "multi"])
def test_adam_hyper_block(C, multi):
    S, h = C.hyper_slots(), O.HB_ADAM
    sizes = MULTI_SIZES if multi else [1027]
    sts = [O.make_state(_numel(s), O.HB_ADAM_SEED + i) for i, s in enumerate(sizes)]
    ps, ms, vs, xs = ([st[k].reshape(s).to(DEV) for st, s in zip(sts, sizes)]
                      for k in ("p", "m", "v", "vmax"))
    blk = _block(C, 2, h, t0=O.ADAM_T0 - 1)
    ratios = []
    for step in range(O.STEPS):
        if step == 2:
            blk[S["lr"]] = 0.5 * h["lr"]
        _begin(C, blk, 2, O.ADAM_T0 + step, first=False)
        blk[S["scale"]] = HB_SCALE
        host = blk.cpu()
        gs = [O.make_grad(p.numel(), O.HB_ADAM_SEED + i, step).reshape(p.shape).to(DEV)
              for i, p in enumerate(ps)]
        snap = [[q.clone() for q in qs] for qs in (ps, ms, vs, xs)]
        # by value: wrong scalars and a wrong step (bias corrections of t = 40)
        wrong = (123.0, 0.5, 0.5, 7.0, 55.0, h["amsgrad"], h["maximize"], h["decoupled"], 40,
                 HB_SCALE)
        if multi:
            C.adam_multi(ps, gs, ms, vs, xs, *wrong, hyper=blk)
        else:
            C.adam_flat(ps[0], gs[0], ms[0], vs[0], xs[0], *wrong, hyper=blk)
        torch.cuda.synchronize()
        he = _adam_from_block(host, S, h, scale=h["grad_scale"])
        bc1, bc2s = float(host[S["bc1"]]), float(host[S["bc2"]])
        for i in range(len(ps)):
            out, bound = O.adam_step(snap[0][i], gs[i], snap[1][i], snap[2][i], snap[3][i], he,
                                     bc1, bc2s)
            ratios += _ratios({"p": ps[i], "m": ms[i], "v": vs[i], "vmax": xs[i]}, out, bound)
    _report("hyper block", "adam_multi" if multi else "adam_flat", ratios)


# ------------------------------------------------------------------------------ GEMM epilogue
# Operands (O.make_operands) are integers in [-15, 15] times 2^-3, stored [K][M] and [K][N]: the
# weight gradient A^T B is exact in fp32, the only rounding left is the element update.
def _operands(M, N, K, seed):
    A, B = O.make_operands(M, N, K, seed)
    return A.to(DEV), B.to(DEV)


class _Override:
    """gemm_f32_set_override(fn, 0, 0), the epilogue variant and lockstep; all restored."""

    def __init__(self, C, fn=0, sgd=-1, adam=-1, persist=-1, lockstep=False):
        self.C, self.fn, self.var, self.lockstep = C, fn, (sgd, adam, persist), lockstep

    def __enter__(self):
        C = self.C
        self.old_var = C.gemm_f32_set_opt_variant()
        self.old_ls = C.gemm_f32_lockstep()
        C.gemm_f32_set_override(self.fn, 0, 0)
        C.gemm_f32_set_opt_variant(sgd=self.var[0], adam=self.var[1], persist=self.var[2])
        C.gemm_f32_set_lockstep(self.lockstep)

    def __exit__(self, *exc):
        C = self.C
        # the override has no getter: (0, 0, 0) is the process default, and what every other
        # test that sets an override leaves behind
        C.gemm_f32_set_override(0, 0, 0)
        C.gemm_f32_set_opt_variant(*self.old_var)
        C.gemm_f32_set_lockstep(self.old_ls)


EPI_SGD, EPI_ADAM = O.EPI_SGD_FLAGS, O.EPI_ADAM_FLAGS
EPI_SHAPES = [(1, 132, 68), (1, 4, 4), (1, 128, 64), (2, 132, 516), (2, 260, 132)]
BIAS_TAIL = 128  # sentinel floats behind a bias slice: one tile's rows


def _wtail(M, N):
    """Sentinel floats behind a weight slice: every row of the last 128-row tile below M (a whole
    tile where M is a multiple of 128), so a broken ``row < p.M`` guard writes into it entirely."""
    return (128 - M % 128) * N


def _ran_lockstep(C, lockstep, refused=False):
    """wgrad_lockstep_kernel ran exactly where the test means it to: lockstep_ok falls back to the
    persistent kernel without notice (split-bf16 products off, amsgrad, a misaligned slice)."""
    if lockstep:
        assert C.gemm_f32_emu() and C.gemm_f32_lockstep()
    assert C.gemm_f32_epilogue_lockstep() is (lockstep and not refused)


def _epilogue_sgd(C, family, case, h, M, N, K, steps=2, lockstep=False):
    """Weight and bias slices inside sentinel arenas (offsets multiples of 4 floats); first = 1
    then 0 through opt_step_begin; the bias gradient is the exact column sum of the stored A."""
    S = C.hyper_slots()
    mom = h["momentum"] != 0.0
    p = Slot(O.make_state(M * N, O.EPI_SGD_STATE_SEED)["p"], 8, tail=_wtail(M, N))
    bp = Slot(O.make_state(M, O.EPI_SGD_STATE_SEED + 1)["p"], 4, tail=BIAS_TAIL)
    buf = Slot(torch.full((M * N,), float("nan")), 12, tail=_wtail(M, N)) if mom else None
    bbuf = Slot(torch.full((M,), float("nan")), 8, tail=BIAS_TAIL) if mom else None
    blk = _block(C, 1, h)
    ratios = []
    for step in range(steps):
        A, B = _operands(M, N, K, O.EPI_SGD_SEED + step)
        _begin(C, blk, 1, step + 1, first=step == 0)
        host = blk.cpu()
        Cm = torch.full((M, N), SENT, device=DEV)
        rs = torch.full((M,), SENT, device=DEV)
        snap = [s.t.clone() if s is not None else None for s in (p, buf, bp, bbuf)]
        ran = C.gemm_f32_sgd(A, B, Cm, False, False, p.t, buf.t if mom else None, blk,
                             h["nesterov"], h["maximize"], rs, bp.t, bbuf.t if mom else None)
        torch.cuda.synchronize()
        assert ran is True, "the optimizer epilogue did not run"
        _ran_lockstep(C, lockstep)
        assert bool((Cm == SENT).all()), "C was written"
        assert bool((rs == SENT).all()), "rowsum was written"
        he = _sgd_from_block(host, S, h)
        gw = (A.double().t() @ B.double()).reshape(-1)
        gb = A.double().sum(0)
        out, bound = O.sgd_step(snap[0], gw, snap[1], he, step == 0)
        ratios += _ratios({"p": p.t, "buf": buf.t if mom else None}, out, bound)
        out, bound = O.sgd_step(snap[2], gb, snap[3], he, step == 0)
        ratios += _ratios({"p": bp.t, "buf": bbuf.t if mom else None}, out, bound)
        for s in (p, buf, bp, bbuf):
            assert s is None or s.intact(), "a neighbour in the arena was overwritten"
    _report(family, case, ratios)


def _epilogue_adam(C, family, case, h, M, N, K, steps=2, lockstep=False):
    S = C.hyper_slots()
    ams = h["amsgrad"]
    w = O.make_state(M * N, 70)
    b = O.make_state(M, 71)
    ws = [Slot(w[k], 4 * (i + 1), tail=_wtail(M, N))
          for i, k in enumerate(("p", "m", "v", "vmax"))]
    bs = [Slot(b[k], 4 * (i + 2), tail=BIAS_TAIL) for i, k in enumerate(("p", "m", "v", "vmax"))]
    blk = _block(C, 2, h)
    ratios = []
    for step in range(steps):
        A, B = _operands(M, N, K, 200 + step)
        host = _begin(C, blk, 2, step + 1, first=False)
        Cm = torch.full((M, N), SENT, device=DEV)
        rs = torch.full((M,), SENT, device=DEV)
        sw, sb = [s.t.clone() for s in ws], [s.t.clone() for s in bs]
        ran = C.gemm_f32_adam(A, B, Cm, False, False, ws[0].t, ws[1].t, ws[2].t,
                              ws[3].t if ams else None, blk, ams, h["maximize"], h["decoupled"],
                              rs, bs[0].t, bs[1].t, bs[2].t, bs[3].t if ams else None)
        torch.cuda.synchronize()
        assert ran is True, "the optimizer epilogue did not run"
        _ran_lockstep(C, lockstep, refused=ams)
        assert bool((Cm == SENT).all()), "C was written"
        assert bool((rs == SENT).all()), "rowsum was written"
        he = _adam_from_block(host, S, h)
        bc1, bc2s = float(host[S["bc1"]]), float(host[S["bc2"]])
        gw = (A.double().t() @ B.double()).reshape(-1)
        gb = A.double().sum(0)
        for slots, snap, g in ((ws, sw, gw), (bs, sb, gb)):
            out, bound = O.adam_step(snap[0], g, snap[1], snap[2], snap[3], he, bc1, bc2s)
            ratios += _ratios(dict(zip(("p", "m", "v", "vmax"), (s.t for s in slots))), out, bound)
            if not ams:
                assert torch.equal(slots[3].t, snap[3]), "vmax written without amsgrad"
            assert all(s.intact() for s in slots), "a neighbour in the arena was overwritten"
    _report(family, case, ratios)


@pytest.mark.parametrize("K", [8, 32])
@pytest.mark.parametrize("fn,M,N", EPI_SHAPES)
@pytest.mark.parametrize("name", list(EPI_SGD))
def test_gemm_epilogue_sgd_shapes(C, name, fn, M, N, K):
    with _Override(C, fn=fn):
        _epilogue_sgd(C, f"gemm epilogue sgd fn={fn}", f"{name} {M}x{N} K={K}", EPI_SGD[name],
                      M, N, K)


@pytest.mark.parametrize("persist", [0, 1])
@pytest.mark.parametrize("variant", [0, 4, 8, 12, 16, 24, 28, 88])
def test_gemm_epilogue_sgd_variants(C, variant, persist):
    with _Override(C, fn=2, sgd=variant, persist=persist):
        _epilogue_sgd(C, "gemm epilogue sgd variants", f"variant={variant} persist={persist}",
                      EPI_SGD["momentum_dampening_wd"], 132, 516, 32)


@pytest.mark.parametrize("name", list(EPI_SGD))
def test_gemm_epilogue_sgd_lockstep(C, name):
    with _Override(C, lockstep=True):
        _epilogue_sgd(C, "gemm epilogue sgd lockstep", f"{name} 132x516 K=128", EPI_SGD[name],
                      132, 516, 128, lockstep=True)


@pytest.mark.parametrize("K", [8, 32])
@pytest.mark.parametrize("fn,M,N", EPI_SHAPES)
@pytest.mark.parametrize("name", list(EPI_ADAM))
def test_gemm_epilogue_adam_shapes(C, name, fn, M, N, K):
    with _Override(C, fn=fn):
        _epilogue_adam(C, f"gemm epilogue adam fn={fn}", f"{name} {M}x{N} K={K}", EPI_ADAM[name],
                       M, N, K)


@pytest.mark.parametrize("persist", [0, 1])
@pytest.mark.parametrize("variant", [0, 16, 24, 28, 88])
@pytest.mark.parametrize("name", ["l2", "amsgrad"])
def test_gemm_epilogue_adam_variants(C, name, variant, persist):
    with _Override(C, fn=2, adam=variant, persist=persist):
        _epilogue_adam(C, "gemm epilogue adam variants",
                       f"{name} variant={variant} persist={persist}", EPI_ADAM[name], 132, 516, 32)


@pytest.mark.parametrize("name", list(EPI_ADAM))
def test_gemm_epilogue_adam_lockstep(C, name):
    """The lockstep kernel refuses amsgrad (lockstep_ok): that case must still come out right,
    through the persistent kernel (_ran_lockstep asserts which of the two ran)."""
    with _Override(C, lockstep=True):
        _epilogue_adam(C, "gemm epilogue adam lockstep", f"{name} 132x516 K=128", EPI_ADAM[name],
                       132, 516, 128, lockstep=True)


# ------------------------------------------------------------------------------ refusals
# Each of these used to reach a kernel with a null, host, foreign-dtype or too-short pointer. The
# host checks in csrc/bindings.cpp (check_like / check_list) precede chunk_table and every launch.
def _multi_args(n=8, count=2):
    mk = lambda: [torch.zeros(n, device=DEV) for _ in range(count)]  # noqa: E731
    return mk(), mk(), mk(), mk(), mk()


SGD_TAIL = (0.1, 0.9, 0.0, 0.0, False, False, True, 1.0)
ADAM_TAIL = (1e-3, 0.9, 0.999, 1e-8, 0.0)


def test_refuse_sgd_multi_missing_buffers(C):
    ps, gs, bufs, _, _ = _multi_args()
    before = [p.clone() for p in ps]
    with pytest.raises(RuntimeError):
        C.sgd_multi(ps, gs, [], *SGD_TAIL)
    with pytest.raises(RuntimeError):
        C.sgd_multi(ps, gs, bufs[:1], *SGD_TAIL)
    torch.cuda.synchronize()
    assert all(torch.equal(a, b) for a, b in zip(ps, before))


@pytest.mark.parametrize("case", ["short_list", "wrong_numel", "non_contiguous", "cpu_state",
                                  "amsgrad_without_vmaxs"])
def test_refuse_adam_multi(C, case):
    ps, gs, ms, vs, xs = _multi_args()
    ams = False
    if case == "short_list":
        ms = ms[:1]
    elif case == "wrong_numel":
        vs[1] = torch.zeros(4, device=DEV)
    elif case == "non_contiguous":
        ms[0] = torch.zeros(16, device=DEV)[::2]
    elif case == "cpu_state":
        vs[0] = torch.zeros(8)
    else:
        ams, xs = True, []
    with pytest.raises(RuntimeError):
        C.adam_multi(ps, gs, ms, vs, xs, *ADAM_TAIL, ams, False, False, 1, 1.0)
    torch.cuda.synchronize()
    assert all(bool((p == 0).all()) for p in ps)


def test_refuse_adam_flat(C):
    p, g, m, v = (torch.zeros(8, device=DEV) for _ in range(4))
    with pytest.raises(RuntimeError):
        C.adam_flat(p, g, torch.zeros(16, device=DEV)[::2], v, None, *ADAM_TAIL, False, False,
                    False, 1, 1.0)
    with pytest.raises(RuntimeError):
        C.adam_flat(p, g.double(), m, v, None, *ADAM_TAIL, False, False, False, 1, 1.0)
    torch.cuda.synchronize()
    assert bool((p == 0).all())
