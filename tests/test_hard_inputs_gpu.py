"""The kernels around the GEMMs (cross-entropy family, max-pool, BatchNorm moments and the conv
epilogue statistics) on the inputs where such kernels go wrong -- large logits, masked (-inf)
classes, ties, NaN, large-mean / small-spread channels, degenerate batches -- against a float64
CPU reference computed from the same fp32 inputs.

Tolerance rule (``_rule``). For a quantity q: e_k = max|q_kernel - q_f64|, e_t = the same for
torch's own fp32 result on the GPU, and the assertion is

    e_k <= 4 * e_t + c * 2**-24 * scale

with ``scale`` the natural magnitude of q (1 for probabilities and for batch-size-times-gradient,
max|q_f64| otherwise) and ``c`` one constant per quantity (``C_``), chosen once after a first
device run and recorded, with the measured e_k / e_t, in the docstring of the test that uses it.
The factor 4 allows for another summation order (test_emu_matches_fp64_like_native_f32). No bound
is derived from the kernel's own output."""
import math

import numpy as np
import pytest
import torch
import torch.nn.functional as F

pytestmark = pytest.mark.gpu

U = 2.0 ** -24

# c of the tolerance rule, one per quantity. Chosen after the first MI355X run of this file from
# the largest c any case needed, (e_k - 4 e_t) / (2**-24 scale), given on the right with the case
# that needed it (a negative figure: 4 e_t alone covered every case); the docstrings name the
# e_k / e_t behind them.
C_ = {
    "loss": 4,    # 1.09  ce[70x1000 eps=0.1 sum] loss: e_k 5.5e-5, e_t 5.6e-6, scale 508
    "lse": 2,     # -0.16 scale[128x10 s=1000] lse: e_k = e_t = 1.0e-5, scale 3143
    "grad": 2,    # -0.29 one-valid[16x10] dpre: e_k 4.4e-8, e_t 1.5e-8 (B * dlogits, scale 1)
    "head": 2,    # -6.2  linear_cross_entropy[w*0.1] db: e_k 1.2e-8, e_t 9.1e-9, scale 0.066
    "mean": 2,    # -0.37 bn_moments(4,64,7,7) mean[off=0]: e_k 2.7e-8, e_t 1.2e-8, scale 1
    "var": 2,     # 0.02  epilogue(2,4,33,29,64,7,2) var: e_k 5.3e-4, e_t 1.3e-4, scale 1072
    "bn_y": 2,    # -1.2  bn_eval[1x16] y: e_k = e_t = 6.9e-8, scale 3.0
    "bn_dx": 2,   # -1.6  bn_train[2x18] db: e_k = e_t = 1.2e-7, scale 3.7
}


@pytest.fixture(scope="module")
def C():
    from tutorial_torch_distributed_data_parallel_amd._native import native

    return native()


def _err(a, ref):
    a, ref = a.detach().double().cpu(), ref.detach().double().cpu()
    assert a.shape == ref.shape, (a.shape, ref.shape)
    if a.numel() == 0:
        return 0.0
    d = (a - ref).abs()
    d = torch.where(a == ref, torch.zeros_like(d), d)  # equal infinities are no error
    return d.max().item() if not torch.isnan(d).any() else float("nan")


def _figures(what, got, t32, ref, c, scale=None):
    """(e_k, e_t, the rule's bound, scale) of one quantity, printed."""
    e_k, e_t = _err(got, ref), _err(t32, ref)
    if scale is None:
        scale = ref.detach().double().abs().max().item() if ref.numel() else 0.0
    bound = 4 * e_t + c * U * scale
    print(f"[rule] {what}: e_k={e_k:.3e} e_t={e_t:.3e} c={c} scale={scale:.3e} bound={bound:.3e}")
    return e_k, e_t, bound, scale


def _rule(what, got, t32, ref, c, scale=None):
    """Assert the module's tolerance rule for one quantity; prints the figures first."""
    e_k, e_t, bound, scale = _figures(what, got, t32, ref, c, scale)
    assert e_k <= bound, f"{what}: e_k {e_k:.3e} > 4 * {e_t:.3e} + {c} * 2^-24 * {scale:.3e}"
    return e_k, e_t


# ------------------------------------------------------------------------------ cross-entropy
def _ce_ref(z, y, eps, reduction, dtype, dev):
    """(loss, dlogits, lse, per-row loss sum) of F.cross_entropy in ``dtype`` on ``dev``."""
    zz = z.detach().to(device=dev, dtype=dtype).requires_grad_()
    yy = y.to(dev)
    loss = F.cross_entropy(zz, yy, label_smoothing=eps, reduction=reduction)
    (g,) = torch.autograd.grad(loss, zz)
    with torch.no_grad():
        total = F.cross_entropy(zz, yy, label_smoothing=eps, reduction="sum")
        lse = torch.logsumexp(zz, 1)
    return loss.detach(), g, lse, total


def _argmax_lowest(z):
    a = z.detach().cpu().numpy()
    return np.array([int(np.flatnonzero(r == r.max())[0]) for r in a])


def _labels(B, Cl, gen, ignore_row=None):
    y = torch.randint(0, Cl, (B,), generator=gen).cuda()
    if ignore_row is not None:
        y[ignore_row] = -100
    return y


def _check_ce(C, z, y, eps, reduction, tag, fused=None, grads=True):
    """Every output of C.ce_fwd / C.ce_bwd for one configuration against float64 by the rule."""
    B, Cl = z.shape
    mean = reduction == "mean"
    r64 = _ce_ref(z, y, eps, reduction, torch.float64, "cpu")
    r32 = _ce_ref(z, y, eps, reduction, torch.float32, "cuda")
    valid = (y != -100)
    nvalid = int(valid.sum().item())
    gs = float(nvalid) if mean else 1.0  # "B times the gradient": a mean's rows carry 1 / B
    correct = int(((torch.from_numpy(_argmax_lowest(z)).cuda() == y) & valid).sum().item())
    if fused is None:
        fused = B * Cl <= (1 << 16)
    acc = torch.tensor([0.0, 5.0, 7.0], device="cuda")
    out = C.ce_fwd(z, y, -100, eps, mean, acc, with_grad=fused)
    loss, lse = out[0], out[1]
    _rule(f"{tag} loss", loss, r32[0], r64[0], C_["loss"])
    _rule(f"{tag} lse", lse[:B], r32[2], r64[2], C_["lse"])
    assert lse[B].item() == nvalid
    _rule(f"{tag} acc[0]", acc[0], r32[3], r64[3], C_["loss"])
    assert acc[1].item() == 5.0 + correct and acc[2].item() == 7.0 + nvalid
    # the forward without the gradient: the same loss and per-row values, bit for bit
    o2 = C.ce_fwd(z, y, -100, eps, mean, None)
    assert len(o2) == 2 and torch.equal(o2[0], loss) and torch.equal(o2[1], lse)
    if not grads:
        return out
    if fused:
        _rule(f"{tag} dpre", out[2] * gs, r32[1] * gs, r64[1] * gs, C_["grad"], 1.0)
        assert not out[2][~valid].any(), "ignored rows carry no gradient"
    for gout in (1.0, 0.5):
        d = C.ce_bwd(z, y, lse, torch.full((1,), gout, device="cuda"), -100, eps, mean)
        _rule(f"{tag} ce_bwd({gout})", d * gs, r32[1] * (gs * gout), r64[1] * (gs * gout),
              C_["grad"], 1.0)
        if fused and gout == 1.0:
            assert torch.equal(d, out[2]), "ce_bwd and the fused gradient share one formula"
    return out


CE_SHAPES = [(7, 3), (128, 10), (256, 32),          # one row per lane
             (257, 10), (600, 32),                  # strided row_serial
             (5, 33), (9, 64), (3, 65), (64, 1000),  # one wave per row
             (70, 1000)]                            # numel > 65536: no fused gradient


@pytest.mark.parametrize("B,Cl", CE_SHAPES)
def test_ce_paths(C, B, Cl):
    """Every row path of ce_fwd_kernel and both sides of its thresholds, label smoothing 0 / 0.1,
    mean / sum, one ignored row: loss, lse, the denominator, acc, the fused gradient and ce_bwd
    (gout 1 and 0.5); ops.cross_entropy's backward for the unit seed (ce_bwd when the logits are
    too many for the fused gradient).

    Measured on MI355X, worst over the shapes: loss e_k 5.5e-5 / e_t 5.6e-6 at scale 508
    ((70,1000), sum); lse e_k = e_t = 1.1e-7; B * dlogits e_k 2.6e-8 / e_t 1.8e-8 ((3,65))."""
    from tutorial_torch_distributed_data_parallel_amd import ops
    from tutorial_torch_distributed_data_parallel_amd.ops import loss as L

    gen = torch.Generator().manual_seed(B * 1000 + Cl)
    z = torch.randn(B, Cl, generator=gen).cuda()
    y = _labels(B, Cl, gen, ignore_row=B // 2)
    for eps in (0.0, 0.1):
        for reduction in ("mean", "sum"):
            _check_ce(C, z, y, eps, reduction, f"ce[{B}x{Cl} eps={eps} {reduction}]")
    zz = z.clone().requires_grad_()
    loss = ops.cross_entropy(zz, y, label_smoothing=0.1)
    assert (loss.grad_fn.dpre is not None) == (B * Cl <= (1 << 16))
    L.backward(loss)
    r64 = _ce_ref(z, y, 0.1, "mean", torch.float64, "cpu")
    r32 = _ce_ref(z, y, 0.1, "mean", torch.float32, "cuda")
    _rule(f"ops.cross_entropy[{B}x{Cl}] loss", loss, r32[0], r64[0], C_["loss"])
    _rule(f"ops.cross_entropy[{B}x{Cl}] grad", zz.grad * (B - 1), r32[1] * (B - 1),
          r64[1] * (B - 1), C_["grad"], 1.0)


def _confident(z, gen):
    """Labels with half the rows on the row's argmax (confident rows), the rest random."""
    B, Cl = z.shape
    y = torch.randint(0, Cl, (B,), generator=gen)
    am = torch.from_numpy(_argmax_lowest(z))
    y[::2] = am[::2]
    return y.cuda()


@pytest.mark.parametrize("s", [1, 30, 100, 1000])
@pytest.mark.parametrize("B,Cl", [(128, 10), (300, 10), (40, 100)])
def test_ce_logit_scale(C, B, Cl, s):
    """randn * s logits with half the targets on the argmax: the loss and B * dlogits obey the
    rule for both fused-gradient branches and ce_bwd. The probability is exp((x - lse) - res)
    with (lse, res) the unevaluated sum max + log(sum exp) (ce_row.h lse_split; res is kept from
    |lse| = 8 upward): rounding lse alone to fp32 costs ulp(|max|) per probability. Measured on MI355X at (128,10), B * dlogits,
    e_k before -> after that split, e_t: s = 30: 1.9e-6 -> 1.3e-7, 1.1e-7; s = 100: 6.6e-6 ->
    1.0e-7, 1.0e-7; s = 1000: 1.0e-5 -> 3.6e-8, 3.6e-8 (the rule holds at s = 1000 too: nothing
    is pinned). Loss: e_k 2.2e-6 / e_t 2.6e-7 at scale 23.6 (s = 30), the largest c needed."""
    gen = torch.Generator().manual_seed(B + Cl + s)
    z = (torch.randn(B, Cl, generator=gen) * s).cuda()
    y = _confident(z, gen)
    for eps, reduction in ((0.0, "mean"), (0.1, "mean"), (0.0, "sum")):
        _check_ce(C, z, y, eps, reduction, f"scale[{B}x{Cl} s={s} eps={eps} {reduction}]")


@pytest.mark.parametrize("B,Cl", [(128, 10), (300, 10), (40, 100)])
def test_ce_lse_residual(C, B, Cl):
    """The saved tensor [lse(B) | valid rows | residual(B)]: lse + residual is the float64
    log-sum-exp to within the error of log(sum exp) itself (a few ulp of log C, not ulp(|max|)) in
    rows with |lse| >= 8; below 8 the residual is exactly 0, which keeps the single-float
    arithmetic -- and a training run at ordinary logits -- bit for bit (csrc/ce_row.h)."""
    gen = torch.Generator().manual_seed(B + Cl)
    scale = torch.tensor([1.0, 3.0, 30.0, 1000.0]).repeat(B)[:B, None]
    z = (torch.randn(B, Cl, generator=gen) * scale).cuda()
    y = _labels(B, Cl, gen)
    lse = C.ce_fwd(z, y, -100, 0.0, True, None)[1]
    val, res = lse[:B].double().cpu(), lse[B + 1:].double().cpu()
    small = val.abs() < 8
    assert small.any() and (~small).any()
    assert (res[small] == 0).all()
    ref = torch.logsumexp(z.double().cpu(), 1)
    err = ((val + res) - ref).abs()[~small].max().item()
    print(f"[lse residual {B}x{Cl}] max |lse + res - f64| = {err:.3e}")
    assert err <= 4 * U * 2 * math.log(Cl)  # log(se) <= log C, 4 ulp of it (__logf, the sum)
    assert (res.abs() <= val.abs() * U).all()


def _head(C, x, w, b, y, eps, mean, acc=None):
    ticket = torch.zeros(16, dtype=torch.int32, device="cuda")
    out = C.head_ce(x, w, b, y, -100, eps, mean, acc, with_grad=True, gate=None, planes=False,
                    ticket=ticket)
    assert out, "head_ce refused a 128 x 64 -> 10 head"
    assert not ticket.any(), "the ticket words are zero again after the launch"
    return out


@pytest.mark.parametrize("wscale", [0.1, 12.0])
def test_head_ce_logit_scale(C, wscale):
    """The fused head + loss (x (128,64) through w (10,64); wscale 12 gives |logit| ~ 100): the
    loss and B * dlogits obey the rule against float64 cross-entropy of the kernel's own fp32
    logits, and ops.linear_cross_entropy's loss, dx, dW, db against the float64 head.

    Measured (w * 12): B * dlogits e_k = e_t = 7.1e-8 (4.2e-6 before lse_split), c = 2; loss
    e_k = e_t = 2.4e-6 at scale 87, c = 4; dW e_k 1.6e-8 / e_t 1.7e-8 at scale 0.094 (w * 0.1)."""
    from tutorial_torch_distributed_data_parallel_amd import ops
    from tutorial_torch_distributed_data_parallel_amd.ops import loss as L

    gen = torch.Generator().manual_seed(17)
    x = torch.randn(128, 64, generator=gen).cuda()
    w = (torch.randn(10, 64, generator=gen) * wscale).cuda()
    b = torch.randn(10, generator=gen).cuda()
    with torch.no_grad():
        y = _confident(x @ w.t() + b, gen)
    y[5] = -100
    nv = 127.0
    for eps in (0.0, 0.1):
        out = _head(C, x, w, b, y, eps, True)
        loss, lse, logits, d = out[0], out[1], out[2], out[3]
        assert wscale < 1 or logits.abs().max().item() > 100
        r64 = _ce_ref(logits, y, eps, "mean", torch.float64, "cpu")
        r32 = _ce_ref(logits, y, eps, "mean", torch.float32, "cuda")
        tag = f"head_ce[w*{wscale} eps={eps}]"
        _rule(f"{tag} loss", loss, r32[0], r64[0], C_["loss"])
        _rule(f"{tag} lse", lse[:128], r32[2], r64[2], C_["lse"])
        _rule(f"{tag} dlogits", d * nv, r32[1] * nv, r64[1] * nv, C_["grad"], 1.0)
        assert lse[128].item() == nv
        d2 = C.ce_bwd(logits, y, lse, torch.ones(1, device="cuda"), -100, eps, True)
        assert torch.equal(d, d2)

    def torch_head(xs, ws, bs, yy):
        return F.cross_entropy(F.linear(xs, ws, bs), yy)

    def run(dtype, dev, fn, backward):
        xs, ws, bs = (t.detach().to(device=dev, dtype=dtype).requires_grad_() for t in (x, w, b))
        loss = fn(xs, ws, bs, y.to(dev))
        backward(loss)
        return loss.detach(), xs.grad, ws.grad, bs.grad

    # the unit seed: the gradients the forward launch itself produced
    got = run(torch.float32, "cuda", ops.linear_cross_entropy, L.backward)
    t32 = run(torch.float32, "cuda", torch_head, torch.Tensor.backward)
    r64 = run(torch.float64, "cpu", torch_head, torch.Tensor.backward)
    for name, g, t, r in zip(("loss", "dx", "dW", "db"), got, t32, r64):
        _rule(f"linear_cross_entropy[w*{wscale}] {name}", g, t, r,
              C_["loss"] if name == "loss" else C_["head"])


def _masked_logits(B, Cl, nmask, gen):
    z = torch.randn(B, Cl, generator=gen) * 3
    y = torch.randint(0, Cl, (B,), generator=gen)
    mask = torch.zeros(B, Cl, dtype=torch.bool)
    for r in range(B):
        cols = [c for c in torch.randperm(Cl, generator=gen).tolist() if c != int(y[r])][:nmask]
        mask[r, cols] = True
    z[mask] = -math.inf
    return z.cuda(), y.cuda(), mask.cuda()


@pytest.mark.parametrize("nmask", [1, 3])
@pytest.mark.parametrize("B,Cl", [(64, 10), (300, 10), (6, 100)])
def test_ce_masked_classes(C, B, Cl, nmask):
    """-inf logits (masked classes, never the target) in each row path. Without smoothing the
    loss and gradient are finite, obey the rule and the gradient is exactly 0 in the masked
    columns (a zero smoothing weight must not multiply the row sum: 0 * -inf). With smoothing the
    loss is +inf, as in torch.

    Measured: loss e_k = e_t = 1.1e-7 at scale 4.7 (NaN before the fix), c = 4; B * dlogits
    e_k 4.8e-8 / e_t 3.3e-8, c = 2."""
    gen = torch.Generator().manual_seed(B + Cl + nmask)
    z, y, mask = _masked_logits(B, Cl, nmask, gen)
    for reduction in ("mean", "sum"):
        out = _check_ce(C, z, y, 0.0, reduction, f"masked[{B}x{Cl} n={nmask} {reduction}]")
        assert torch.isfinite(out[0]) and torch.isfinite(out[2]).all()
        assert (out[2][mask] == 0).all()
        d = C.ce_bwd(z, y, out[1], torch.ones(1, device="cuda"), -100, 0.0, reduction == "mean")
        assert torch.isfinite(d).all() and (d[mask] == 0).all()
    ref = F.cross_entropy(z.double().cpu(), y.cpu(), label_smoothing=0.1)
    loss = C.ce_fwd(z, y, -100, 0.1, True, None)[0]
    assert ref.item() == math.inf and loss.item() == math.inf


@pytest.mark.parametrize("B,Cl", [(64, 10), (300, 10), (6, 100)])
def test_ce_row_sum_overflow(C, B, Cl):
    """Logits at +-3e38 without smoothing: the row sum overflows to +inf (even rows: two logits at
    3e38, one of them the target) or -inf (odd rows: two at -3e38); loss and gradient stay finite
    and obey the rule: the loss log 2 of an even row lies wholly in the residual of lse (3e38).

    Measured: loss e_k 2.1e-5 / e_t 9.8e-6 at scale 481 ((300,10), sum; NaN before the fix),
    c = 4; B * dlogits e_k = e_t = 2.3e-8, c = 2."""
    gen = torch.Generator().manual_seed(B + Cl)
    z = torch.randn(B, Cl, generator=gen)
    y = torch.randint(2, Cl, (B,), generator=gen)
    z[::2, 0] = 3e38
    z[::2, 1] = 3e38
    z[::2, 2] = -3e38
    y[::2] = torch.randint(0, 2, (len(y[::2]),), generator=gen)
    z[1::2, 0] = -3e38
    z[1::2, 1] = -3e38
    z, y = z.cuda(), y.cuda()
    for reduction in ("mean", "sum"):
        out = _check_ce(C, z, y, 0.0, reduction, f"overflow[{B}x{Cl} {reduction}]")
        assert torch.isfinite(out[0]) and torch.isfinite(out[2]).all()


def _tie_cases():
    cases = []
    for B, Cl in ((16, 10), (300, 10), (6, 100)):
        cases.append((f"const[{B}x{Cl}]", B, Cl, None))
        cases.append((f"max@3,7[{B}x{Cl}]", B, Cl, (3, 7)))
    cases.append(("max@1,65,129[9x200]", 9, 200, (1, 65, 129)))  # one lane's strided scan
    cases.append(("max@70,5,135[9x200]", 9, 200, (70, 5, 135)))  # lanes 6, 5, 7: the merge
    cases.append(("max@last[5x65]", 5, 65, (64,)))
    cases.append(("max@last[5x1000]", 5, 1000, (999,)))
    return cases


@pytest.mark.parametrize("name,B,Cl,at", _tie_cases(), ids=[c[0] for c in _tie_cases()])
def test_ce_argmax_ties(C, name, B, Cl, at):
    """The lowest index of the maximum wins (row_serial's scan, row_wave's shuffle merge across
    lanes): constant rows, a maximum at several indices, a maximum only at the last index. The
    labels sit on each tied index in turn, so a wrong winner changes the count."""
    gen = torch.Generator().manual_seed(Cl)
    if at is None:
        z = torch.full((B, Cl), 0.25)
        cand = [0, 1, Cl - 1]
    else:
        z = torch.randn(B, Cl, generator=gen).clamp_(-3, 3)
        z[:, list(at)] = 5.0
        cand = list(at) + [0]
    y = torch.tensor([cand[r % len(cand)] for r in range(B)])
    want = int((torch.from_numpy(_argmax_lowest(z)) == y).sum().item())
    assert 0 < want < B or len(cand) == 1
    z, y = z.cuda(), y.cuda()
    acc = torch.zeros(3, device="cuda")
    C.ce_fwd(z, y, -100, 0.0, True, acc)
    assert acc[1].item() == want and acc[2].item() == B
    acc = torch.zeros(3, device="cuda")
    C.count_correct(z, y, acc)
    assert acc[0].item() == 0 and acc[1].item() == want and acc[2].item() == B


@pytest.mark.parametrize("B,Cl", [(16, 10), (300, 10), (6, 100)])
def test_ce_all_rows_ignored(C, B, Cl):
    """Every row ignored under 'mean': the loss is NaN as in torch; the fused gradient and ce_bwd
    are all zeros (no inf * 0); acc is unchanged."""
    z = torch.randn(B, Cl, device="cuda")
    y = torch.full((B,), -100, device="cuda")
    assert math.isnan(F.cross_entropy(z, y).item())
    acc = torch.tensor([1.5, 2.0, 3.0], device="cuda")
    loss, lse, d = C.ce_fwd(z, y, -100, 0.1, True, acc, with_grad=True)
    assert math.isnan(loss.item()) and lse[B].item() == 0
    assert torch.equal(d, torch.zeros_like(d))
    assert acc.tolist() == [1.5, 2.0, 3.0]
    for gout in (1.0, 0.5):
        d2 = C.ce_bwd(z, y, lse, torch.full((1,), gout, device="cuda"), -100, 0.1, True)
        assert torch.equal(d2, torch.zeros_like(d2))
    assert C.ce_fwd(z, y, -100, 0.0, False, None)[0].item() == 0.0  # 'sum' of nothing


@pytest.mark.parametrize("B,Cl", [(16, 10), (300, 10), (6, 100), (1, 10), (1, 100)])
def test_ce_one_valid_row(C, B, Cl):
    """Exactly one valid row (and B = 1): the mean's denominator is 1. Measured: loss e_k = e_t =
    6.5e-9 at scale 4.5 (c = 4); dlogits e_k 4.4e-8 / e_t 1.5e-8 (c = 2)."""
    gen = torch.Generator().manual_seed(B + Cl)
    z = (torch.randn(B, Cl, generator=gen) * 3).cuda()
    y = torch.full((B,), -100)
    y[B // 3] = int(torch.randint(0, Cl, (1,), generator=gen))
    y = y.cuda()
    for eps in (0.0, 0.1):
        out = _check_ce(C, z, y, eps, "mean", f"one-valid[{B}x{Cl} eps={eps}]")
        assert out[1][B].item() == 1


@pytest.mark.parametrize("B,Cl", [(64, 10), (300, 10), (6, 100)])
def test_ce_row_stride(C, B, Cl):
    """Logits as a [:, :C] view of a wider buffer (ld > C; the padding holds 1e30, so a misread
    shows): every output equals the contiguous call's bit for bit. ops.cross_entropy takes a
    transposed (inner stride != 1) tensor."""
    from tutorial_torch_distributed_data_parallel_amd import ops

    gen = torch.Generator().manual_seed(B * Cl)
    buf = torch.full((B, Cl + 7), 1e30)
    buf[:, :Cl] = torch.randn(B, Cl, generator=gen) * 3
    buf = buf.cuda()
    view, z = buf[:, :Cl], buf[:, :Cl].contiguous()
    assert view.stride(0) == Cl + 7
    y = _labels(B, Cl, gen, ignore_row=1)
    a1, a2 = torch.zeros(3, device="cuda"), torch.zeros(3, device="cuda")
    o1 = C.ce_fwd(view, y, -100, 0.1, True, a1, with_grad=True)
    o2 = C.ce_fwd(z, y, -100, 0.1, True, a2, with_grad=True)
    assert all(torch.equal(p, q) for p, q in zip(o1, o2)) and torch.equal(a1, a2)
    g = torch.full((1,), 0.5, device="cuda")
    assert torch.equal(C.ce_bwd(view, y, o1[1], g, -100, 0.1, True),
                       C.ce_bwd(z, y, o2[1], g, -100, 0.1, True))
    c1, c2 = torch.zeros(3, device="cuda"), torch.zeros(3, device="cuda")
    C.count_correct(view, y.clamp(min=0), c1)
    C.count_correct(z, y.clamp(min=0), c2)
    assert torch.equal(c1, c2) and c1[2].item() == B
    zt = z.t().contiguous().t().requires_grad_()  # [B, C] with strides (1, B)
    assert zt.stride(1) != 1
    loss = ops.cross_entropy(zt, y, label_smoothing=0.1)
    loss.backward()
    assert torch.equal(loss.detach(), o2[0]) and torch.equal(zt.grad, o2[2])


# ----------------------------------------------------------------------------------- max-pool
POOL_FAMILIES = {"nchw": (3, torch.contiguous_format), "nhwc": (5, torch.channels_last),
                 "nhwc4": (64, torch.channels_last)}
POOL_CFGS = [(3, 2, 0, 13, 14), (3, 2, 1, 12, 11), (2, 2, 0, 8, 8), (3, 1, 1, 6, 7)]


def _pool_input(kind, Cn, k, p, H, W, gen):
    if kind == "ties":  # relu outputs quantised to {0, 0.5, 1}: every window ties, many at 0
        return torch.randint(0, 3, (2, Cn, H, W), generator=gen) * 0.5
    if kind == "negative":  # padding must behave as -inf, not as 0
        return -torch.rand(2, Cn, H, W, generator=gen) - 1
    x = torch.randn(2, Cn, H, W, generator=gen)
    if kind == "ninf":
        x[torch.rand(x.shape, generator=gen) < 0.2] = -math.inf
        x[0, :, :k - p, :k - p] = -math.inf  # output (0, 0) of image 0: a fully -inf window
    elif kind == "nan":
        x[:, :, ::4, ::4] = math.nan
    return x


@pytest.mark.parametrize("kind", ["ties", "negative", "ninf", "nan"])
@pytest.mark.parametrize("k,s,p,H,W", POOL_CFGS)
@pytest.mark.parametrize("family", list(POOL_FAMILIES))
def test_maxpool_hard_inputs(family, k, s, p, H, W, kind):
    """The three forward kernels' "first maximum wins; a NaN wins and then sticks" rule and the
    backward's argmax routing against F.max_pool2d in float64 on the CPU: exact forward, backward
    within 1e-6 (the upstream gradient is a multiple of 1/4, so sums over overlapping windows are
    exact and only the routing can differ)."""
    from tutorial_torch_distributed_data_parallel_amd import ops

    Cn, fmt = POOL_FAMILIES[family]
    gen = torch.Generator().manual_seed(H * 100 + W + k)
    x = _pool_input(kind, Cn, k, p, H, W, gen)
    if kind == "nan":  # at most one NaN per window: torch keeps the last of several, we the first
        per = F.unfold(x.isnan().double(), k, padding=p, stride=s).view(2, Cn, k * k, -1).sum(2)
        assert per.max().item() == 1
    xr = x.double().requires_grad_()
    yr = F.max_pool2d(xr, k, s, p)
    dy = torch.randint(-8, 9, yr.shape, generator=gen) * 0.25
    yr.backward(dy.double())
    xg = x.cuda().contiguous(memory_format=fmt).requires_grad_()
    y = ops.max_pool2d(xg, k, s, p)
    y.backward(dy.cuda())
    yc, nan = y.detach().cpu().double(), yr.detach().isnan()
    assert torch.equal(yc.isnan(), nan)
    assert torch.equal(yc[~nan], yr.detach()[~nan])
    if kind == "ninf":
        assert (yc[0, :, 0, 0] == -math.inf).all()
        if s > p:  # no other window holds input (0, 0): it gets exactly that window's dy
            assert torch.equal(xg.grad[0, :, 0, 0].cpu(), dy[0, :, 0, 0])
    if kind == "nan":
        assert nan.any()
    torch.testing.assert_close(xg.grad.cpu().double(), xr.grad, rtol=0, atol=1e-6)


# ---------------------------------------------------------------------------------- BatchNorm
OFFSETS = (0.0, 10.0, 1e3, -1e4)
STDS = (1.0, 0.1)


def _bn_input(shape, gen):
    """x[:, c] = offset_c + std_c * randn: offsets cycle through OFFSETS, std through STDS."""
    Cn = shape[1]
    off = torch.tensor([OFFSETS[c % 4] for c in range(Cn)])
    std = torch.tensor([STDS[c % 2] for c in range(Cn)])
    view = (1, Cn) + (1,) * (len(shape) - 2)
    return (torch.randn(shape, generator=gen) * std.view(view) + off.view(view)).cuda()


def _mean_scale(off, std):
    """ulp(offset) / 2**-24, the granularity of an fp32 mean near the offset (the spread's own
    magnitude for the channels centred on 0)."""
    return max(2.0 ** (math.floor(math.log2(abs(off))) + 1) if off else 0.0, std)


def _rule_moments(tag, mean, var, x, dims, tmean=None, tvar=None):
    """Mean / variance of one kind of channel at a time (the four (offset, std) classes), each
    with its own scale: std**2 for the variance, ulp(offset) / 2**-24 for the mean."""
    xd = x.double().cpu()
    v64, m64 = torch.var_mean(xd, dims, correction=0)
    if tmean is None:
        tvar, tmean = torch.var_mean(x, dims, correction=0)
    for k in range(4):
        off, std = OFFSETS[k], STDS[k % 2]
        sel = slice(k, None, 4)
        if m64[sel].numel() == 0:
            continue
        _rule(f"{tag} mean[off={off:g} std={std}]", mean[sel], tmean[sel], m64[sel], C_["mean"],
              _mean_scale(off, std))
        _rule(f"{tag} var[off={off:g} std={std}]", var[sel], tvar[sel], v64[sel], C_["var"],
              std * std)


BN_MOMENT_SHAPES = [((77, 12), False), ((300, 64), False), ((8, 16, 33), False),
                    ((4, 64, 7, 7), False), ((4, 64, 7, 7), True)]


@pytest.mark.parametrize("shape,nhwc", BN_MOMENT_SHAPES)
def test_bn_moments_large_mean(C, shape, nhwc):
    """C.bn_moments (moments_rows4 / moments_1d / moments_2d, and the [pixels, C] rows of a
    channels_last tensor) on channels with a large mean and a small spread, against float64; e_t
    is torch.var_mean in fp32 on the GPU. A sum / sum-of-squares variance misses this by orders of
    magnitude: at offset -1e4, std 0.1 it loses every digit.

    Measured, worst class: mean e_k 2.7e-8 / e_t 1.2e-8 at scale 1 (offset 0), c = 2; variance
    e_k 9.9e-8 / e_t 9.6e-8 at scale 1, c = 2."""
    gen = torch.Generator().manual_seed(sum(shape) + nhwc)
    x = _bn_input(shape, gen)
    Cn = shape[1]
    dims = [0] + list(range(2, x.dim()))
    rows = x.permute(0, 2, 3, 1).reshape(-1, Cn).contiguous() if nhwc else x
    st = C.bn_moments(rows)[0]
    assert st[2 * Cn].item() == x.numel() // Cn
    _rule_moments(f"bn_moments{shape}{' nhwc' if nhwc else ''}", st[:Cn], st[Cn:2 * Cn], x, dims)


def _bn_ref(x, w, b, dy, dtype, dev, relu=False, eps=1e-5):
    """(y, dx, dw, db, running_mean, running_var, save_mean, save_invstd) of torch's batch norm."""
    xs, ws, bs = (t.detach().to(device=dev, dtype=dtype).requires_grad_() for t in (x, w, b))
    Cn = x.shape[1]
    rm = torch.zeros(Cn, dtype=dtype, device=dev)
    rv = torch.ones(Cn, dtype=dtype, device=dev)
    y = F.batch_norm(xs, rm, rv, ws, bs, True, 0.1, eps)
    if relu:
        y = F.relu(y)
    gx, gw, gb = torch.autograd.grad(y, (xs, ws, bs), dy.to(device=dev, dtype=dtype))
    dims = [0] + list(range(2, x.dim()))
    with torch.no_grad():
        var, mean = torch.var_mean(xs, dims, correction=0)
        invstd = torch.rsqrt(var + eps)
    return y.detach(), gx, gw, gb, rm, rv, mean, invstd


@pytest.mark.parametrize("N,Cn", [(128, 64), (77, 16)])
def test_bn1d_local_large_mean(C, N, Cn):
    """The one-launch BatchNorm1d forward / backward (bn1d_local_fwd / bn1d_local_bwd) on
    large-mean channels: saved mean and invstd, running statistics, y, dx, dw, db by the rule.
    y and dx carry the ulp(offset) / std error of an fp32 mean in both implementations.

    Measured at (128,64): y e_k 8.8e-3 / e_t 1.7e-2 at scale 5.9; dx 2.4e-2 / 6.4e-2 at scale 52;
    dw 9.4e-2 / 1.7e-1; invstd 2.5e-4 / 9.5e-3; variance 2.3e-7 / 1.6e-7 (std 1); c = 2 each."""
    gen = torch.Generator().manual_seed(N + Cn)
    x = _bn_input((N, Cn), gen)
    w = (torch.rand(Cn, generator=gen) + 0.5).cuda()
    b = torch.randn(Cn, generator=gen).cuda()
    dy = torch.randn(N, Cn, generator=gen).cuda()
    rm, rv = torch.zeros(Cn, device="cuda"), torch.ones(Cn, device="cuda")
    r = C.bn1d_local_fwd(x, w, b, False, 1e-5, 0.1, rmean=rm, rvar=rv)
    assert r, "bn1d_local_fwd takes N <= 512 rows, C % 16 == 0"
    y, stats = r
    dw, db = torch.empty(Cn, device="cuda"), torch.empty(Cn, device="cuda")
    dx = C.bn1d_local_bwd(dy, x, stats, w, dw=dw, db=db)
    assert dx is not None
    r64 = _bn_ref(x, w, b, dy, torch.float64, "cpu")
    r32 = _bn_ref(x, w, b, dy, torch.float32, "cuda")
    tag = f"bn1d_local[{N}x{Cn}]"
    assert stats[2 * Cn].item() == N
    got_var = 1.0 / stats[Cn:2 * Cn].double() ** 2 - 1e-5
    t_var = 1.0 / r32[7].double() ** 2 - 1e-5
    _rule_moments(tag, stats[:Cn], got_var, x, [0], r32[6], t_var)
    _rule(f"{tag} invstd", stats[Cn:2 * Cn], r32[7], r64[7], C_["var"])
    _rule(f"{tag} running_mean", rm, r32[4], r64[4], C_["mean"])
    _rule(f"{tag} running_var", rv, r32[5], r64[5], C_["var"])
    _rule(f"{tag} y", y, r32[0], r64[0], C_["bn_y"])
    _rule(f"{tag} dx", dx, r32[1], r64[1], C_["bn_dx"])
    _rule(f"{tag} dw", dw, r32[2], r64[2], C_["bn_dx"])
    _rule(f"{tag} db", db, r32[3], r64[3], C_["bn_dx"])


def _module_bn(x, w, b, dy, relu=False):
    """(y, dx, dw, db, running_mean, running_var) of the package's BatchNorm module."""
    import tutorial_torch_distributed_data_parallel_amd as tdp

    cls = tdp.nn.BatchNorm2d if x.dim() == 4 else tdp.nn.BatchNorm1d
    m = cls(x.shape[1], relu=relu, device="cuda")
    with torch.no_grad():
        m.weight.copy_(w)
        m.bias.copy_(b)
    xs = x.detach().clone(memory_format=torch.preserve_format).requires_grad_()
    y = m(xs)
    y.backward(dy)
    return y.detach(), xs.grad, m.weight.grad, m.bias.grad, m.running_mean, m.running_var, m


BN_MODULE_SHAPES = [((128, 64), False), ((77, 16), False), ((77, 12), False), ((50, 18), False),
                    ((4, 64, 7, 7), False), ((4, 64, 7, 7), True)]


@pytest.mark.parametrize("shape,nhwc", BN_MODULE_SHAPES)
def test_bn_module_large_mean(shape, nhwc):
    """nn.BatchNorm1d / nn.BatchNorm2d forward and backward on large-mean channels (C = 12 and
    C = 18: the 1-D paths for a channel count that is no multiple of 16 / of 4): y, dx, dw, db
    and the running statistics by the rule.

    Measured at (50,18): y e_k 9.4e-3 / e_t 1.1e-2 at scale 4.9; dx 7.6e-2 / 4.9e-2 at scale 37;
    dw 5.2e-2 / 2.9e-2; running_var 3.5e-6 / 2.9e-6; c = 2 each. (torch's own fp32 result on the
    channels_last case is far off: y e_t 1.3e+2 against e_k 1.5e-2.)"""
    gen = torch.Generator().manual_seed(sum(shape) + 2 * nhwc)
    x = _bn_input(shape, gen)
    Cn = shape[1]
    w = (torch.rand(Cn, generator=gen) + 0.5).cuda()
    b = torch.randn(Cn, generator=gen).cuda()
    dy = torch.randn(shape, generator=gen).cuda()
    if nhwc:
        x = x.contiguous(memory_format=torch.channels_last)
        dy = dy.contiguous(memory_format=torch.channels_last)
    got = _module_bn(x, w, b, dy)
    r64 = _bn_ref(x, w, b, dy, torch.float64, "cpu")
    r32 = _bn_ref(x, w, b, dy, torch.float32, "cuda")
    tag = f"bn_module{shape}{' nhwc' if nhwc else ''}"
    for i, (name, c) in enumerate((("y", "bn_y"), ("dx", "bn_dx"), ("dw", "bn_dx"),
                                   ("db", "bn_dx"), ("running_mean", "mean"),
                                   ("running_var", "var"))):
        _rule(f"{tag} {name}", got[i], r32[i], r64[i], C_[c])
    assert got[6].num_batches_tracked.item() == 1


@pytest.mark.parametrize("shape,nhwc", [((128, 64), False), ((77, 12), False),
                                        ((4, 64, 7, 7), True)])
def test_bn_constant_channel(C, shape, nhwc):
    """A constant channel (and a constant channel at a large value): the variance is exactly 0
    (Welford's deviations are all 0), y == relu(bias) exactly (the normalisation centres x before
    it scales: x * scale + shift with the mean folded into the shift misses the bias by
    ulp(mean * scale)), dx is finite and follows the rule.

    Measured: dx e_k 2.6e-5 / e_t 2.6e-5 at scale 515; y e_k 6.9e-7 / e_t 7.2e-7; c = 2."""
    gen = torch.Generator().manual_seed(sum(shape))
    Cn = shape[1]
    x = torch.randn(shape, generator=gen)
    x[:, 1] = 3.7
    x[:, 6] = -12345.678
    x = x.cuda()
    w = (torch.rand(Cn, generator=gen) + 0.5).cuda()
    b = torch.randn(Cn, generator=gen).cuda()
    b[1], b[6] = 0.75, -0.5
    dy = torch.randn(shape, generator=gen).cuda()
    rows = x.permute(0, 2, 3, 1).reshape(-1, Cn).contiguous() if nhwc else x
    st = C.bn_moments(rows)[0]
    assert st[Cn + 1].item() == 0.0 and st[Cn + 6].item() == 0.0
    assert st[1].item() == x[0, 1].flatten()[0].item() and st[6].item() == x[0, 6].flatten()[0].item()
    if nhwc:
        x = x.contiguous(memory_format=torch.channels_last)
        dy = dy.contiguous(memory_format=torch.channels_last)
    got = _module_bn(x, w, b, dy, relu=True)
    assert (got[0][:, 1] == 0.75).all() and (got[0][:, 6] == 0.0).all()
    r64 = _bn_ref(x, w, b, dy, torch.float64, "cpu", relu=True)
    r32 = _bn_ref(x, w, b, dy, torch.float32, "cuda", relu=True)
    assert torch.isfinite(got[1]).all()
    tag = f"bn_const{shape}"
    _rule(f"{tag} dx", got[1], r32[1], r64[1], C_["bn_dx"])
    _rule(f"{tag} dx[const channel]", got[1][:, 1], r32[1][:, 1], r64[1][:, 1], C_["bn_dx"])
    _rule(f"{tag} y", got[0], r32[0], r64[0], C_["bn_y"])


@pytest.mark.parametrize("Cn", [16, 12, 18])
def test_bn_tiny_batches(Cn):
    """One sample per channel in eval mode (the running statistics normalise it) and N = 2 in
    training mode (the unbiased running variance divides by N - 1 = 1).

    Measured: eval y e_k = e_t = 6.9e-8 at scale 3.0; N = 2 y e_k = e_t = 1.1e-2 at scale 2.0, dx
    e_k 8.0 / e_t 7.9 at scale 17 (two samples 0.1 apart at -1e4: both lose the spread), running
    variance 4.6e-8 / 4.8e-8; c = 2 each."""
    import tutorial_torch_distributed_data_parallel_amd as tdp

    gen = torch.Generator().manual_seed(Cn)
    w = (torch.rand(Cn, generator=gen) + 0.5).cuda()
    b = torch.randn(Cn, generator=gen).cuda()
    x1 = _bn_input((1, Cn), gen)
    rm = torch.tensor([OFFSETS[c % 4] for c in range(Cn)]).cuda()
    rv = torch.tensor([STDS[c % 2] ** 2 for c in range(Cn)]).cuda()
    m = tdp.nn.BatchNorm1d(Cn, device="cuda").eval()
    with torch.no_grad():
        m.weight.copy_(w)
        m.bias.copy_(b)
        m.running_mean.copy_(rm)
        m.running_var.copy_(rv)
        y = m(x1)
    t32 = F.batch_norm(x1, rm, rv, w, b, False, 0.0, 1e-5)
    r64 = F.batch_norm(*(t.double().cpu() for t in (x1, rm, rv, w, b)), False, 0.0, 1e-5)
    _rule(f"bn_eval[1x{Cn}] y", y, t32, r64, C_["bn_y"])
    assert torch.equal(m.running_mean, rm) and torch.equal(m.running_var, rv)
    x2 = _bn_input((2, Cn), gen)
    dy = torch.randn(2, Cn, generator=gen).cuda()
    got = _module_bn(x2, w, b, dy)
    r64 = _bn_ref(x2, w, b, dy, torch.float64, "cpu")
    r32 = _bn_ref(x2, w, b, dy, torch.float32, "cuda")
    for i, (name, c) in enumerate((("y", "bn_y"), ("dx", "bn_dx"), ("dw", "bn_dx"),
                                   ("db", "bn_dx"), ("running_mean", "mean"),
                                   ("running_var", "var"))):
        _rule(f"bn_train[2x{Cn}] {name}", got[i], r32[i], r64[i], C_[c])


# ------------------------------------------------------------- conv-epilogue BatchNorm statistics
def _conv_with_stats(C, x, w, st, R):
    from tutorial_torch_distributed_data_parallel_amd import ops

    C.gemm_f32_set_override(0, 1, 0)  # unsplit: small test shapes would plan split-K
    try:
        y = ops.conv2d(x, w, None, st, R // 2, bn_stats=True)
    finally:
        C.gemm_f32_set_override(0, 0, 0)
    tag = getattr(y, "_tdp_bn_part", None)
    assert tag is not None, "an unsplit forward plan must emit statistics"
    Cout = y.shape[1]
    rows = y.permute(0, 2, 3, 1).reshape(-1, Cout)
    got = C.bn_moments_partials(tag[0], float(rows.shape[0]))
    welford = C.bn_moments(rows)[0]
    v64, m64 = torch.var_mean(rows.double().cpu(), 0, correction=0)
    assert got[2 * Cout].item() == rows.shape[0]
    return got[:Cout], got[Cout:2 * Cout], welford[:Cout], welford[Cout:2 * Cout], m64, v64


EPI_SHAPES = [(2, 4, 33, 29, 64, 7, 2), (3, 128, 9, 9, 512, 1, 1)]
# measured max error (mean, variance) of the merged epilogue statistics with an outlier in the
# shift row, MI355X; test_conv_epilogue_stats_outlier_shift_row allows twice these
EPI_OUTLIER_PINS = {EPI_SHAPES[0]: (4.879e-4, 9.381), EPI_SHAPES[1]: (1.694e-3, 78.53)}


def _epi_operands(shape, gen):
    B, Cin, H, W, Cout, R, st = shape
    x = (5 + 0.01 * torch.randn(B, Cin, H, W, generator=gen)).cuda().contiguous(
        memory_format=torch.channels_last)
    w = (torch.randn(Cout, Cin, R, R, generator=gen).abs() * 0.2).cuda().contiguous(
        memory_format=torch.channels_last)
    return x, w


@pytest.mark.parametrize("shape", EPI_SHAPES)
def test_conv_epilogue_stats_large_mean(C, shape):
    """The forward GEMM epilogue's shifted one-pass statistics on an output with a large mean and
    a small spread (x = 5 + 0.01 randn, positive weights): the merged mean and variance follow the
    rule against the float64 moments of the stored output; e_t is the Welford pass (C.bn_moments)
    over the same output.

    Measured: mean e_k 1.4e-5 / e_t 1.5e-5 at scale 148; variance e_k 5.3e-4 / e_t 1.3e-4 at scale
    1072 (needs c = 0.02) for the 7x7 stem, 1.4e-8 / 5.4e-8 for the 1x1; c = 2."""
    gen = torch.Generator().manual_seed(shape[2])
    x, w = _epi_operands(shape, gen)
    mean, var, wmean, wvar, m64, v64 = _conv_with_stats(C, x, w, shape[6], shape[5])
    _rule(f"epilogue{shape} mean", mean, wmean, m64, C_["mean"])
    _rule(f"epilogue{shape} var", var, wvar, v64, C_["var"])


@pytest.mark.parametrize("shape", EPI_SHAPES)
def test_conv_epilogue_stats_outlier_shift_row(C, shape):
    """The shift of the one-pass sums is the tile's first row. +1e3 on the input pixels behind
    output pixel 0 of the first image puts that row far from the rest of tile 0 (the kernel's
    precondition "the tile's first row within O(std) of the tile mean" is violated). The merged
    statistics then miss the rule, so the measured error is pinned with a margin of 2x (a
    documented bound: docs/PARITY.md "numerical edge contracts", as
    test_emu_subnormal_operands_documented_bound does for the GEMM)."""
    gen = torch.Generator().manual_seed(shape[2] + 1)
    x, w = _epi_operands(shape, gen)
    R = shape[5]
    x[0, :, :R - R // 2, :R - R // 2] += 1e3
    mean, var, wmean, wvar, m64, v64 = _conv_with_stats(C, x, w, shape[6], R)
    fm = _figures(f"epilogue-outlier{shape} mean", mean, wmean, m64, C_["mean"])
    fv = _figures(f"epilogue-outlier{shape} var", var, wvar, v64, C_["var"])
    pin_mean, pin_var = EPI_OUTLIER_PINS[shape]
    assert fm[0] <= 2 * pin_mean and fv[0] <= 2 * pin_var
