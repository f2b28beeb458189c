"""Cross-entropy against class-probability targets (csrc/loss_soft.hip), dense and pair form,
against ``F.cross_entropy`` in float64 on the CPU from the same fp32 inputs, by the rule of
tests/test_hard_inputs_gpu.py: e_k <= 4 e_t + c 2^-24 scale, e_t being ``F.cross_entropy`` in fp32
on the GPU with the dense target; c = 4 for a loss (scale max|loss_f64|), c = 2 for B * dlogits
(scale 1; the plain gradient for reduction="sum").

test_numerics[dense-*] is the test that fails without the feature: before it, a ``[B, C]``
probability target was cast to int64 and refused (or misread) by the index-target kernel."""
import pytest
import torch
import torch.nn.functional as F

import tutorial_torch_distributed_data_parallel_amd as tdp
from tutorial_torch_distributed_data_parallel_amd.ops.loss import pair_target

pytestmark = pytest.mark.gpu

U = 2.0 ** -24
# (B, C): idle lanes + scalar | odd C, unaligned rows | 16-byte path, ragged B | the workload's
# row | the register cap | the re-read path
SHAPES = [(1, 5), (3, 33), (5, 68), (4, 1000), (2, 4096), (3, 4100)]
CASES = [(s, eps, red) for s in SHAPES for eps in (0.0, 0.1) for red in ("mean", "sum")]
IDS = [f"{b}x{c}-eps{eps}-{red}" for (b, c), eps, red in CASES]


def _rule(what, got, t32, ref, c, scale=None):
    got, t32, ref = (v.detach().double().cpu() for v in (got, t32, ref))
    e_k, e_t = (got - ref).abs().max().item(), (t32 - ref).abs().max().item()
    scale = ref.abs().max().item() if scale is None else scale
    print(f"[rule] {what}: e_k={e_k:.3e} e_t={e_t:.3e} c={c} scale={scale:.3e}")
    assert e_k <= 4 * e_t + c * U * scale, f"{what}: e_k {e_k:.3e}, e_t {e_t:.3e}, scale {scale:.3e}"


def _ref(fn, z, dtype, dev):
    """(loss, dlogits, summed loss) of ``fn(logits)`` -> (loss, total) in ``dtype`` on ``dev``."""
    zz = z.detach().to(device=dev, dtype=dtype).requires_grad_()
    loss, total = fn(zz)
    return loss.detach(), torch.autograd.grad(loss, zz)[0], total.detach()


def _dense_ref(t, eps, red):
    def fn(zz):
        tt = t.to(device=zz.device, dtype=zz.dtype)
        return (F.cross_entropy(zz, tt, label_smoothing=eps, reduction=red),
                F.cross_entropy(zz, tt, label_smoothing=eps, reduction="sum"))
    return fn


def _check(z, run, ref_fn, red, targ, tag):
    """Loss, gradient (unit seed, autograd's own seed, a non-unit seed) and acc of ``run(logits,
    acc)`` against ``ref_fn`` in float64."""
    B = z.shape[0]
    r64, r32 = _ref(ref_fn, z, torch.float64, "cpu"), _ref(ref_fn, z, torch.float32, "cuda")
    gs = float(B) if red == "mean" else 1.0
    grads = []
    for seed in ("unit", "plain", 0.25):
        zk = z.detach().requires_grad_()
        acc = torch.tensor([0.0, 5.0, 7.0], device="cuda")
        loss = run(zk, acc)
        if seed == "unit":
            tdp.ops.backward(loss)
        elif seed == "plain":
            loss.backward()
        else:
            loss.backward(torch.tensor(seed, device="cuda"))
        grads.append(zk.grad)
    _rule(f"{tag} loss", loss, r32[0], r64[0], 4)
    _rule(f"{tag} grad", grads[0] * gs, r32[1] * gs, r64[1] * gs, 2, 1.0)
    assert torch.equal(grads[1], grads[0])
    assert torch.equal(grads[2], grads[0] * 0.25)  # a power of two: the scale kernel is exact
    _rule(f"{tag} acc[0]", acc[0], r32[2], r64[2], 4)
    assert acc[1].item() == 5 + int((z.argmax(1) == targ).sum()) and acc[2].item() == 7 + B


def _pair(B, C, gen):
    ya, yb = (torch.randint(0, C, (B,), generator=gen).cuda() for _ in range(2))
    yb[-1] = ya[-1]
    lam = torch.rand(B, generator=gen)
    lam[:3] = torch.tensor([0.0, 1.0, 0.5])[:B]  # one label only, the other only, the argmax tie
    return ya, yb, lam.cuda()


@pytest.mark.parametrize("shape,eps,red", CASES, ids=IDS)
@pytest.mark.parametrize("form", ["dense", "pair"])
def test_numerics(form, shape, eps, red):
    B, C = shape
    gen = torch.Generator().manual_seed(B * 10007 + C)
    z = (torch.randn(B, C, generator=gen) * 2).cuda()
    if form == "dense":
        t = torch.softmax(torch.randn(B, C, generator=gen) * 3, 1)
        if shape == (5, 68):  # rows that do not sum to 1
            t = t * torch.linspace(0.5, 1.5, B).view(B, 1)
        t = t.cuda()
        _check(z, lambda zk, acc: tdp.ops.cross_entropy(zk, t, label_smoothing=eps,
                                                        reduction=red, acc=acc),
               _dense_ref(t, eps, red), red, t.argmax(1), f"dense{shape}")
    else:
        ya, yb, lam = _pair(B, C, gen)

        def ref_fn(zz):  # the dense target in the reference's own precision, from the fp32 lam
            return _dense_ref(pair_target(ya.to(zz.device), yb.to(zz.device),
                                          lam.to(device=zz.device, dtype=zz.dtype), C),
                              eps, red)(zz)
        _check(z, lambda zk, acc: tdp.ops.cross_entropy_pair(zk, ya, yb, lam, eps, red, acc),
               ref_fn, red, torch.where(lam >= 0.5, ya, yb), f"pair{shape}")


@pytest.mark.parametrize("kind", ["scale1000", "stride3", "stride4", "neginf"])
def test_hard_rows(kind):
    B, C = 5, 68
    gen = torch.Generator().manual_seed(7)
    z = torch.randn(B, 100, generator=gen).cuda()
    t = torch.softmax(torch.randn(B, C, generator=gen), 1).cuda()
    if kind == "neginf":  # pair form, eps = 0: an unnamed class at -inf costs nothing
        ya, yb, lam = _pair(B, C, gen)
        free = [c for c in range(C) if c not in ya.tolist() + yb.tolist()][0]
        z = z[:, :C].contiguous()
        z[:, free] = float("-inf")

        def ref_fn(zz):  # 0 * -inf is NaN in the dense composition: the index form's mixture
            la = lam.to(device=zz.device, dtype=zz.dtype)
            rows = (la * F.cross_entropy(zz, ya.to(zz.device), reduction="none") +
                    (1 - la) * F.cross_entropy(zz, yb.to(zz.device), reduction="none"))
            return rows.mean(), rows.sum()
        zk = z.detach().requires_grad_()
        loss = tdp.ops.cross_entropy_pair(zk, ya, yb, lam)
        loss.backward()
        assert torch.isfinite(loss) and bool((zk.grad[:, free] == 0).all())
        _check(z, lambda zk, acc: tdp.ops.cross_entropy_pair(zk, ya, yb, lam, acc=acc), ref_fn,
               "mean", torch.where(lam >= 0.5, ya, yb), kind)
        return
    if kind == "scale1000":  # the lse residual
        z = z[:, :C].contiguous() * 1000
    else:  # a column slice of a wider tensor: row stride 100 > C, base unaligned / aligned
        off = int(kind[-1])
        z = z[:, off:off + C]
    _check(z, lambda zk, acc: tdp.ops.cross_entropy(zk, t, label_smoothing=0.1, acc=acc),
           _dense_ref(t, 0.1, "mean"), "mean", t.argmax(1), kind)


@pytest.mark.parametrize("form", ["dense", "pair"])
@pytest.mark.parametrize("shape", [(3, 33), (5, 68), (3, 4100)])
def test_bitwise(form, shape):
    """Two runs agree bitwise, and row r of a batch is bitwise that row run alone (loss term and
    gradient, reduction="sum") -- the lone row at a 4-byte aligned address, so for (5, 68) the
    batch takes 16-byte loads and the lone row 4-byte loads."""
    C_ = tdp._native.native()
    B, C = shape
    gen = torch.Generator().manual_seed(3)
    z = torch.randn(B, C, generator=gen).cuda()
    t = torch.softmax(torch.randn(B, C, generator=gen), 1).cuda()
    ya, yb, lam = _pair(B, C, gen)

    def run(zz, rows):
        if form == "dense":
            return C_.soft_ce_fwd(zz, target=t[rows], smoothing=0.1, mean=False, with_grad=True)
        return C_.soft_ce_fwd(zz, ya=ya[rows], yb=yb[rows], lam=lam[rows], smoothing=0.1,
                              mean=False, with_grad=True)
    every = slice(0, B)
    first, second = run(z, every), run(z, every)
    assert all(torch.equal(a, b) for a, b in zip(first, second))
    for r in range(B):
        lone = torch.empty(C + 1, device="cuda")[1:].view(1, C).copy_(z[r:r + 1])
        _, rows, d = run(lone, slice(r, r + 1))
        assert rows[0, 0] == first[1][0, r] and torch.equal(d[0], first[2][r])
