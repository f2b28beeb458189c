"""ReLU6 in the BatchNorm kernels, the stand-alone ReLU6 and MobileNetV2 on the GPU.

ReLU6 contracts are bitwise: ``bn(x, relu6) == clamp(bn(x, relu), max=6)`` with identical running
statistics, and the backward under ReLU6 equals the ReLU form's backward fed ``dy * (y_relu < 6)``
(both kernels then see the same gated dy in the same order). Against a float64 twin of the same
fp32 inputs everything follows the rule of tests/test_hard_inputs_gpu.py,
``e_k <= 4 e_t + c 2^-24 scale`` with that file's c = 2 for BatchNorm outputs and gradients and
e_t the error of torch's own fp32 result on the GPU."""
import copy

import pytest
import torch
import torch.nn.functional as F

import tutorial_torch_distributed_data_parallel_amd as tdp
from tutorial_torch_distributed_data_parallel_amd import ops
from tutorial_torch_distributed_data_parallel_amd.models.mobilenet import (InvertedResidual,
                                                                            mobilenet_v2)

from mobilenet_twin import (TwinInvertedResidual, TwinMobileNetV2, U, check_grads_rule,
                            check_rule)

pytestmark = pytest.mark.gpu
CL = torch.channels_last
C_BN = 2  # tests/test_hard_inputs_gpu.py C_["bn_y"] and C_["bn_dx"]


# ------------------------------------------------------------------------- BatchNorm + ReLU6
def _inputs(shape, nhwc, residual):
    g = torch.Generator().manual_seed(3)  # every case has > 13 % of its outputs in each region
    Cn = shape[1]
    x = torch.randn(shape, generator=g)
    w = torch.empty(Cn).uniform_(2, 4, generator=g)  # a real share of outputs in each region
    b = torch.empty(Cn).uniform_(1, 4, generator=g)
    dy = torch.randn(shape, generator=g)
    res = torch.randn(shape, generator=g) if residual else None
    return x, w, b, dy, res, nhwc


def _dev(t, nhwc, dtype=torch.float32, dev="cuda"):
    t = t.to(device=dev, dtype=dtype)
    return t.contiguous(memory_format=CL) if (nhwc and t.dim() == 4) else t


def _ours(inp, act, dy=None, training=True):
    """ops.batch_norm on the GPU with activation ``act`` (1 ReLU, 2 ReLU6): y, grads, stats."""
    x, w, b, dy0, res, nhwc = inp
    dy = dy0 if dy is None else dy
    Cn = x.shape[1]
    lv = [_dev(t, nhwc).requires_grad_(training) for t in (x, w, b)]
    r = _dev(res, nhwc).requires_grad_(training) if res is not None else None
    rm = torch.zeros(Cn, device="cuda") if training else torch.full((Cn,), 0.1, device="cuda")
    rv = torch.ones(Cn, device="cuda") if training else torch.full((Cn,), 0.8, device="cuda")
    with torch.set_grad_enabled(training):
        y = ops.batch_norm(lv[0], rm, rv, lv[1], lv[2], training=training, relu=act == 1,
                           relu6=act == 2, residual=r)
    grads = None
    if training:
        y.backward(_dev(dy, nhwc))
        grads = [t.grad for t in lv] + ([r.grad] if r is not None else [])
    return y.detach(), grads, rm, rv


def _torch(inp, dtype, dev, training=True):
    """F.relu6(F.batch_norm(.) [+ res]) under autograd: y, the pre-activation, grads."""
    x, w, b, dy, res, nhwc = inp
    Cn = x.shape[1]
    lv = [_dev(t, False, dtype, dev).requires_grad_() for t in (x, w, b)]
    r = _dev(res, False, dtype, dev).requires_grad_() if res is not None else None
    kw = dict(dtype=dtype, device=dev)
    rm = torch.zeros(Cn, **kw) if training else torch.full((Cn,), 0.1, **kw)
    rv = torch.ones(Cn, **kw) if training else torch.full((Cn,), 0.8, **kw)
    pre = F.batch_norm(lv[0], rm, rv, lv[1], lv[2], training=training)
    pre = pre + r if r is not None else pre
    y = F.relu6(pre)
    y.backward(_dev(dy, False, dtype, dev))
    return y.detach(), pre.detach(), [t.grad for t in lv] + ([r.grad] if r is not None else [])


BN_CASES = [
    ((2, 8, 5, 5), True, False),    # NHWC mask path, C a multiple of 4 but not of 16
    ((3, 12, 7, 5), True, False),
    ((2, 6, 5, 5), False, False),   # NCHW fallback: float-output backward
    ((37, 16), False, False),       # BatchNorm1d whole-column kernels
    ((37, 32), False, False),
    ((37, 20), False, False),       # BatchNorm1d split kernels (C % 16 != 0)
    ((2, 8, 5, 5), True, True),     # fused residual
]


@pytest.mark.parametrize("shape, nhwc, residual", BN_CASES,
                         ids=lambda v: "x".join(map(str, v)) if isinstance(v, tuple) else str(v))
def test_bn_relu6_train(shape, nhwc, residual):
    inp = _inputs(shape, nhwc, residual)
    y6, g6, rm6, rv6 = _ours(inp, 2)
    y1, _, rm1, rv1 = _ours(inp, 1)
    # exact contracts
    assert torch.equal(y6, y1.clamp(max=6.0))
    assert torch.equal(rm6, rm1) and torch.equal(rv6, rv1)
    lo, mid, hi = (y6 == 0).float().mean(), ((y6 > 0) & (y6 < 6)).float().mean(), \
        (y1 >= 6).float().mean()
    print(f"shares: y<=0 {lo:.3f}  0<y<6 {mid:.3f}  y>=6 {hi:.3f}")
    assert min(lo, mid, hi) > 0.10
    assert bool((y6[y1 >= 6] == 6.0).all()) and y6.max().item() == 6.0
    _, g1, _, _ = _ours(inp, 1, dy=inp[3] * (y1 < 6).cpu().contiguous())
    for name, a, b in zip(("dx", "dw", "db", "dres"), g6, g1):
        assert torch.equal(a, b), name
    # float64 rule
    yr, pre, gr = _torch(inp, torch.float64, "cpu")
    yt, _, gt = _torch(inp, torch.float32, "cuda")
    scale = yr.abs().max().item()
    _, e_t = check_rule("y", y6, yt, yr, scale, C_BN)
    bound = 4 * e_t + C_BN * U * scale
    near = (pre.abs() <= bound) | ((pre - 6).abs() <= bound)  # the gate may differ there
    assert near.float().mean().item() <= 1e-3
    keep = ~near
    for name, a, t, r in zip(("dx", "dw", "db", "dres"), g6, gt, gr):
        if name in ("dx", "dres"):
            a, t, r = a.cpu()[keep], t.cpu()[keep], r[keep]
        elif near.any():
            continue  # a per-channel sum over an element whose gate may differ
        check_rule(name, a, t, r, r.abs().max().item(), C_BN)


@pytest.mark.parametrize("shape, nhwc", [((2, 8, 5, 5), True), ((2, 6, 5, 5), False)])
def test_bn_relu6_eval(shape, nhwc):
    inp = _inputs(shape, nhwc, False)
    y6, _, _, _ = _ours(inp, 2, training=False)
    y1, _, _, _ = _ours(inp, 1, training=False)
    assert torch.equal(y6, y1.clamp(max=6.0))
    assert (y1 >= 6).any() and bool((y6[y1 >= 6] == 6.0).all()) and (y6 == 0).any()
    yr, _, _ = _torch(inp, torch.float64, "cpu", training=False)
    yt, _, _ = _torch(inp, torch.float32, "cuda", training=False)
    check_rule("y", y6, yt, yr, yr.abs().max().item(), C_BN)


def test_bn_relu6_eval_with_grad_and_residual_fallback():
    """The two branches of ops.batch_norm that finish in torch ops use F.relu6 too."""
    inp = _inputs((2, 6, 5, 5), False, True)  # C % 4 != 0: the residual is added outside
    y6, g6, _, _ = _ours(inp, 2)
    yr, _, gr = _torch(inp, torch.float64, "cpu")
    yt, _, gt = _torch(inp, torch.float32, "cuda")
    check_rule("y", y6, yt, yr, yr.abs().max().item(), C_BN)
    for name, a, t, r in zip(("dx", "dw", "db", "dres"), g6, gt, gr):
        check_rule(name, a, t, r, r.abs().max().item(), C_BN)
    x, w, b, dy, _, _ = inp
    xa = x.cuda().requires_grad_()
    rm, rv = torch.full((6,), 0.1, device="cuda"), torch.full((6,), 0.8, device="cuda")
    y = ops.batch_norm(xa, rm, rv, w.cuda(), b.cuda(), training=False, relu6=True)
    ref = F.relu6(F.batch_norm(x.double(), rm.double().cpu(), rv.double().cpu(), w.double(),
                               b.double(), training=False))
    assert y.max().item() == 6.0 and y.min().item() == 0.0
    torch.testing.assert_close(y.double().cpu(), ref, rtol=1e-6, atol=1e-5)


@pytest.mark.parametrize("Cn", [16, 20])
def test_bn_relu6_sync_halves(Cn):
    """SyncBatchNorm's kernels around the collectives (a group of one rank): bn1d_moments ->
    bn1d_gathered_fwd and bn1d_sums at C % 16 == 0, bn_merge + the split kernels otherwise. Same
    bitwise contracts, and the results equal the group-less forms by the float64 rule."""
    from tutorial_torch_distributed_data_parallel_amd.parallel import runtime as rt

    inp = _inputs((37, Cn), False, False)

    def run(act, dy):
        lv = [t.cuda().requires_grad_() for t in inp[:3]]
        rm, rv = torch.zeros(Cn, device="cuda"), torch.ones(Cn, device="cuda")
        y = ops.batch_norm(lv[0], rm, rv, lv[1], lv[2], training=True, relu=act == 1,
                           relu6=act == 2, group=rt.SyncGroup())
        y.backward(dy.cuda())
        return y.detach(), [t.grad for t in lv], rm, rv

    y6, g6, rm6, rv6 = run(2, inp[3])
    y1, _, rm1, rv1 = run(1, inp[3])
    assert torch.equal(y6, y1.clamp(max=6.0)) and (y1 >= 6).float().mean() > 0.1
    assert torch.equal(rm6, rm1) and torch.equal(rv6, rv1)
    _, g1, _, _ = run(1, inp[3] * (y1 < 6).cpu())
    for name, a, b in zip(("dx", "dw", "db"), g6, g1):
        assert torch.equal(a, b), name
    yr, _, gr = _torch(inp, torch.float64, "cpu")
    yt, _, gt = _torch(inp, torch.float32, "cuda")
    check_rule("y", y6, yt, yr, yr.abs().max().item(), C_BN)
    for name, a, t, r in zip(("dx", "dw", "db"), g6, gt, gr):
        check_rule(name, a, t, r, r.abs().max().item(), C_BN)


# ------------------------------------------------------------------------- stand-alone ReLU6
def _specials():
    z, six = torch.tensor(0.0), torch.tensor(6.0)
    inf = torch.tensor(float("inf"))
    return torch.stack([z, six, -z, torch.nextafter(z, inf), torch.nextafter(z, -inf),
                        torch.nextafter(six, inf), torch.nextafter(six, -inf), inf, -inf,
                        torch.tensor(3.0), torch.tensor(-2.0), torch.tensor(7.5)])


@pytest.mark.parametrize("n", [1, 3, 4, 1023, 4099])
def test_standalone_relu6(n):
    sp = _specials()
    g = torch.Generator().manual_seed(n)
    # short sizes cannot hold every special value at once: every window of the list is run
    starts = range(len(sp)) if n < len(sp) else [0]
    for s0 in starts:
        body = torch.cat([sp.roll(-s0), torch.randn(max(n, 1), generator=g) * 4 + 3])[:n]
        if n >= len(sp):
            assert all((body == v).any() for v in sp) and (body[2:3].signbit()).all()
        x = body.cuda().requires_grad_()
        dy = torch.randn(n, generator=g).cuda()
        y = ops.relu6(x)
        assert torch.equal(y, F.relu6(body).cuda())
        y.backward(dy)
        open_ = ((body > 0) & (body < 6)).cuda()
        assert torch.equal(x.grad, torch.where(open_, dy, torch.zeros_like(dy)))
    nan = torch.full((n,), float("nan"), device="cuda")
    assert torch.isnan(ops.relu6(nan)).all() and torch.isnan(F.relu6(nan)).all()


def test_standalone_relu6_module_and_layouts():
    x = (torch.randn(2, 8, 5, 7) * 4 + 3).cuda().contiguous(memory_format=CL).requires_grad_()
    y = tdp.nn.ReLU6()(x)
    assert y.is_contiguous(memory_format=CL) and torch.equal(y, F.relu6(x.detach()))
    dy = torch.randn(2, 8, 5, 7, device="cuda")  # NCHW upstream gradient for an NHWC forward
    y.backward(dy)
    xd = x.detach()
    assert torch.equal(x.grad, torch.where((xd > 0) & (xd < 6), dy, torch.zeros_like(dy)))
    with pytest.raises(TypeError):
        ops.relu6(torch.zeros(4, device="cuda", dtype=torch.float64))
    # a view that starts 4 bytes into its storage: the element-by-element form of both kernels
    base = (torch.randn(1030) * 4 + 3).cuda()
    xu = base[1:].detach().requires_grad_()
    assert xu.data_ptr() % 16 == 4
    yu = ops.relu6(xu)
    assert torch.equal(yu, F.relu6(base[1:]))
    du = torch.randn(1030, device="cuda")[1:]
    yu.backward(du)
    bu = base[1:]
    assert torch.equal(xu.grad, torch.where((bu > 0) & (bu < 6), du, torch.zeros_like(du)))


# ------------------------------------------------------- depthwise BatchNorm statistics
# A 256-thread block of dwconv_kernel covers 256 (channel quad, 8-pixel chunk) items: 1024 pixels
# at C = 8, about 227 at C = 36 (where 256 is no multiple of the 9 quads, so a chunk's quads
# straddle two blocks). (N, C, H, W, R, stride, pad)
DW_STATS = [
    (1, 8, 7, 5, 3, 1, 1),       # 35 pixels: less than one block covers
    (8, 8, 21, 19, 3, 1, 1),     # 3192 pixels: 4 blocks, the last ragged
    (5, 36, 13, 11, 3, 1, 1),    # 715 pixels, 810 items: 4 blocks, the last ragged
    (4, 36, 15, 13, 3, 2, 1),    # stride 2, odd extents
    (3, 8, 21, 19, 5, 1, 2),     # 5x5, 2 blocks
    (2, 36, 9, 7, 5, 2, 2),      # 5x5 stride 2
]


@pytest.fixture
def dw_stats_on():
    old, ops.conv.DW_BN_STATS = ops.conv.DW_BN_STATS, True
    yield
    ops.conv.DW_BN_STATS = old


def _dw_operands(N, Cn, H, W, R, mult=1):
    g = torch.Generator(device="cuda").manual_seed(5)
    x = torch.randn(N, Cn, H, W, device="cuda", generator=g).contiguous(memory_format=CL) + 0.7
    w = torch.randn(Cn * mult, 1, R, R, device="cuda", generator=g) * 0.2
    return x, w


@pytest.mark.parametrize("geom", DW_STATS, ids=lambda g: "x".join(map(str, g)))
def test_depthwise_bn_stats(geom, dw_stats_on):
    """ops.conv2d(groups=C, bn_stats=True) with DW_BN_STATS: the per-block (count, mean, M2)
    merged by bn_moments_partials equal the moments of the stored output (the assertions and
    bounds of tests/test_cnn_gpu.py::test_conv_epilogue_bn_stats), bitwise repeatable, with y
    bitwise the output without the epilogue; batch_norm consumes them."""
    from tutorial_torch_distributed_data_parallel_amd._native import native

    C = native()
    N, Cn, H, W, R, st, pad = geom
    x, w = _dw_operands(N, Cn, H, W, R)
    y = ops.conv2d(x, w, None, st, pad, groups=Cn, bn_stats=True)
    tag = getattr(y, "_tdp_bn_part", None)
    assert tag is not None and tag[0].shape[1:] == (3, Cn)
    items = (Cn // 4) * ((y.numel() // Cn + 7) // 8)
    assert tag[0].shape[0] == (items + 255) // 256
    y2 = ops.conv2d(x, w, None, st, pad, groups=Cn, bn_stats=True)
    assert torch.equal(y2._tdp_bn_part[0], tag[0])
    ops.conv.DW_BN_STATS = False
    y0 = ops.conv2d(x, w, None, st, pad, groups=Cn, bn_stats=True)
    ops.conv.DW_BN_STATS = True
    assert getattr(y0, "_tdp_bn_part", None) is None and torch.equal(y0, y)
    assert getattr(ops.conv2d(x, w, None, st, pad, groups=Cn), "_tdp_bn_part", None) is None
    rows = y.permute(0, 2, 3, 1).reshape(-1, Cn)
    ref = C.bn_moments(rows)[0]
    got = C.bn_moments_partials(tag[0], float(rows.shape[0]))
    assert tag[0][:, 0].sum(0).tolist() == [float(rows.shape[0])] * Cn
    torch.testing.assert_close(got[:Cn], ref[:Cn], atol=1e-5, rtol=1e-5)
    torch.testing.assert_close(got[Cn:2 * Cn], ref[Cn:2 * Cn], atol=1e-5, rtol=1e-4)
    assert got[2 * Cn].item() == rows.shape[0]
    yd = y.double()
    torch.testing.assert_close(got[:Cn].double(), yd.mean((0, 2, 3)), atol=1e-5, rtol=1e-5)
    torch.testing.assert_close(got[Cn:2 * Cn].double(), yd.var((0, 2, 3), unbiased=False),
                               atol=1e-5, rtol=1e-4)
    gamma, beta = torch.randn(Cn, device="cuda"), torch.randn(Cn, device="cuda")
    o1 = ops.batch_norm(y, None, None, gamma, beta, training=True, relu6=True)
    o2 = ops.batch_norm(y.clone(), None, None, gamma, beta, training=True, relu6=True)
    torch.testing.assert_close(o1, o2, atol=1e-5, rtol=1e-5)


def test_depthwise_bn_stats_forms_without_statistics(dw_stats_on):
    """The generic stencil (7x7; channel multiplier 2), a bias and a fused ReLU emit no tag."""
    x, w = _dw_operands(1, 8, 9, 9, 7)
    assert getattr(ops.conv2d(x, w, None, 2, 3, groups=8, bn_stats=True), "_tdp_bn_part",
                   None) is None
    x, w = _dw_operands(1, 8, 6, 6, 3, mult=2)
    assert getattr(ops.conv2d(x, w, None, 1, 1, groups=8, bn_stats=True), "_tdp_bn_part",
                   None) is None
    x, w = _dw_operands(1, 8, 6, 6, 3)
    b = torch.zeros(8, device="cuda")
    assert getattr(ops.conv2d(x, w, b, 1, 1, groups=8, bn_stats=True), "_tdp_bn_part",
                   None) is None
    assert getattr(ops.conv2d(x, w, None, 1, 1, groups=8, bn_stats=True, relu=True),
                   "_tdp_bn_part", None) is None


# ------------------------------------------------------------------------------- the blocks
@pytest.mark.parametrize("inp, oup, stride", [(32, 32, 1), (24, 32, 2)])
@pytest.mark.parametrize("fused", [True, False])
@pytest.mark.parametrize("dw_stats", [False, True])
def test_inverted_residual_matches_float64_twin(inp, oup, stride, fused, dw_stats, monkeypatch):
    monkeypatch.setattr(ops.conv, "DW_BN_STATS", dw_stats)
    torch.manual_seed(0)
    blk = InvertedResidual(inp, oup, stride, 6, device="cuda").train()
    blk._fused_join = fused
    assert blk.use_res_connect == (stride == 1)
    t32 = TwinInvertedResidual(inp, oup, stride, 6).cuda().train()
    with torch.no_grad():
        for m in blk.modules():  # spread the BatchNorm affine so that ReLU6 clamps both ways
            if isinstance(m, tdp.nn.BatchNorm2d) and m.relu6:
                m.weight.uniform_(1, 3)
                m.bias.uniform_(1, 3)
    t32.load_state_dict(blk.state_dict())
    t64 = copy.deepcopy(t32).double().cpu()
    g = torch.Generator().manual_seed(3)
    x = torch.randn(4, inp, 14, 14, generator=g)
    dy = torch.randn(4, oup, 14 // stride, 14 // stride, generator=g)
    xs = [x.cuda().contiguous(memory_format=CL).requires_grad_(), x.cuda().requires_grad_(),
          x.double().requires_grad_()]
    ys = [blk(xs[0]), t32(xs[1]), t64(xs[2])]
    for y, d in zip(ys, (dy.cuda(), dy.cuda(), dy.double())):
        y.backward(d)
    check_rule("y", ys[0], ys[1], ys[2], ys[2].abs().max().item(), C_BN)
    check_rule("dx", xs[0].grad, xs[1].grad, xs[2].grad, xs[2].grad.abs().max().item(), C_BN)
    check_grads_rule("block", blk, t32, t64, C_BN)


# -------------------------------------------------------------------------------- the model
@pytest.fixture(scope="module")
def pg():
    if not tdp.parallel.is_initialized():
        tdp.init_process_group("nccl", rank=0, world_size=1, local_rank=0)
    yield tdp
    tdp.destroy_process_group()


@pytest.fixture(scope="module")
def nets():
    """The model and its fp32 / float64 twins with the same weights; dropout off (the model's
    and torch's generators draw different masks, which no tolerance covers)."""
    torch.manual_seed(0)
    net = mobilenet_v2(num_classes=10, device="cuda")
    t32 = TwinMobileNetV2(num_classes=10).cuda()
    t32.load_state_dict(net.state_dict())
    for m in (net, t32):
        m.classifier[0].p = 0.0
    return net, t32, copy.deepcopy(t32).double().cpu()


def test_eval_forward_and_autocast(nets):
    """Eval-mode forward against the twins, on copies that share weights AND running statistics:
    those of one batch (momentum 1) taken by the float64 twin, so that the comparison is of the
    eval forward alone. (With the initial 0 / 1 the signal all but vanishes through 52 layers;
    with each side's own fp32 statistics the comparison would be of the training-mode moments,
    which tests/test_cnn_gpu.py and tests/test_hard_inputs_gpu.py bound.)"""
    net, t32, t64 = (copy.deepcopy(m) for m in nets)
    gen = torch.Generator().manual_seed(2)
    x0 = torch.randn(8, 3, 64, 64, generator=gen)
    with torch.no_grad():
        for b in t64.modules():
            if isinstance(b, torch.nn.modules.batchnorm._BatchNorm):
                b.momentum = 1.0
        t64.train()(x0.double())
    net.load_state_dict(t64.state_dict())
    t32.load_state_dict(t64.state_dict())
    assert net.features[0][1].running_var.dtype == torch.float32
    net.eval(), t32.eval(), t64.eval()
    x = torch.randn(8, 3, 64, 64, generator=gen)
    with torch.no_grad():
        y, yt, yr = net(x.cuda()), t32(x.cuda()), t64(x.double())
        assert yr.abs().max().item() > 1e-2  # a live signal
        check_rule("eval logits", y, yt, yr, yr.abs().max().item(), C_BN)
        # under autocast the 1x1 convolutions run in bf16 and the depthwise layers stay fp32:
        # fed the same input, a depthwise layer gives bitwise the result it gives outside
        dw = net.features[2].conv[1][0]
        assert dw.groups == dw.in_channels == 96
        h = torch.randn(8, 96, 32, 32, device="cuda").contiguous(memory_format=CL)
        ref = dw(h)
        with tdp.autocast():
            ya = net(x.cuda())
            assert torch.equal(dw(h), ref)
        assert ya.shape == (8, 10) and bool(torch.isfinite(ya).all())
        assert not torch.equal(ya, y)  # the dense layers did run in bf16


def test_three_sgd_steps_under_ddp_match_torch(pg, nets):
    """mobilenet_v2(num_classes=10), batch 8 at 64x64 (the final map is 2x2: every BatchNorm sees
    >= 32 values per channel), three SGD steps (lr 0.01, momentum 0.9) under tdp.DDP at world
    size 1 against the torch twin with torch.optim.SGD. Every parameter must either meet the
    ResNeXt test's rtol = 1e-4 / atol = 1e-5 against the fp32 twin, or lie within 4x torch
    fp32's own distance from the float64 twin run on the same steps (+ 2 * 2^-24 * scale): the
    project rule, not a widened tolerance. The BatchNorm running statistics are held to the same
    criterion. Measured: the fp32 twin itself ends up to 8.3e3 tolerances away from this model
    -- and as far from its own float64 copy -- because the untrained network's gradients are
    large and a ReLU6 gate that flips on a rounding moves them; against float64 this model stays
    within 0.76 of the 4 e_t bound. Figures: profiles/r18/mobilenet_v2.md."""
    net, t32, t64 = nets
    ddp = tdp.DDP(net, device_ids=[0])
    opt = tdp.optim.SGD(ddp.parameters(), lr=0.01, momentum=0.9)
    assert ddp.register_fused_optimizer(opt)
    opts = [torch.optim.SGD(t.parameters(), lr=0.01, momentum=0.9) for t in (t32, t64)]
    gen = torch.Generator().manual_seed(1)
    for _ in range(3):
        x = torch.randn(8, 3, 64, 64, generator=gen)
        y = torch.randint(0, 10, (8,), generator=gen)
        opt.zero_grad(set_to_none=True)
        tdp.ops.cross_entropy(ddp(x.cuda()), y.cuda()).backward()
        opt.step()
        for t, o, xx, yy in ((t32, opts[0], x.cuda(), y.cuda()), (t64, opts[1], x.double(), y)):
            o.zero_grad(set_to_none=True)
            F.cross_entropy(t(xx), yy).backward()
            o.step()
    torch.cuda.synchronize()
    # parameters and the BatchNorm running statistics, one criterion
    def named(m):
        return [(n, t) for n, t in list(m.named_parameters()) + list(m.named_buffers())
                if t.dtype.is_floating_point]

    worst_close = worst_rule = worst_ek = worst_et = 0.0
    bad = []
    for (n, p), (_, q), (_, r) in zip(named(net), named(t32), named(t64)):
        p, q, r = p.detach().double().cpu(), q.detach().double().cpu(), r.detach()
        d = (p - q).abs()
        close = bool((d <= 1e-5 + 1e-4 * q.abs()).all())
        e_k, e_t = (p - r).abs().max().item(), (q - r).abs().max().item()
        bound = 4 * e_t + C_BN * U * r.abs().max().item()
        worst_close = max(worst_close, (d / (1e-5 + 1e-4 * q.abs())).max().item())
        worst_rule = max(worst_rule, e_k / bound)
        worst_ek, worst_et = max(worst_ek, e_k), max(worst_et, e_t)
        if not (close or e_k <= bound):
            bad.append((n, d.max().item(), e_k, e_t))
    print(f"[steps] worst |p - q| / (atol + rtol |q|) = {worst_close:.3f}; "
          f"worst e_k / (4 e_t + 2 U scale) = {worst_rule:.3f}; "
          f"largest e_k = {worst_ek:.3e}, largest e_t = {worst_et:.3e}")
    assert not bad, bad[:5]
    del ddp
