"""Mixed-precision convolution (csrc/conv_bf16.hip) under tdp.autocast: fp32 tensors, every operand
element of each pass rounded once to bf16 (RNE), exact products, fp32 accumulation.

The oracle is float64 ``F.conv2d`` (and its autograd) on the ROUNDED operands; the error is scaled
by the same convolution of the absolute values and bounded by (8 + 2 sqrt(K)) 2^-24, the bound of
tests/test_gemm_bf16_gpu.py for the same MFMA instruction, with K the pass's reduction length:
R*S*Cin (forward), taps*Cout (input gradient; a strided gradient runs as stride phases, so the
taps of the largest phase, ceil(R/sh)*ceil(S/sw)), N*P*Q (weight gradient)."""
import math

import pytest
import torch
import torch.nn.functional as F

import tutorial_torch_distributed_data_parallel_amd as tdp
from tutorial_torch_distributed_data_parallel_amd import ops
from tutorial_torch_distributed_data_parallel_amd.ops import conv as convmod

pytestmark = pytest.mark.gpu

U = 2.0 ** -24

# (N, C, H, W, Cout, R, stride, pad)
GEOMS = [
    (2, 3, 63, 63, 64, 11, 4, 2),      # stem padded to 4 channels, stride-4 phases
    (2, 64, 15, 15, 192, 5, 1, 2),
    (2, 192, 13, 13, 384, 3, 1, 1),
    (3, 64, 14, 14, 256, 1, 1, 0),
    (2, 256, 14, 14, 512, 1, 2, 0),
    (2, 128, 15, 15, 128, 3, 2, 1),
    (2, 3, 40, 40, 64, 7, 2, 3),
    (1, 4, 5, 5, 4, 3, 1, 1),          # everything under one tile, K = 36
    (2, 12, 9, 7, 20, 3, 1, 1),        # C % 8 == 4: a chunk straddles two taps; Cout % 8 != 0
    (1, 8, 6, 6, 8, 3, 2, 0),          # phases with an empty tap set
    (4, 64, 8, 8, 132, 3, 1, 1),       # Cout one quad past a tile; C % 64 == 0: uniform path
]
G_C12 = (2, 12, 9, 7, 20, 3, 1, 1)
G_C64R5 = (2, 64, 15, 15, 192, 5, 1, 2)
G_SPLIT = (2, 192, 13, 13, 384, 3, 1, 1)


@pytest.fixture(scope="module")
def C():
    from tutorial_torch_distributed_data_parallel_amd._native import native

    return native()


def _bound(K):
    return (8 + 2 * K ** 0.5) * U


def _out_hw(geom):
    N, Cin, H, W, Cout, R, s, p = geom
    return (H + 2 * p - R) // s + 1, (W + 2 * p - R) // s + 1


def _reductions(geom):
    """K of (forward, input gradient, weight gradient)"""
    N, Cin, H, W, Cout, R, s, p = geom
    P, Q = _out_hw(geom)
    return R * R * Cin, math.ceil(R / s) ** 2 * Cout, N * P * Q


def _tensors(geom, dist="normal", seed=0):
    N, Cin, H, W, Cout, R, s, p = geom
    P, Q = _out_hw(geom)
    g = torch.Generator(device="cpu").manual_seed(seed + sum(geom))
    ts = [torch.randn(N, Cin, H, W, generator=g), torch.randn(Cout, Cin, R, R, generator=g),
          torch.randn(N, Cout, P, Q, generator=g)]
    if dist == "wide":  # 2^[-20, 20] magnitudes
        ts = [t * torch.exp2(torch.randint(-20, 21, t.shape, generator=g).float()) for t in ts]
    return ts


def _oracle(x, w, dy, geom, rounded=True):
    """float64 (y, dx, dw) of the (rounded) operands and their |.| scales, on the CPU"""
    s, p = geom[6], geom[7]
    cast = (lambda t: t.detach().cpu().bfloat16().double()) if rounded else \
        (lambda t: t.detach().cpu().double())
    res = []
    for f in (lambda t: t, torch.abs):
        xr, wr = f(cast(x)).requires_grad_(), f(cast(w)).requires_grad_()
        y = F.conv2d(xr, wr, None, s, p)
        y.backward(f(cast(dy)))
        res.append((y.detach(), xr.grad, wr.grad))
    return res


def _scaled_err(out, ref, scale):
    return ((out.double().cpu() - ref).abs() / scale.clamp_min(1e-300)).max().item()


def _passes(x, w, dy, geom, bf16, bias=None, relu=False):
    """(y, dx, dw[, db]) of the NHWC convolution op family on the GPU"""
    s, p = geom[6], geom[7]
    x = x.cuda().requires_grad_()
    w = w.cuda().contiguous(memory_format=torch.channels_last).requires_grad_()
    b = None if bias is None else bias.cuda().requires_grad_()
    y = convmod._ConvNHWCFn.apply(x, w, b, (s, s), (p, p), relu, None, None, bf16)
    y.backward(dy.cuda())
    torch.cuda.synchronize()
    out = (y.detach(), x.grad, w.grad)
    return out if b is None else out + (b.grad,)


@pytest.fixture(scope="module")
def reference():
    """per (geometry, distribution): the operands and the oracle, computed once and shared"""
    cache = {}

    def get(geom, dist="normal"):
        if (geom, dist) not in cache:
            x, w, dy = _tensors(geom, dist)
            cache[(geom, dist)] = (x, w, dy, _oracle(x, w, dy, geom))
        return cache[(geom, dist)]

    return get


@pytest.mark.parametrize("geom", GEOMS, ids=lambda g: "x".join(map(str, g)))
@pytest.mark.parametrize("dist", ["normal", "wide"])
def test_passes_match_rounded_operand_oracle(C, reference, geom, dist):
    x, w, dy, (ref, scale) = reference(geom, dist)
    out = _passes(x, w, dy, geom, True)
    errs = []
    for name, o, r, sc, K in zip(("forward", "dgrad", "wgrad"), out, ref, scale,
                                 _reductions(geom)):
        e = _scaled_err(o, r, sc)
        print(f"{name}: scaled error {e / U:.2f} u, bound {_bound(K) / U:.2f} u (K = {K})")
        errs.append((name, e, _bound(K)))
    for name, e, b in errs:
        assert e < b, (name, e, b)


@pytest.mark.parametrize("geom", [G_C12, G_C64R5], ids=["C12", "C64R5"])
def test_exact_on_representable_operands(C, geom):
    # integers |v| <= 7 times a power of two are bf16 values; at most 1600 products of <= 49 sum
    # far below 2^24 in units of the common scale: every partial sum is exact in fp32, in any
    # order, so any wrong tap, pixel, padding decision or tail shows as a mismatch
    g = torch.Generator(device="cpu").manual_seed(11)
    shapes = [t.shape for t in _tensors(geom)]
    x, w, dy = [torch.randint(-7, 8, sh, generator=g).float() * 2.0 ** e
                for sh, e in zip(shapes, (-3, 2, 5))]
    (ref, _) = _oracle(x, w, dy, geom, rounded=False)
    out = _passes(x, w, dy, geom, True)
    for name, o, r in zip(("forward", "dgrad", "wgrad"), out, ref):
        assert torch.equal(o.cpu(), r.float()), name


def test_bias_and_relu_epilogue_bitwise(C):
    geom = G_C12
    x, w, dy = _tensors(geom)
    b = torch.randn(geom[4])
    y_plain = _passes(x, w, dy, geom, True)[0]
    y, _, _, db = _passes(x, w, dy, geom, True, bias=b, relu=True)
    want = torch.relu(y_plain + b.cuda().view(1, -1, 1, 1))
    assert torch.equal(y, want)
    # the bias gradient is summed from the UNROUNDED masked gradient
    g = dy.cuda() * (y > 0)
    n = g.numel() // geom[4]
    err = (db.double() - g.double().sum(dim=(0, 2, 3))).abs()
    assert bool((err <= _bound(n) * g.double().abs().sum(dim=(0, 2, 3))).all())
    gr = g.bfloat16().float()
    assert not torch.equal(g, gr)


def test_operands_are_really_rounded(C, reference):
    geom = G_C64R5
    x, w, dy, (ref, scale) = reference(geom)
    y16 = _passes(x, w, dy, geom, True)[0]
    y32 = _passes(x, w, dy, geom, False)[0]
    assert not torch.equal(y16, y32)
    (ref32, scale32) = _oracle(x, w, dy, geom, rounded=False)
    K = _reductions(geom)[0]
    assert _scaled_err(y16, ref[0], scale[0]) < _bound(K)
    assert _scaled_err(y16, ref32[0], scale32[0]) > _bound(K)


def test_dgrad_w_accumulates_into_out(C):
    geom = G_C64R5
    N, Cin, H, W, Cout, R, s, p = geom
    x, w, dy = _tensors(geom)
    wt = w.cuda().contiguous(memory_format=torch.channels_last)
    g = dy.cuda().contiguous(memory_format=torch.channels_last)
    plain = C.conv_nhwc_dgrad_w(g, wt, [N, Cin, H, W], 1, 1, p, p, bf16=True)
    old = torch.randn(N, Cin, H, W, device="cuda").contiguous(memory_format=torch.channels_last)
    out = old.clone(memory_format=torch.channels_last)
    res = C.conv_nhwc_dgrad_w(g, wt, [N, Cin, H, W], 1, 1, p, p, out=out, beta=1.0, bf16=True)
    torch.cuda.synchronize()
    assert res.data_ptr() == out.data_ptr()
    assert torch.equal(out, old + plain)


def test_split_k_weight_gradient_is_deterministic(C):
    geom = G_SPLIT
    N, Cin, H, W, Cout, R, s, p = geom
    splits, kps = C.conv_bf16_plan(2, [N, Cin, H, W], Cout, R, R, s, s, p, p)
    assert splits > 1 and kps % 64 == 0
    x, w, dy = _tensors(geom)
    a = _passes(x, w, dy, geom, True)[2]
    b = _passes(x, w, dy, geom, True)[2]
    assert torch.equal(a, b)


def _conv2d_passes(x, w, dy, geom, backward_inside=True, autocast=True):
    s, p = geom[6], geom[7]
    x = x.cuda().requires_grad_()
    w = w.cuda().contiguous(memory_format=torch.channels_last).requires_grad_()
    with tdp.autocast(enabled=autocast):
        y = ops.conv2d(x, w, None, s, p)
        if backward_inside:
            y.backward(dy.cuda())
    if not backward_inside:
        y.backward(dy.cuda())
    torch.cuda.synchronize()
    return y.detach(), x.grad, w.grad


@pytest.mark.parametrize("geom", [G_C12, (2, 128, 15, 15, 128, 3, 2, 1)], ids=["C12", "s2"])
def test_dispatch(C, geom):
    x, w, dy = _tensors(geom)
    direct16 = _passes(x, w, dy, geom, True)
    direct32 = _passes(x, w, dy, geom, False)
    assert not torch.equal(direct16[0], direct32[0])
    for a, b in zip(_conv2d_passes(x, w, dy, geom), direct16):
        assert torch.equal(a, b)
    for a, b in zip(_conv2d_passes(x, w, dy, geom, autocast=False), direct32):
        assert torch.equal(a, b)
    # chosen in forward: the backward outside the region follows it
    for a, b in zip(_conv2d_passes(x, w, dy, geom, backward_inside=False), direct16):
        assert torch.equal(a, b)
    # the A/B switch keeps the convolution fp32 inside the region
    convmod.AUTOCAST_FP32_CONV = True
    try:
        for a, b in zip(_conv2d_passes(x, w, dy, geom), direct32):
            assert torch.equal(a, b)
    finally:
        convmod.AUTOCAST_FP32_CONV = False


def test_backward_outside_region_meets_the_contract(C, reference):
    geom = G_C12
    x, w, dy, (ref, scale) = reference(geom)
    out = _conv2d_passes(x, w, dy, geom, backward_inside=False)
    for o, r, sc, K in zip(out, ref, scale, _reductions(geom)):
        assert _scaled_err(o, r, sc) < _bound(K)


def test_odd_shape_stays_fp32_under_autocast(C):
    geom = (1, 5, 9, 11, 7, 3, 1, 1)  # channel counts the NHWC path does not take
    x, w, dy = _tensors(geom)
    inside = _conv2d_passes(x, w, dy, geom)
    outside = _conv2d_passes(x, w, dy, geom, autocast=False)
    for a, b in zip(inside, outside):
        assert torch.equal(a, b)


# ------------------------------------------------------------------------------- layer-wise models
class _Tap:
    """Hooks on every tdp.nn.Conv2d: the layer's actual input, output and their gradients."""

    def __init__(self, model):
        self.rec = {}
        for name, m in model.named_modules():
            if isinstance(m, tdp.nn.Conv2d):
                m.register_forward_hook(self._hook(name))

    def _hook(self, name):
        def fwd(mod, args, out):
            r = self.rec[name] = {"mod": mod, "x": args[0].detach().clone(),
                                  "y": out.detach().clone(), "bn_part": hasattr(out, "_tdp_bn_part")}
            if args[0].requires_grad:
                args[0].register_hook(lambda g: r.__setitem__("dx", g.detach().clone()))
            out.register_hook(lambda g: r.__setitem__("dy", g.detach().clone()))
        return fwd


def _check_layer(name, r, check_dx=True):
    mod = r["mod"]
    s, p = mod.stride[0], mod.padding[0]
    x, w, y, dy = r["x"], mod.weight.detach(), r["y"], r["dy"]
    N, Cin, H, W = x.shape
    Cout, _, R, _ = w.shape
    geom = (N, Cin, H, W, Cout, R, s, p)
    g = dy * (y > 0) if mod.relu else dy   # the unrounded masked gradient is what gets rounded
    (ref, scale) = _oracle(x, w, g, geom)
    Kf, Kd, Kw = _reductions(geom)
    yref, ysc = ref[0], scale[0]
    if mod.bias is not None:
        # the bias is added in fp32 after the accumulation: one more rounding of the result
        yref = yref + mod.bias.detach().double().cpu().view(1, -1, 1, 1)
        ysc = ysc + mod.bias.detach().double().abs().cpu().view(1, -1, 1, 1)
    if mod.relu:
        yref = yref.clamp_min(0)
    assert _scaled_err(y, yref, ysc) < _bound(Kf) + U, (name, "forward")
    assert _scaled_err(mod.weight.grad, ref[2], scale[2]) < _bound(Kw), (name, "wgrad")
    if check_dx:
        assert _scaled_err(r["dx"], ref[1], scale[1]) < _bound(Kd), (name, "dgrad")
    assert not r["bn_part"], (name, "statistics epilogue under autocast")


def test_small_net_layerwise(C):
    torch.manual_seed(0)
    conv2 = tdp.nn.Conv2d(16, 24, 3, stride=2, padding=1, bias=False, device="cuda")
    conv2.bn_stats = True  # asks for the statistics epilogue: under autocast BatchNorm falls back
    net = torch.nn.Sequential(
        tdp.nn.Conv2d(8, 16, 3, padding=1, relu=True, device="cuda"), tdp.nn.MaxPool2d(2),
        conv2, tdp.nn.BatchNorm2d(24, device="cuda"), torch.nn.Flatten(),
        tdp.nn.Linear(24 * 4 * 4, 10, device="cuda")).train()
    tap = _Tap(net)
    x = torch.randn(4, 8, 16, 16, device="cuda", requires_grad=True)
    with tdp.autocast():
        out = net(x)
    out.square().sum().backward()
    torch.cuda.synchronize()
    assert len(tap.rec) == 2
    for name, r in tap.rec.items():
        _check_layer(name, r)
    bn = net[3]
    assert torch.isfinite(bn.running_var).all() and not torch.equal(
        bn.running_var, torch.ones_like(bn.running_var))


def test_bottleneck_layerwise(C):
    from tutorial_torch_distributed_data_parallel_amd.models.resnet import Bottleneck

    torch.manual_seed(1)
    ds = torch.nn.Sequential(tdp.nn.Conv2d(32, 64, 1, stride=2, bias=False, device="cuda"),
                             tdp.nn.BatchNorm2d(64, device="cuda"))
    blk = Bottleneck(32, 16, stride=2, downsample=ds, device="cuda").train()
    for c in (blk.conv1, blk.conv2, blk.conv3, ds[0]):
        c.bn_stats = True
    tap = _Tap(blk)
    x = torch.randn(4, 32, 12, 12, device="cuda", requires_grad=True)
    with tdp.autocast():
        out = blk(x)
    out.square().sum().backward()
    torch.cuda.synchronize()
    assert len(tap.rec) == 4
    for name, r in tap.rec.items():
        # conv1 and the downsample accumulate their input gradients into one shared buffer
        # (covered by test_dgrad_w_accumulates_into_out): check the other two
        _check_layer(name, r, check_dx=name in ("conv2", "conv3"))


@pytest.fixture()
def pg():
    from tutorial_torch_distributed_data_parallel_amd.parallel import runtime as rt

    if tdp.parallel.is_initialized() and rt.get_backend() != "nccl":
        tdp.destroy_process_group()
    if not tdp.parallel.is_initialized():
        tdp.init_process_group("nccl", rank=0, world_size=1, local_rank=0)
    yield tdp
    tdp.destroy_process_group()


def test_alexnet_trains_under_accelerator_bf16(pg):
    from tutorial_torch_distributed_data_parallel_amd.accelerate import Accelerator
    from tutorial_torch_distributed_data_parallel_amd.models.registry import build_model

    torch.manual_seed(0)
    acc = Accelerator(mixed_precision="bf16")
    m = build_model("alexnet").cuda().eval()  # eval: no dropout noise between the steps
    opt = tdp.optim.SGD(m.parameters(), lr=1e-2)
    m, opt = acc.prepare(m, opt)
    x = torch.randn(2, 3, 224, 224, device="cuda")
    y = torch.tensor([1, 7], device="cuda")
    losses = []
    for _ in range(4):
        opt.zero_grad()
        loss = tdp.ops.cross_entropy(m(x), y)
        losses.append(loss.item())
        if len(losses) == 4:
            break
        acc.backward(loss)
        for p in m.parameters():
            assert p.dtype == torch.float32 and p.grad is not None
            assert p.grad.dtype == torch.float32
        opt.step()
    print("losses", losses)
    assert all(math.isfinite(v) for v in losses)
    assert losses[-1] < losses[0]
    assert all(v.dtype == torch.float32 for v in m.state_dict().values() if v.is_floating_point())
