"""Grouped and depthwise convolution (csrc/conv_grouped.hip; ops.conv2d / nn.Conv2d ``groups=``).

The oracle is float64 ``F.conv2d(..., groups=)`` and its autograd on the same fp32 operands,
computed on the CPU with no operand rounding. The error of each output is scaled by the same
convolution of the absolute values (``_oracle`` / ``_scaled_err`` of tests/test_conv_bf16_gpu.py)
and must stay under (8 + 2 sqrt(K)) 2^-24, the project's bound for one rounding per accumulation
step, with K the pass's reduction length: R*S*Cg (forward), taps*Kg (input gradient: the kernel
gathers directly and the skipped taps add exact zeros, so the taps of the largest stride phase,
ceil(R/s)^2, are what accumulates), N*P*Q (weight gradient).

Whole-block and bias-gradient checks use the rule of tests/test_hard_inputs_gpu.py,
e_k <= 4 e_t + c 2^-24 scale, with e_t the error of torch's own fp32 result on the GPU, scale the
largest reference magnitude and c = 2, the constant that file uses for gradient quantities."""
import math

import pytest
import torch
import torch.nn.functional as F

import tutorial_torch_distributed_data_parallel_amd as tdp
from tutorial_torch_distributed_data_parallel_amd import ops
from tutorial_torch_distributed_data_parallel_amd.ops._grad import SharedGrad, fork

pytestmark = pytest.mark.gpu

U = 2.0 ** -24
C_RULE = 2

# (N, Cin, H, W, Cout, R, stride, pad, groups)
GROUPED = [
    (2, 8, 7, 7, 8, 3, 1, 1, 2),          # minimum Cg = Kg = 4, everything under one tile
    (2, 128, 14, 14, 128, 3, 1, 1, 32),   # ResNeXt shape: a tile spans many groups
    (2, 128, 15, 15, 128, 3, 2, 1, 32),   # stride 2, odd extent, phase with a short tap set
    (2, 16, 9, 7, 24, 3, 1, 1, 2),        # Cg = 8, Kg = 12, non-square image
    (1, 96, 13, 13, 256, 5, 1, 2, 2),     # two-tower AlexNet conv2, Cg = 48, K = 1200
    (2, 64, 6, 6, 64, 1, 1, 0, 4),        # grouped 1x1
    (1, 8, 6, 6, 8, 3, 2, 0, 2),          # a phase with no taps
    (2, 8, 5, 5, 8, 3, 1, 2, 2),          # padding beyond R/2
]
DEPTHWISE = [
    (2, 32, 9, 9, 32, 3, 1, 1, 32),       # baseline depthwise
    (2, 24, 10, 7, 24, 3, 2, 1, 24),      # C not a multiple of 32, stride 2
    (1, 8, 6, 6, 16, 3, 1, 1, 8),         # channel multiplier 2
    (2, 16, 11, 11, 16, 5, 2, 2, 16),     # 5x5, stride 2
    (1, 4, 5, 5, 4, 3, 1, 1, 4),          # minimum C
]
# beyond the issue's list: the stencil's generic form (taps and channels from memory) in both
# directions for a filter that is neither 3x3 nor 5x5, and for a multiplier > 1 at another size
DEPTHWISE_MORE = [
    (1, 8, 9, 9, 8, 7, 2, 3, 8),          # 7x7 stride 2, channel multiplier 1
    (2, 4, 7, 6, 12, 5, 2, 2, 4),         # channel multiplier 3, 5x5 stride 2, non-square
]
WIDE = [GROUPED[1], GROUPED[3], DEPTHWISE[1]]
G_BIAS = [GROUPED[3], DEPTHWISE[1]]
G_SPLIT = (8, 16, 28, 28, 16, 3, 1, 1, 4)  # N*P*Q = 6272


def _ids(g):
    return "x".join(map(str, g))


@pytest.fixture(scope="module")
def C():
    from tutorial_torch_distributed_data_parallel_amd._native import native

    return native()


def _bound(K):
    return (8 + 2 * K ** 0.5) * U


def _out_hw(geom):
    N, Cin, H, W, Cout, R, s, p, g = geom
    return (H + 2 * p - R) // s + 1, (W + 2 * p - R) // s + 1


def _reductions(geom):
    """K of (forward, input gradient, weight gradient)"""
    N, Cin, H, W, Cout, R, s, p, g = geom
    P, Q = _out_hw(geom)
    return R * R * (Cin // g), math.ceil(R / s) ** 2 * (Cout // g), N * P * Q


def _tensors(geom, dist="normal", seed=0):
    N, Cin, H, W, Cout, R, s, p, g = geom
    P, Q = _out_hw(geom)
    gen = torch.Generator(device="cpu").manual_seed(seed + sum(geom))
    ts = [torch.randn(N, Cin, H, W, generator=gen), torch.randn(Cout, Cin // g, R, R, generator=gen),
          torch.randn(N, Cout, P, Q, generator=gen)]
    if dist == "wide":  # 2^[-20, 20] magnitudes
        ts = [t * torch.exp2(torch.randint(-20, 21, t.shape, generator=gen).float()) for t in ts]
    return ts


def _oracle(x, w, dy, geom):
    """float64 (y, dx, dw) of the fp32 operands and their |.| scales, on the CPU"""
    s, p, g = geom[6], geom[7], geom[8]
    cast = lambda t: t.detach().cpu().double()  # noqa: E731
    res = []
    for f in (lambda t: t, torch.abs):
        xr, wr = f(cast(x)).requires_grad_(), f(cast(w)).requires_grad_()
        y = F.conv2d(xr, wr, None, s, p, 1, g)
        y.backward(f(cast(dy)))
        res.append((y.detach(), xr.grad, wr.grad))
    return res


def _scaled_err(out, ref, scale):
    return ((out.double().cpu() - ref).abs() / scale.clamp_min(1e-300)).max().item()


def _param(w):
    """the weight as nn.Conv2d stores it: channels_last when Cg % 4 == 0"""
    w = w.cuda()
    if w.shape[1] % 4 == 0:
        w = w.contiguous(memory_format=torch.channels_last)
    return w.requires_grad_()


def _passes(x, w, dy, geom, bias=None, relu=False):
    """(y, dx, dw[, db]) of ops.conv2d(groups=) on the GPU"""
    s, p, g = geom[6], geom[7], geom[8]
    x = x.cuda().requires_grad_()
    w = _param(w)
    b = None if bias is None else bias.cuda().requires_grad_()
    y = ops.conv2d(x, w, b, s, p, relu=relu, groups=g)
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


def _check_passes(out, ref, scale, geom):
    errs = []
    for name, o, r, sc, K in zip(("forward", "dgrad", "wgrad"), out, ref, scale,
                                 _reductions(geom)):
        assert o.shape == r.shape, (name, o.shape, r.shape)
        e = _scaled_err(o, r, sc)
        print(f"{name}: scaled error {e / U:.2f} u, bound {_bound(K) / U:.2f} u (K = {K})")
        errs.append((name, e, _bound(K)))
    for name, e, b in errs:
        assert e < b, (name, e, b)


@pytest.mark.parametrize("geom", GROUPED + DEPTHWISE + DEPTHWISE_MORE, ids=_ids)
def test_passes_match_float64_oracle(C, reference, geom):
    x, w, dy, (ref, scale) = reference(geom)
    _check_passes(_passes(x, w, dy, geom), ref, scale, geom)


@pytest.mark.parametrize("geom", WIDE, ids=_ids)
def test_passes_wide_magnitudes(C, reference, geom):
    x, w, dy, (ref, scale) = reference(geom, "wide")
    _check_passes(_passes(x, w, dy, geom), ref, scale, geom)


@pytest.mark.parametrize("geom", G_BIAS, ids=_ids)
def test_bias_relu_epilogue_and_masked_backward(C, reference, geom):
    x, w, dy, (ref0, scale0) = reference(geom)
    b = torch.randn(geom[4], generator=torch.Generator().manual_seed(3))
    y, dx, dw, db = _passes(x, w, dy, geom, bias=b, relu=True)
    Kf, Kd, Kw = _reductions(geom)
    # the bias is added in fp32 after the accumulation: one more rounding of the result
    yref = (ref0[0] + b.double().view(1, -1, 1, 1)).clamp_min(0)
    ysc = scale0[0] + b.double().abs().view(1, -1, 1, 1)
    assert _scaled_err(y, yref, ysc) < _bound(Kf) + U
    # backward of the masked gradient g = dy * (y > 0), the mask taken from the kernel's own y
    g = dy * (y.cpu() > 0)
    (ref, scale) = _oracle(x, w, g, geom)
    assert _scaled_err(dx, ref[1], scale[1]) < _bound(Kd)
    assert _scaled_err(dw, ref[2], scale[2]) < _bound(Kw)
    dbref = g.double().sum(dim=(0, 2, 3))
    db32 = g.cuda().sum(dim=(0, 2, 3))
    e_k = (db.double().cpu() - dbref).abs().max().item()
    e_t = (db32.double().cpu() - dbref).abs().max().item()
    sc = dbref.abs().max().item()
    print(f"db: e_k={e_k:.3e} e_t={e_t:.3e} scale={sc:.3e}")
    assert e_k <= 4 * e_t + C_RULE * U * sc


def test_split_weight_gradient_is_deterministic(C, reference):
    geom = G_SPLIT
    N, Cin, H, W, Cout, R, s, p, g = geom
    splits, kps = C.conv_grouped_wgrad_plan([N, Cin, H, W], Cout, R, R, s, s, p, p, g)
    assert splits > 1 and splits * kps >= N * 28 * 28 > (splits - 1) * kps
    x, w, dy, (ref, scale) = reference(geom)
    a = _passes(x, w, dy, geom)
    b = _passes(x, w, dy, geom)
    for name, u, v in zip(("forward", "dgrad", "wgrad"), a, b):
        assert torch.equal(u, v), name
    _check_passes(a, ref, scale, geom)


@pytest.mark.parametrize("geom", [GROUPED[3], GROUPED[2], DEPTHWISE[2]], ids=_ids)
def test_group_isolation(C, geom):
    """Perturbing one group's input channels changes only that group's output channels; the
    same for dy and the input gradient. Everything else stays bitwise equal."""
    N, Cin, H, W, Cout, R, s, p, g = geom
    Cg, Kg = Cin // g, Cout // g
    x, w, dy = _tensors(geom)
    grp = g - 1
    y0, dx0, _ = _passes(x, w, dy, geom)
    x1 = x.clone()
    x1[:, grp * Cg:(grp + 1) * Cg] += 1.0
    y1 = _passes(x1, w, dy, geom)[0]
    other = torch.ones(Cout, dtype=torch.bool)
    other[grp * Kg:(grp + 1) * Kg] = False
    assert torch.equal(y1[:, other], y0[:, other])
    assert not torch.equal(y1[:, ~other], y0[:, ~other])
    dy1 = dy.clone()
    dy1[:, grp * Kg:(grp + 1) * Kg] += 1.0
    dx1 = _passes(x, w, dy1, geom)[1]
    other = torch.ones(Cin, dtype=torch.bool)
    other[grp * Cg:(grp + 1) * Cg] = False
    assert torch.equal(dx1[:, other], dx0[:, other])
    assert not torch.equal(dx1[:, ~other], dx0[:, ~other])


def test_grad_into_shared_buffer(C):
    """Two grouped convolutions of one forked input share a SharedGrad: the first deposits its
    input gradient, the second accumulates into it in the kernel's epilogue. The sum is held to
    the input-gradient bound against the summed scales, plus one rounding for the add."""
    geom = GROUPED[3]
    N, Cin, H, W, Cout, R, s, p, g = geom
    x, w1, dy1 = _tensors(geom, seed=1)
    _, w2, dy2 = _tensors(geom, seed=2)
    (r1, s1), (r2, s2) = _oracle(x, w1, dy1, geom), _oracle(x, w2, dy2, geom)
    xg = x.cuda().requires_grad_()
    sink = SharedGrad()
    xa, xb = fork(xg, sink)
    ya = ops.conv2d(xa, _param(w1), None, s, p, groups=g, grad_into=sink)
    yb = ops.conv2d(xb, _param(w2), None, s, p, groups=g, grad_into=sink)
    ((ya * dy1.cuda()).sum() + (yb * dy2.cuda()).sum()).backward()
    torch.cuda.synchronize()
    Kd = _reductions(geom)[1]
    assert _scaled_err(xg.grad, r1[1] + r2[1], s1[1] + s2[1]) < _bound(Kd) + U
    sep = _passes(x, w1, dy1, geom)[1] + _passes(x, w2, dy2, geom)[1]
    assert torch.equal(xg.grad, sep)  # fp32 addition commutes: either order gives the same bits


@pytest.mark.parametrize("groups", [4, 16], ids=["grouped", "depthwise"])
def test_weight_gradient_lands_in_parameter_layout(C, groups):
    torch.manual_seed(0)
    conv = tdp.nn.Conv2d(16, 16, 3, padding=1, groups=groups, bias=False, device="cuda")
    if groups == 4:
        assert conv.weight.is_contiguous(memory_format=torch.channels_last)
    x = torch.randn(2, 16, 9, 9, device="cuda")
    y = conv(x)
    dy = torch.randn_like(y)
    y.backward(dy)
    assert conv.weight.grad.stride() == conv.weight.stride()
    tmp = torch.empty(16, 3, 3, 16 // groups, device="cuda").permute(0, 3, 1, 2)
    cl = torch.channels_last
    C.conv_grouped_wgrad(dy.contiguous(memory_format=cl), x.contiguous(memory_format=cl), tmp,
                         1, 1, 1, 1, groups)
    torch.cuda.synchronize()
    assert torch.equal(conv.weight.grad, tmp)


def test_unsupported_combinations_raise(C):
    x = torch.randn(1, 4, 5, 5, device="cuda")
    with pytest.raises(NotImplementedError, match="multiples of 4"):  # Cg = 2
        ops.conv2d(x, torch.randn(4, 2, 3, 3, device="cuda"), None, 1, 1, groups=2)
    x6 = torch.randn(1, 6, 5, 5, device="cuda")
    with pytest.raises(NotImplementedError, match="multiple of 4"):   # depthwise, Cin = 6
        ops.conv2d(x6, torch.randn(6, 1, 3, 3, device="cuda"), None, 1, 1, groups=6)
    x8 = torch.randn(1, 8, 7, 7, device="cuda")
    with pytest.raises(NotImplementedError, match="dilation"):
        ops.conv2d(x8, torch.randn(8, 4, 3, 3, device="cuda"), None, 1, 2, groups=2, dilation=2)
    with pytest.raises(NotImplementedError, match="dilation"):
        tdp.nn.Conv2d(8, 8, 3, groups=2, dilation=2)
    # a module built for the GPU refuses at construction, not at its first forward
    with pytest.raises(NotImplementedError, match="multiples of 4"):
        tdp.nn.Conv2d(4, 4, 3, groups=2, device="cuda")


@pytest.mark.parametrize("geom", [GROUPED[3], DEPTHWISE[0]], ids=_ids)
def test_autocast_keeps_grouped_convolution_fp32(C, geom):
    x, w, dy = _tensors(geom)
    plain = _passes(x, w, dy, geom)
    with tdp.autocast():
        inside = _passes(x, w, dy, geom)
    for name, u, v in zip(("forward", "dgrad", "wgrad"), inside, plain):
        assert torch.equal(u, v), name


class _TwinBottleneck(torch.nn.Module):
    """torch.nn twin of models.resnet.Bottleneck (same state_dict keys)"""

    def __init__(self, inplanes, planes, stride, groups, base_width):
        super().__init__()
        nn = torch.nn
        width = int(planes * base_width / 64) * groups
        self.conv1 = nn.Conv2d(inplanes, width, 1, bias=False)
        self.bn1 = nn.BatchNorm2d(width)
        self.conv2 = nn.Conv2d(width, width, 3, stride, 1, groups=groups, bias=False)
        self.bn2 = nn.BatchNorm2d(width)
        self.conv3 = nn.Conv2d(width, planes * 4, 1, bias=False)
        self.bn3 = nn.BatchNorm2d(planes * 4)
        self.downsample = nn.Sequential(nn.Conv2d(inplanes, planes * 4, 1, stride, bias=False),
                                        nn.BatchNorm2d(planes * 4))

    def forward(self, x):
        out = torch.relu(self.bn1(self.conv1(x)))
        out = torch.relu(self.bn2(self.conv2(out)))
        return torch.relu(self.bn3(self.conv3(out)) + self.downsample(x))


def test_resnext_bottleneck_matches_float64_twin(C):
    """ResNeXt's stride-2 block with a 32-group 3x3 in train mode, batch 4 at 12x12, against a
    float64 torch.nn twin with the same weights; output, input gradient and every parameter
    gradient by the hard-inputs rule. The block is Bottleneck(64, 64, ...), ResNeXt-50's own
    first block (width 128, Cg = 4): at planes = 32 torchvision's width rule gives width 64 and
    Cg = 2, which the grouped kernels refuse by design."""
    from tutorial_torch_distributed_data_parallel_amd.models.resnet import Bottleneck
    from tutorial_torch_distributed_data_parallel_amd.nn import BatchNorm2d, Conv2d

    torch.manual_seed(0)
    ds = torch.nn.Sequential(Conv2d(64, 256, 1, stride=2, bias=False), BatchNorm2d(256))
    blk = Bottleneck(64, 64, stride=2, groups=32, base_width=4, downsample=ds).cuda().train()
    assert blk.conv2.groups == 32 and tuple(blk.conv2.weight.shape) == (128, 4, 3, 3)
    sd = {k: v.detach().cpu() for k, v in blk.state_dict().items()}
    t64 = _TwinBottleneck(64, 64, 2, 32, 4).double().train()
    t32 = _TwinBottleneck(64, 64, 2, 32, 4).cuda().train()
    t64.load_state_dict(sd)
    t32.load_state_dict(sd)
    x = torch.randn(4, 64, 12, 12)
    dy = torch.randn(4, 256, 6, 6)

    def run(m, x, dy):
        x = x.clone().requires_grad_()
        y = m(x)
        y.backward(dy)
        return y.detach(), x.grad, {n: p.grad for n, p in m.named_parameters()}

    yk, dxk, gk = run(blk, x.cuda(), dy.cuda())
    yt, dxt, gt = run(t32, x.cuda(), dy.cuda())
    yr, dxr, gr = run(t64, x.double(), dy.double())
    torch.cuda.synchronize()
    bad = []
    for name, k, t, r in [("y", yk, yt, yr), ("dx", dxk, dxt, dxr)] + \
            [(n, gk[n], gt[n], gr[n]) for n in gr]:
        e_k = (k.double().cpu() - r).abs().max().item()
        e_t = (t.double().cpu() - r).abs().max().item()
        sc = r.abs().max().item()
        print(f"[rule] {name}: e_k={e_k:.3e} e_t={e_t:.3e} scale={sc:.3e}")
        if not e_k <= 4 * e_t + C_RULE * U * sc:
            bad.append((name, e_k, e_t, sc))
    assert not bad, bad


@pytest.fixture(scope="module")
def pg():
    if not tdp.parallel.is_initialized():
        tdp.init_process_group("nccl", rank=0, world_size=1, local_rank=0)
    yield tdp
    tdp.destroy_process_group()


def test_three_sgd_steps_under_ddp_match_torch(pg):
    """conv(g=2) + ReLU, depthwise, BatchNorm, Linear: three SGD steps under tdp.DDP (world size
    1, fused optimizer) against the torch.nn twin with torch.optim.SGD, both fp32 on the GPU.
    Tolerance rtol = 1e-4, atol = 1e-5, what tests/test_cnn_gpu.py asks of one block's step. The
    three steps move the parameters by about 2e-2, so a gradient wrong by 0.1 % (2e-5) fails,
    while two correct fp32 implementations differ by gradient rounding, about 1e-5 relative of
    a 2e-2 update, some 1e-7."""
    nn = torch.nn
    torch.manual_seed(0)
    net = nn.Sequential(
        tdp.nn.Conv2d(8, 16, 3, padding=1, groups=2, relu=True, device="cuda"),
        tdp.nn.Conv2d(16, 16, 3, padding=1, groups=16, bias=False, device="cuda"),
        tdp.nn.BatchNorm2d(16, device="cuda"), nn.Flatten(),
        tdp.nn.Linear(16 * 8 * 8, 10, device="cuda")).train()
    twin = nn.Sequential(
        nn.Conv2d(8, 16, 3, padding=1, groups=2), nn.ReLU(),
        nn.Conv2d(16, 16, 3, padding=1, groups=16, bias=False),
        nn.BatchNorm2d(16), nn.Flatten(), nn.Linear(16 * 8 * 8, 10)).cuda().train()
    with torch.no_grad():
        for p, q in zip(net.parameters(), twin.parameters()):
            q.copy_(p)
    ddp = tdp.DDP(net, device_ids=[0])
    opt = tdp.optim.SGD(ddp.parameters(), lr=0.05, momentum=0.9)
    assert ddp.register_fused_optimizer(opt)
    topt = torch.optim.SGD(twin.parameters(), lr=0.05, momentum=0.9)
    gen = torch.Generator().manual_seed(1)
    for _ in range(3):
        x = torch.randn(4, 8, 8, 8, generator=gen).cuda()
        y = torch.randint(0, 10, (4,), generator=gen).cuda()
        opt.zero_grad(set_to_none=True)
        tdp.ops.cross_entropy(ddp(x), y).backward()
        opt.step()
        topt.zero_grad(set_to_none=True)
        F.cross_entropy(twin(x), y).backward()
        topt.step()
    torch.cuda.synchronize()
    for (n, p), q in zip(net.named_parameters(), twin.parameters()):
        print(f"{n}: max |diff| {(p.detach() - q.detach()).abs().max().item():.3e}")
    for (n, p), q in zip(net.named_parameters(), twin.parameters()):
        torch.testing.assert_close(p.detach(), q.detach(), rtol=1e-4, atol=1e-5,
                                   msg=lambda m: f"{n}: {m}")
    del ddp
