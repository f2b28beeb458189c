"""The GroupNorm kernels (csrc/groupnorm.hip) on the device: both layout forms, forward and every
gradient, against a float64 CPU reference computed from the same fp32 inputs.

Tolerance rule (that of tests/test_hard_inputs_gpu.py). For a quantity q: e_k = max|q_kernel -
q_f64|, e_t = the same for torch's own fp32 ``F.group_norm`` on the GPU, and the assertion is

    e_k <= 4 * e_t + c * 2**-24 * scale,    scale = max|q_f64|

with one ``c`` per quantity (``C_``). No bound is derived from the kernel's own output.

c was chosen after the first MI355X run of this file as the smallest integer >= 1 covering the
largest figure (e_k - 4 e_t) / (2**-24 scale) any case needed:

    quantity  c  needed  case                                    e_k      e_t      scale
    y         1  -4.58   nhwc (2,8,3,3,2) affine                 3.7e-7   3.7e-7   4.09
    dx        1  -2.22   generic (2,8,7) G=2 affine relu         3.6e-7   2.0e-7   3.41
    dw        1  -0.72   generic (1,4,64,65,1) affine relu       1.1e-5   3.2e-6   31.9
    db        1   0.00   nhwc (1,32,1,1,8) affine (e_k = e_t = 0; elsewhere negative)

(a negative "needed": 4 e_t alone covered every case.)"""
import pytest
import torch
import torch.nn as nn
import torch.nn.functional as F

import tutorial_torch_distributed_data_parallel_amd as tdp
from tutorial_torch_distributed_data_parallel_amd import ops

pytestmark = pytest.mark.gpu

U = 2.0 ** -24
C_ = {"y": 1, "dx": 1, "dw": 1, "db": 1}

NHWC = [(2, 8, 3, 3, 2),        # Cg = 4
        (3, 64, 5, 7, 32),      # Cg = 2: a 16-byte load spans two groups
        (2, 12, 4, 4, 12),      # Cg = 1
        (2, 24, 9, 9, 3),       # Cg = 8: a group spans two loads
        (1, 32, 1, 1, 8),       # one pixel
        (2, 2048, 2, 2, 32),    # more 4-channel columns than a workgroup has threads
        (2, 16, 37, 41, 4)]     # 1517 pixels > the 1024 of one part: split and merged
GENERIC = [(2, 6, 5, 5, 3),     # NCHW, C % 4 != 0
           (2, 10, 3, 3, 5),    # odd run length 18
           (2, 8, 7, 2),        # 3-D [N, C, L]
           (4, 12, 3),          # 2-D [N, C]
           (1, 4, 64, 65, 1)]   # one long run (16640 floats: 5 parts)


def _err(a, ref):
    a, ref = a.detach().double().cpu(), ref.detach().double().cpu()
    assert a.shape == ref.shape, (a.shape, ref.shape)
    d = (a - ref).abs()
    d = torch.where(a == ref, torch.zeros_like(d), d)
    return d.max().item() if not torch.isnan(d).any() else float("nan")


def _rule(what, got, t32, ref, c):
    """Assert the module's tolerance rule for one quantity; prints the figures first."""
    e_k, e_t = _err(got, ref), _err(t32, ref)
    scale = ref.detach().double().abs().max().item()
    bound = 4 * e_t + c * U * scale
    need = (e_k - 4 * e_t) / (U * scale) if scale > 0 else 0.0
    print(f"[rule] {what}: e_k={e_k:.3e} e_t={e_t:.3e} c={c} scale={scale:.3e} "
          f"bound={bound:.3e} needed={need:.2f}")
    assert e_k <= bound, f"{what}: e_k {e_k:.3e} > 4 * {e_t:.3e} + {c} * 2^-24 * {scale:.3e}"


def _split(case):
    *dims, G = case
    return tuple(dims), G


def _make(shape, seed=0, x=None):
    g = torch.Generator().manual_seed(seed)
    C = shape[1]
    x = torch.randn(shape, generator=g) if x is None else x
    return dict(x=x, w=torch.empty(C).uniform_(0.5, 2, generator=g),
                b=torch.empty(C).uniform_(-1, 1, generator=g),
                res=torch.randn(shape, generator=g), dy=torch.randn(shape, generator=g))


def _place(t, nhwc, offset=False):
    t = t.cuda()
    if nhwc and t.dim() == 4:
        return t.contiguous(memory_format=torch.channels_last)
    if offset:  # a contiguous view that starts 4 bytes into its storage
        buf = torch.empty(t.numel() + 1, device="cuda")
        buf[1:].copy_(t.flatten())
        t = buf[1:].view(t.shape)
        assert t.data_ptr() % 16 == 4 and t.is_contiguous()
    return t


def _torch(d, G, affine, relu, residual, dtype, dev, nhwc=False):
    """(y, dx, dw, db, dres) of F.group_norm (+ residual, + relu) in ``dtype`` on ``dev``."""
    def put(t):
        t = t.to(device=dev, dtype=dtype)
        return _place(t, True) if (nhwc and dev == "cuda") else t

    x, res = put(d["x"]).requires_grad_(), put(d["res"]).requires_grad_()
    w = put(d["w"]).requires_grad_() if affine else None
    b = put(d["b"]).requires_grad_() if affine else None
    z = F.group_norm(x, G, w, b)
    z = z + res if residual else z
    y = F.relu(z) if relu else z
    y.backward(put(d["dy"]))
    return (y.detach(), x.grad, w.grad if affine else None, b.grad if affine else None,
            res.grad if residual else None)


def _kernel(d, G, affine, relu, residual, nhwc, offset=False, sink=None):
    x = _place(d["x"], nhwc, offset).requires_grad_()
    res = _place(d["res"], nhwc).requires_grad_() if residual else None
    w = d["w"].cuda().requires_grad_() if affine else None
    b = d["b"].cuda().requires_grad_() if affine else None
    y = ops.group_norm(x, G, w, b, relu=relu, residual=res, residual_grad_into=sink)
    if nhwc:
        assert y.is_contiguous(memory_format=torch.channels_last)
    y.backward(_place(d["dy"], nhwc))
    return (y.detach(), x.grad, w.grad if affine else None, b.grad if affine else None,
            res.grad if residual else None)


_REFS = {}


def _refs(key, d, G, affine, relu, residual, nhwc):
    """float64 CPU reference and torch's fp32 GPU result of one case, computed once."""
    k = (key, G, affine, relu, residual, nhwc)
    if k not in _REFS:
        _REFS[k] = (_torch(d, G, affine, relu, residual, torch.float64, "cpu"),
                    _torch(d, G, affine, relu, residual, torch.float32, "cuda", nhwc))
    return _REFS[k]


def _check(tag, d, G, affine, relu, residual, nhwc, offset=False):
    r64, r32 = _refs(tag, d, G, affine, relu, residual, nhwc)
    got = _kernel(d, G, affine, relu, residual, nhwc, offset)
    for name, i in (("y", 0), ("dx", 1), ("dw", 2), ("db", 3)):
        if got[i] is None:
            assert r64[i] is None
            continue
        _rule(f"{tag} affine={affine} relu={relu} {name}", got[i], r32[i], r64[i], C_[name])
    return got, r64


@pytest.mark.parametrize("case", NHWC, ids=lambda c: "x".join(map(str, c)))
@pytest.mark.parametrize("affine", [True, False])
@pytest.mark.parametrize("relu", [False, True])
def test_nhwc_form(case, affine, relu):
    shape, G = _split(case)
    _check(f"nhwc{case}", _make(shape), G, affine, relu, False, True)


@pytest.mark.parametrize("case", GENERIC, ids=lambda c: "x".join(map(str, c)))
@pytest.mark.parametrize("affine", [True, False])
@pytest.mark.parametrize("relu", [False, True])
def test_generic_form(case, affine, relu):
    shape, G = _split(case)
    _check(f"gen{case}", _make(shape), G, affine, relu, False, False)


@pytest.mark.parametrize("affine", [True, False])
@pytest.mark.parametrize("relu", [False, True])
def test_generic_form_view_at_a_4_byte_offset(affine, relu):
    _check("gen-offset(2,8,3,3,2)", _make((2, 8, 3, 3)), 2, affine, relu, False, False,
           offset=True)


@pytest.mark.parametrize("case, nhwc", [((2, 16, 6, 6, 4), True), ((2, 6, 5, 5, 3), False)])
def test_fused_residual(case, nhwc):
    """relu(gn(x) + r): dx by the rule; dres is the ReLU-masked dy itself, also when it is
    deposited through a SharedGrad."""
    from tutorial_torch_distributed_data_parallel_amd.ops._grad import SharedGrad

    shape, G = _split(case)
    d = _make(shape)
    got, r64 = _check(f"res{case}", d, G, True, True, True, nhwc)
    y, dres = got[0], got[4]
    masked = torch.where(y > 0, d["dy"].cuda(), torch.zeros_like(y))
    assert torch.equal(dres, masked)
    assert (y == 0).any() and (y > 0).any()
    sink = SharedGrad()
    again = _kernel(d, G, True, True, True, nhwc, sink=sink)
    assert torch.equal(again[4], masked) and torch.equal(again[1], got[1])
    assert sink.buf is not None and torch.equal(sink.buf, masked)


# ------------------------------------------------------------------------------- hard inputs
@pytest.mark.parametrize("nhwc", [True, False])
@pytest.mark.parametrize("kind", ["100+randn", "1000+0.01randn"])
def test_large_mean_small_spread(kind, nhwc):
    """E[x^2] - E[x]^2 would lose every digit of these variances."""
    shape, G = (3, 64, 5, 7), 32
    g = torch.Generator().manual_seed(3)
    r = torch.randn(shape, generator=g)
    x = 100 + r if kind == "100+randn" else 1000 + 0.01 * r
    _check(f"hard[{kind}] nhwc={nhwc}", _make(shape, x=x), G, True, False, False, nhwc)
    _check(f"hard[{kind}] nhwc={nhwc}", _make(shape, x=x), G, True, True, False, nhwc)


@pytest.mark.parametrize("nhwc", [True, False])
def test_constant_group(nhwc):
    """One (sample, group) constant: variance 0, y = b exactly there, dx finite; the rest by the
    rule."""
    shape, G = (2, 16, 6, 6), 4
    d = _make(shape)
    d["x"][1, 4:8] = 3.25
    got, _ = _check(f"const nhwc={nhwc}", d, G, True, False, False, nhwc)
    y, dx = got[0], got[1]
    assert torch.equal(y[1, 4:8], d["b"].cuda()[4:8].view(4, 1, 1).expand(4, 6, 6))
    assert bool(torch.isfinite(dx).all())


@pytest.mark.parametrize("nhwc", [True, False])
def test_nan_stays_in_its_group(nhwc):
    shape, G = (3, 16, 4, 4), 4
    d = _make(shape)
    d["x"][1, 9, 2, 1] = float("nan")
    clean = _make(shape)
    clean["x"][1, 8:12] = 0.0  # what the other groups must still equal
    y, dx, dw, db, _ = _kernel(d, G, True, False, False, nhwc)
    yc, dxc, _, _, _ = _kernel(clean, G, True, False, False, nhwc)
    hit = torch.zeros(shape, dtype=torch.bool, device="cuda")
    hit[1, 8:12] = True
    assert bool(torch.isnan(y[hit]).all()) and bool(torch.isnan(dx[hit]).all())
    assert torch.equal(y[~hit], yc[~hit]) and torch.equal(dx[~hit], dxc[~hit])
    ch = torch.zeros(16, dtype=torch.bool, device="cuda")
    ch[8:12] = True
    # dw = sum g xhat carries the NaN in the group's channels; db = sum g never reads x
    assert bool(torch.isnan(dw[ch]).all())
    assert bool(torch.isfinite(dw[~ch]).all()) and bool(torch.isfinite(db[~ch]).all())


# -------------------------------------------------------------------------- exact properties
FORMS = [((3, 64, 5, 7), 32, True), ((3, 16, 37, 41), 4, True), ((3, 6, 5, 5), 3, False),
         ((3, 4, 64, 65), 1, False)]


@pytest.mark.parametrize("shape, G, nhwc", FORMS)
def test_relu_is_the_clamp_and_calls_repeat_bitwise(shape, G, nhwc):
    d = _make(shape)
    plain = _kernel(d, G, True, False, False, nhwc)
    a = _kernel(d, G, True, True, False, nhwc)
    b = _kernel(d, G, True, True, False, nhwc)
    assert torch.equal(a[0], plain[0].clamp_min(0))
    for p, q in zip(a[:4], b[:4]):
        assert torch.equal(p, q)
    # grad disabled: the same forward, nothing saved
    with torch.no_grad():
        y = ops.group_norm(_place(d["x"], nhwc), G, d["w"].cuda(), d["b"].cuda(), relu=True)
    assert torch.equal(y, a[0]) and y.grad_fn is None
    # inside autocast the op stays fp32 and bitwise the same
    with tdp.autocast():
        c = _kernel(d, G, True, True, False, nhwc)
    assert c[0].dtype == torch.float32
    for p, q in zip(a[:4], c[:4]):
        assert torch.equal(p, q)


@pytest.mark.parametrize("shape, G, nhwc", FORMS)
def test_a_sample_does_not_see_its_batch(shape, G, nhwc):
    """y[n] and dx[n] of a batch of 3 equal the sample run alone, bit for bit."""
    d = _make(shape)
    y, dx, _, _, _ = _kernel(d, G, True, True, False, nhwc)
    for n in range(shape[0]):
        one = {k: (v[n:n + 1].clone() if v.dim() == len(shape) else v) for k, v in d.items()}
        y1, dx1, _, _, _ = _kernel(one, G, True, True, False, nhwc)
        assert torch.equal(y[n:n + 1], y1) and torch.equal(dx[n:n + 1], dx1)


# ------------------------------------------------------------------------------ other checks
def test_graph_capture_replays_bitwise():
    torch.manual_seed(0)
    m = tdp.nn.GroupNorm(4, 16, relu=True).cuda()
    with torch.no_grad():
        m.weight.uniform_(0.5, 2)
        m.bias.uniform_(-1, 1)
    xs = torch.zeros(2, 16, 6, 6, device="cuda").contiguous(memory_format=torch.channels_last)
    xs.requires_grad_()
    gs = torch.zeros_like(xs)

    def step():
        y = m(xs)
        dx, dw, db = torch.autograd.grad(y, (xs, m.weight, m.bias), gs)
        return y, dx, dw, db

    inputs = [(torch.randn_like(xs), torch.randn_like(xs)) for _ in range(3)]
    with torch.no_grad():
        xs.copy_(inputs[0][0])
        gs.copy_(inputs[0][1])
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        step()  # warm-up on the capture stream
    torch.cuda.current_stream().wait_stream(side)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph, stream=side):
        outs = step()
    for xv, gv in inputs[1:]:
        with torch.no_grad():
            xs.copy_(xv)
            gs.copy_(gv)
        graph.replay()
        torch.cuda.synchronize()
        got = [o.clone() for o in outs]
        eager = step()
        for p, q in zip(got, eager):
            assert torch.equal(p, q)


def _cut_down_pair():
    from tutorial_torch_distributed_data_parallel_amd.models.resnet import ResNet
    from groupnorm_twin import TwinResNetGN

    torch.manual_seed(0)

    def norm(c, relu=False, device=None):
        return tdp.nn.GroupNorm(32, c, relu=relu, device=device)

    m = ResNet((1, 1, 1, 1), num_classes=10, norm_layer=norm)
    for g in m.modules():
        if isinstance(g, nn.GroupNorm):
            nn.init.uniform_(g.weight, 0.5, 1.5)
            nn.init.uniform_(g.bias, -0.5, 0.5)
    t = TwinResNetGN((1, 1, 1, 1), num_classes=10)
    t.load_state_dict(m.state_dict())
    return m.cuda(), t.cuda()


def test_cut_down_resnet50_gn_matches_its_twin_on_the_device():
    """One forward / backward against the fp32 torch.nn twin on the GPU, at the tolerances of
    tests/test_cnn_gpu.py's ResNet block comparison (1e-5 on the output, 1e-4 on gradients)."""
    m, t = _cut_down_pair()
    x = torch.randn(2, 3, 32, 32, device="cuda")
    xm, xt = x.clone().requires_grad_(), x.clone().requires_grad_()
    y, yt = m(xm), t(xt)
    print(f"[model] |y - yt| max {(y - yt).abs().max().item():.3e} of {yt.abs().max().item():.3e}")
    g = torch.randn_like(yt)
    y.backward(g)
    yt.backward(g)
    worst = max(((p.grad - q.grad).abs().max() / q.grad.abs().max().clamp_min(1e-30)).item()
                for p, q in zip(m.parameters(), t.parameters()))
    print(f"[model] worst relative gradient difference {worst:.3e}")
    torch.testing.assert_close(y, yt, atol=1e-5, rtol=1e-5)
    torch.testing.assert_close(xm.grad, xt.grad, atol=1e-4, rtol=1e-4)
    for (n, p), q in zip(m.named_parameters(), t.parameters()):
        torch.testing.assert_close(p.grad, q.grad, atol=1e-4, rtol=1e-4,
                                   msg=lambda s: f"{n}: {s}")


@pytest.fixture()
def pg():
    from tutorial_torch_distributed_data_parallel_amd.parallel import runtime as rt

    if tdp.parallel.is_initialized() and rt.get_backend() != "nccl":
        tdp.destroy_process_group()
    if not tdp.parallel.is_initialized():
        tdp.init_process_group("nccl", rank=0, world_size=1, local_rank=0)
    yield tdp
    tdp.destroy_process_group()


def test_cut_down_resnet50_gn_trains_under_ddp(pg):
    m, _ = _cut_down_pair()
    ddp = tdp.DDP(m)
    opt = tdp.optim.SGD(ddp.parameters(), lr=0.003)
    g = torch.Generator().manual_seed(5)
    x = torch.randn(4, 3, 32, 32, generator=g).cuda()
    y = torch.randint(0, 10, (4,), generator=g).cuda()
    losses = []
    for _ in range(4):
        opt.zero_grad()
        loss = tdp.ops.cross_entropy(ddp(x), y)
        loss.backward()
        opt.step()
        losses.append(loss.item())
    print("[model] losses", losses)
    assert all(torch.isfinite(torch.tensor(losses)))
    assert losses[3] < losses[0]  # the loss after 3 steps


def test_errors():
    with pytest.raises(TypeError, match="float32"):
        ops.group_norm(torch.randn(2, 8, 3, 3, device="cuda", dtype=torch.float64), 2)
    with pytest.raises(TypeError, match="float32"):
        ops.group_norm(torch.randn(2, 8, 3, 3, device="cuda").bfloat16(), 2)
    with pytest.raises(ValueError, match="not divisible"):
        ops.group_norm(torch.randn(2, 6, 3, 3, device="cuda"), 4)
    with pytest.raises(ValueError, match="at least 2D"):
        ops.group_norm(torch.randn(8, device="cuda"), 2)
