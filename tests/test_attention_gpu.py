"""The fused attention kernels (csrc/attention.hip) on the device against a float64 evaluation of
the same fp32 inputs. Tile sizes built: 128 own rows a workgroup (32 a wave), 64-row walked tiles.

Tolerance rule (that of tests/test_hard_inputs_gpu.py). For a quantity x: e_k = max|x_kernel -
x_f64|, e_t = the same for the plain fp32 torch composition ``softmax((q @ k^T) * scale) @ v`` and
its autograd on the GPU, and the assertion is

    e_k <= 4 * e_t + c * 2**-24 * scale,   scale = max|v| for o, max|x_f64| for the gradients

with c = 2 for every quantity (``C_``). No bound is derived from the kernel's own output.

c = 2 was never exceeded. On an MI355X, the largest (e_k - 4 e_t) / (2**-24 scale) per quantity
over the numerics cases (negative: 4 e_t alone covered it):

    quantity  c  needed  case              e_k      e_t      scale
    o         2   0.00   D=32 (1,1)        0        0        3.39   (elsewhere <= -2.62)
    dq        2  -7.94   D=32 (5,7)        2.4e-7   2.1e-7   1.28
    dk        2  -4.16   D=64 (5,7)        3.3e-7   2.1e-7   1.98
    dv        2  -3.27   D=32 (5,7)        6.6e-7   2.8e-7   2.25
    hard rows: o -2.86 (huge-column: e_k 0.173, e_t 0.187, scale 3.4e6); dq / dk / dv <= -17

The (1, 1) cases have dq = dk = 0 exactly in float64 and in torch's composition, so their bound is
0: the kernels meet it (e_k = 0) because delta is the diagonal of the same six-product MFMA GEMM
that forms dP (csrc/attention.hip, the delta kernel). With delta as a plain fp32 dot product dq
came out at 6.6e-8 (D = 32) and 7.4e-7 (D = 64).
"""
import pytest
import torch

import tutorial_torch_distributed_data_parallel_amd as tdp
from tutorial_torch_distributed_data_parallel_amd import ops

pytestmark = pytest.mark.gpu

U = 2.0 ** -24
C_ = {"o": 2, "dq": 2, "dk": 2, "dv": 2}
B, H = 2, 3
SHAPES = [(1, 1), (5, 7),   # below one tile in both dimensions
          (128, 64),        # exactly one query tile and one key tile
          (33, 65),         # ragged last tile in each dimension
          (197, 197),       # ViT's length: 2 query tiles, 4 key tiles, ragged tails
          (130, 70)]        # cross shape


def _err(a, ref):
    a, ref = a.detach().double().cpu(), ref.detach().double().cpu()
    assert a.shape == ref.shape, (a.shape, ref.shape)
    d = (a - ref).abs()
    d = torch.where(a == ref, torch.zeros_like(d), d)
    return d.max().item() if not torch.isnan(d).any() else float("nan")


def _rule(what, got, t32, ref, c, scale):
    e_k, e_t = _err(got, ref), _err(t32, ref)
    bound = 4 * e_t + c * U * scale
    need = (e_k - 4 * e_t) / (U * scale) if scale > 0 else 0.0
    print(f"[rule] {what}: e_k={e_k:.3e} e_t={e_t:.3e} c={c} scale={scale:.3e} "
          f"bound={bound:.3e} needed={need:.2f}")
    assert bool(torch.isfinite(got).all()), f"{what}: not finite"
    assert e_k <= bound, f"{what}: e_k {e_k:.3e} > 4 * {e_t:.3e} + {c} * 2^-24 * {scale:.3e}"


def _packed(Sq, Sk, D, seed=0):
    """One [B, S, 3, H, D] buffer (S = max(Sq, Sk)); q, k, v and dO as CPU tensors."""
    g = torch.Generator().manual_seed(seed)
    buf = torch.randn(B, max(Sq, Sk), 3, H, D, generator=g)
    return buf, torch.randn(B, H, Sq, D, generator=g)


def _views(buf, Sq, Sk):
    """q [B, H, Sq, D], k and v [B, H, Sk, D]: strided views of the packed buffer."""
    q, k, v = buf.permute(2, 0, 3, 1, 4).unbind(0)
    return q[:, :, :Sq], k[:, :, :Sk], v[:, :, :Sk]


def _composition(q, k, v, do, dtype, dev):
    """(o, dq, dk, dv) of the plain torch composition in ``dtype`` on ``dev``."""
    q, k, v = (t.to(device=dev, dtype=dtype).contiguous().requires_grad_() for t in (q, k, v))
    o = torch.softmax((q @ k.transpose(-1, -2)) * q.shape[-1] ** -0.5, dim=-1) @ v
    o.backward(do.to(device=dev, dtype=dtype))
    return o.detach(), q.grad, k.grad, v.grad


def _kernel(buf, do, Sq, Sk):
    """(o, dq, dk, dv) of ops.scaled_dot_product_attention on strided views."""
    buf = buf.cuda().requires_grad_()
    q, k, v = _views(buf, Sq, Sk)
    assert not q.is_contiguous()
    o = ops.scaled_dot_product_attention(q, k, v)
    assert o.transpose(1, 2).is_contiguous()  # memory is [B, Sq, H, D]
    dq, dk, dv = torch.autograd.grad(o, (q, k, v), do.cuda())
    return o.detach(), dq, dk, dv


def _check(tag, buf, do, Sq, Sk):
    q, k, v = _views(buf, Sq, Sk)
    r64 = _composition(q, k, v, do, torch.float64, "cpu")
    r32 = _composition(q, k, v, do, torch.float32, "cuda")
    got = _kernel(buf, do, Sq, Sk)
    for name, g, t, r in zip(("o", "dq", "dk", "dv"), got, r32, r64):
        scale = v.abs().max().item() if name == "o" else r.abs().max().item()
        _rule(f"{tag} {name}", g, t, r, C_[name], scale)
    return got


@pytest.mark.parametrize("Sq, Sk", SHAPES)
@pytest.mark.parametrize("D", [32, 64])
def test_numerics_and_packed_form(D, Sq, Sk):
    buf, do = _packed(Sq, Sk, D)
    o, dq, dk, dv = _check(f"D={D} ({Sq},{Sk})", buf, do, Sq, Sk)
    if Sq != Sk:
        return  # the packed form is self-attention
    qkv = buf.reshape(B, Sq, 3 * H * D).cuda().requires_grad_()
    y = ops.attention_qkvpacked(qkv, H)
    assert y.shape == (B, Sq, H * D) and y.is_contiguous()
    y.backward(do.cuda().transpose(1, 2).reshape(B, Sq, H * D))
    assert torch.equal(y, o.transpose(1, 2).reshape(B, Sq, H * D))
    gq, gk, gv = qkv.grad.view(B, Sq, 3, H, D).permute(2, 0, 3, 1, 4).unbind(0)
    assert qkv.grad.is_contiguous()
    assert torch.equal(gq, dq) and torch.equal(gk, dk) and torch.equal(gv, dv)


@pytest.mark.parametrize("kind", ["one-hot", "equal-scores", "rescale-underflow", "huge-column"])
def test_hard_rows(kind):
    """Sq = 70, Sk = 197 (four key tiles), D = 64; finite and within the rule."""
    Sq, Sk, D = 70, 197, 64
    buf, do = _packed(Sq, Sk, D, seed=2)
    q, k, v = _views(buf, Sq, Sk)
    if kind == "one-hot":
        q *= 1e3 / 8  # scores reach ~1e3 after the D ** -0.5 scale
    elif kind == "equal-scores":
        q[0, 1, 2] = 0.0
        q[1, 2, 69] = 0.0
    elif kind == "rescale-underflow":
        # tiles 0, 2, 3 score ~ -200 and tile 1 ~ +200: entering tile 1 the rescale factor
        # exp(-400) underflows to 0, and tiles 2, 3 have probability 0
        q[..., 0] = 40.0
        k[..., 0] = -40.0
        k[:, :, 64:128, 0] = 40.0
    else:
        v[..., 3] *= 1e6
    _check(f"hard[{kind}]", buf, do, Sq, Sk)


@pytest.mark.parametrize("D, Sq, Sk", [(64, 197, 197), (32, 130, 70)])
def test_repeats_bitwise_and_a_sample_does_not_see_its_batch(D, Sq, Sk):
    buf, do = _packed(Sq, Sk, D, seed=3)
    a, b = _kernel(buf, do, Sq, Sk), _kernel(buf, do, Sq, Sk)
    assert all(torch.equal(x, y) for x, y in zip(a, b))
    q, k, v = (t[1:2].cuda().requires_grad_() for t in _views(buf, Sq, Sk))
    o = ops.scaled_dot_product_attention(q, k, v)
    alone = (o.detach(), *torch.autograd.grad(o, (q, k, v), do[1:2].cuda()))
    assert all(torch.equal(x[1:2], y) for x, y in zip(a, alone))
    with tdp.autocast():  # the core stays fp32, bitwise
        c = _kernel(buf, do, Sq, Sk)
    assert all(torch.equal(x, y) for x, y in zip(a, c))


def test_views_the_kernels_cannot_read_get_the_native_copy():
    """Inner stride 2 and a 4-byte offset: one attn_copy4d each, the same result bitwise."""
    Sq, Sk, D = 33, 65, 32
    buf, do = _packed(Sq, Sk, D, seed=4)
    ref = _kernel(buf, do, Sq, Sk)
    q, k, v = (t.cuda() for t in _views(buf, Sq, Sk))
    q2 = torch.empty(B, H, Sq, 2 * D, device="cuda")[..., ::2].copy_(q).requires_grad_()
    k2 = torch.empty(k.numel() + 1, device="cuda")[1:].view(B, H, Sk, D).copy_(k).requires_grad_()
    assert q2.stride(3) == 2 and k2.data_ptr() % 16 == 4
    o = ops.scaled_dot_product_attention(q2, k2, v)
    dq, dk = torch.autograd.grad(o, (q2, k2), do.cuda())
    assert torch.equal(o, ref[0]) and torch.equal(dq, ref[1]) and torch.equal(dk, ref[2])


def test_errors():
    q = torch.randn(1, 2, 5, 32, device="cuda")
    with pytest.raises(TypeError, match="float32"):
        ops.scaled_dot_product_attention(q.double(), q.double(), q.double())
    with pytest.raises(TypeError, match="float32"):
        ops.attention_qkvpacked(torch.randn(1, 5, 192, device="cuda").bfloat16(), 2)
    with pytest.raises(NotImplementedError, match="32 and 64"):
        ops.scaled_dot_product_attention(q[..., :16], q[..., :16], q[..., :16])
    big = torch.zeros(1, 1, 1, 32, device="cuda").expand(65536, 1, 1, 32)
    with pytest.raises(ValueError, match="65535"):
        ops.scaled_dot_product_attention(big, big, big)


def test_module_matches_its_torch_twin_and_trains():
    """E = 64, H = 2, B = 2, S = 5 against torch.nn.MultiheadAttention in fp32 on the GPU, at the
    tolerances of test_groupnorm_gpu.py's model test (1e-5 output, 1e-4 gradients).
    Measured: |y - yt| max 1.8e-7 of 0.78; worst relative gradient difference 2.5e-7: the twin is
    well inside both figures."""
    torch.manual_seed(0)
    m = tdp.nn.MultiheadAttention(64, 2, device="cuda")
    t = torch.nn.MultiheadAttention(64, 2, batch_first=True, device="cuda")
    with torch.no_grad():
        for n, p in m.named_parameters():
            if n.endswith("bias"):  # initialised to zero
                p.uniform_(-0.1, 0.1)
    t.load_state_dict(m.state_dict())
    x = torch.randn(2, 5, 64, device="cuda")
    xm, xt = x.clone().requires_grad_(), x.clone().requires_grad_()
    y, w = m(xm)
    yt, _ = t(xt, xt, xt, need_weights=False)
    assert w is None
    g = torch.randn_like(yt)
    y.backward(g)
    yt.backward(g)
    print(f"[module] |y - yt| max {(y - yt).abs().max().item():.3e} of {yt.abs().max().item():.3e}")
    worst = max(((p.grad - q.grad).abs().max() / q.grad.abs().max()).item()
                for p, q in zip(m.parameters(), t.parameters()))
    print(f"[module] worst relative gradient difference {worst:.3e}")
    torch.testing.assert_close(y, yt, atol=1e-5, rtol=1e-5)
    torch.testing.assert_close(xm.grad, xt.grad, atol=1e-4, rtol=1e-4)
    for (n, p), q in zip(m.named_parameters(), t.parameters()):
        torch.testing.assert_close(p.grad, q.grad, atol=1e-4, rtol=1e-4, msg=lambda s: f"{n}: {s}")
    before = [p.detach().clone() for p in m.parameters()]
    tdp.optim.SGD(m.parameters(), lr=0.1).step()
    assert len(before) == 4 and all(not torch.equal(p, b) for p, b in zip(m.parameters(), before))


def test_graph_capture_replays_bitwise():
    Bc, S, Hc, D = 2, 70, 2, 64
    xs = torch.zeros(Bc, S, 3 * Hc * D, device="cuda", requires_grad=True)
    gs = torch.zeros(Bc, S, Hc * D, device="cuda")

    def step():
        y = ops.attention_qkvpacked(xs, Hc)
        (dx,) = torch.autograd.grad(y, (xs,), gs)
        return y, dx

    inputs = [(torch.randn_like(xs), torch.randn_like(gs)) for _ in range(3)]
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
    for xv, gv in inputs:
        with torch.no_grad():
            xs.copy_(xv)
            gs.copy_(gv)
        graph.replay()
        torch.cuda.synchronize()
        got = [o.clone() for o in outs]
        eager = step()
        for p, q in zip(got, eager):
            assert torch.equal(p, q)
