"""The weight-standardisation kernels (csrc/weight_std.hip) on the device against the float64
composition of the same fp32 inputs, by the tolerance rule of tests/test_groupnorm_gpu.py at
c = 1 for both quantities:

    e_k <= 4 * e_t + 2**-24 * scale,    scale = max|q_f64|

e_k the kernel's error, e_t that of the same composition in torch fp32 on the GPU. Where the
exact result is (nearly) zero -- ``g`` a multiple of ``w_hat`` plus a constant -- ``scale`` is
max|rstd * g|, the size of the terms that cancel. Every figure is printed before it is asserted."""
import pytest
import torch

import tutorial_torch_distributed_data_parallel_amd as tdp
from tutorial_torch_distributed_data_parallel_amd import ops
from tutorial_torch_distributed_data_parallel_amd._native import native

import weight_std_workers as W  # noqa: E402  (tests/ is on sys.path via conftest)

pytestmark = pytest.mark.gpu

U = 2.0 ** -24
CL, NCHW, OFF = "channels_last", "contiguous", "channels_last+4B"
CASES = [((5, 4, 1, 1), CL),      # K = 4; a tail block of one row
         ((8, 1, 3, 3), CL),      # K = 9
         ((6, 16, 1, 1), CL),     # K = 64: one float per lane
         ((7, 3, 7, 7), NCHW),    # K = 147: scalar form
         ((5, 8, 3, 3), OFF),     # unaligned base: scalar form
         ((3, 512, 3, 3), CL),    # K = 4608: at the register cap
         ("cap+4", CL)]           # [2, cap/4 + 1, 2, 2]: the first row length past the cap


def _place(t, layout):
    t = t.cuda()
    if layout == NCHW:
        return t.contiguous()
    t = t.contiguous(memory_format=torch.channels_last)
    if layout == OFF:  # the same layout, viewed 4 bytes into its storage
        buf = torch.empty(t.numel() + 1, device="cuda")
        v = buf.as_strided(t.shape, t.stride(), 1)
        v.copy_(t)
        assert v.data_ptr() % 16 == 4
        return v
    return t


def _run(fn, w, g, layout):
    """(w_hat, dw) of ``fn`` on the placed weight."""
    w = _place(w, layout).requires_grad_()
    y = fn(w)
    assert y.stride() == w.stride()
    return y.detach(), torch.autograd.grad(y, w, _place(g, layout))[0]


def _rule(what, got, t32, ref, scale=None):
    def err(a):
        a = a.double().cpu()
        return torch.where(a == ref, torch.zeros_like(ref), (a - ref).abs()).max().item()

    e_k, e_t = err(got), err(t32)
    scale = ref.abs().max().item() if scale is None else scale
    print(f"[rule] {what}: e_k={e_k:.3e} e_t={e_t:.3e} scale={scale:.3e} "
          f"needed={(e_k - 4 * e_t) / (U * scale) if scale > 0 else 0.0:.2f}")
    assert bool(torch.isfinite(got).all()), what
    assert e_k <= 4 * e_t + U * scale, f"{what}: e_k {e_k:.3e} > 4 * {e_t:.3e} + 2^-24 * {scale:.3e}"


def _check(tag, w, g, layout, rows=None, dw_scale=None):
    got, t32 = _run(ops.weight_standardize, w, g, layout), _run(W.compose, w, g, layout)
    wd = w.double().requires_grad_()
    ref = W.compose(wd)
    ref = (ref.detach(), torch.autograd.grad(ref, wd, g.double())[0])
    for o in (range(w.shape[0]) if rows else [slice(None)]):  # per row where the rows differ in size
        row = f" row {o}" if rows else ""
        _rule(f"{tag}{row} w_hat", got[0][o], t32[0][o], ref[0][o])
        _rule(f"{tag}{row} dw", got[1][o], t32[1][o], ref[1][o], dw_scale)
    return got


@pytest.mark.parametrize("shape, layout", CASES, ids=lambda c: str(c).replace(" ", ""))
def test_forward_and_backward_against_float64(shape, layout):
    if shape == "cap+4":
        shape = (2, native().ws_cap // 4 + 1, 2, 2)
    g = torch.Generator().manual_seed(0)
    w = 0.02 + 0.05 * torch.randn(shape, generator=g)
    _check(f"{shape} {layout}", w, torch.randn(shape, generator=g), layout)


def _hard():
    g = torch.Generator().manual_seed(4)
    w = 0.05 * torch.randn(4, 16, 3, 3, generator=g)
    w[0] = 0.37
    w[1] = 1e3 + 1e-3 * torch.randn(16, 3, 3, generator=g)
    w[2] = 0
    w[2, 5, 1, 1] = 1e30
    return w, torch.randn(4, 16, 3, 3, generator=g)


def test_hard_rows():
    """A constant row (w_hat exactly 0, dw finite), 1e3 + 1e-3 randn, a single 1e30 among zeros:
    finite and within the rule, row by row."""
    w, g = _hard()
    w_hat, dw = _check("hard", w, g, CL, rows=True)
    assert not w_hat[0].any() and bool(torch.isfinite(dw).all())


def test_gradient_that_cancels():
    """g = 3 w_hat + 0.5: dw vanishes but for the eps term; the bound is absolute, on the size of
    the cancelling terms rstd * g."""
    w, g = _hard()
    w, g = w[3:], g[3:]
    h = W.compose(w.double())
    g = (3 * h + 0.5).float()
    rstd = torch.rsqrt(w.double().var(dim=(1, 2, 3), unbiased=False) + 1e-5).max().item()
    _check("cancel", w, g, CL, dw_scale=rstd * g.abs().max().item())


@pytest.mark.parametrize("layout", [CL, OFF], ids=["register", "scalar"])
def test_runs_repeat_and_a_row_does_not_see_its_tensor(layout):
    g = torch.Generator().manual_seed(2)
    w, dy = torch.randn(9, 32, 3, 3, generator=g), torch.randn(9, 32, 3, 3, generator=g)
    y, dw = _run(ops.weight_standardize, w, dy, layout)
    y2, dw2 = _run(ops.weight_standardize, w, dy, layout)
    assert torch.equal(y, y2) and torch.equal(dw, dw2)
    for o in range(9):
        y1, dw1 = _run(ops.weight_standardize, w[o:o + 1], dy[o:o + 1], layout)
        assert torch.equal(y[o:o + 1], y1) and torch.equal(dw[o:o + 1], dw1)


def test_cut_down_resnet50_gn_ws_matches_its_twin_on_the_device():
    """At the tolerances of test_groupnorm_gpu.py's cut-down model test (1e-5 on the output,
    1e-4 on gradients)."""
    m, t = W.cut_down_pair()
    m, t = m.cuda(), t.cuda()
    x = torch.randn(2, 3, 32, 32, device="cuda")
    y, yt = m(x), t(x)
    g = torch.randn_like(yt)
    y.backward(g)
    yt.backward(g)
    worst = max(((p.grad - q.grad).abs().max() / q.grad.abs().max().clamp_min(1e-30)).item()
                for p, q in zip(m.parameters(), t.parameters()))
    print(f"[model] |y - yt| max {(y - yt).abs().max().item():.3e} of {yt.abs().max().item():.3e}; "
          f"worst relative gradient difference {worst:.3e}")
    torch.testing.assert_close(y, yt, atol=1e-5, rtol=1e-5)
    for (n, p), q in zip(m.named_parameters(), t.parameters()):
        torch.testing.assert_close(p.grad, q.grad, atol=1e-4, rtol=1e-4, msg=lambda s: f"{n}: {s}")


def test_gradients_land_in_the_arena_under_ddp():
    from tutorial_torch_distributed_data_parallel_amd.parallel import runtime as rt
    from tutorial_torch_distributed_data_parallel_amd.parallel.arena import slot_view

    if tdp.parallel.is_initialized() and rt.get_backend() != "nccl":
        tdp.destroy_process_group()
    if not tdp.parallel.is_initialized():
        tdp.init_process_group("nccl", rank=0, world_size=1, local_rank=0)
    try:
        m = W.cut_down_pair()[0].cuda()
        before = m.layer1[0].conv2.weight.detach().clone()
        ddp = tdp.DDP(m)
        opt = tdp.optim.SGD(ddp.parameters(), lr=0.01)
        opt.zero_grad()
        x = torch.randn(2, 3, 32, 32, device="cuda")
        tdp.ops.cross_entropy(ddp(x), torch.tensor([1, 3], device="cuda")).backward()
        for n, p in m.named_parameters():
            buf, off = p._tdp_gslot
            assert p.grad is not None and p.grad.stride() == p.stride(), n
            assert p.grad.data_ptr() == slot_view(buf, p, off).data_ptr(), n
            assert bool(p.grad.any()) and bool(torch.isfinite(p.grad).all()), n
        opt.step()
        assert not torch.equal(m.layer1[0].conv2.weight, before)
    finally:
        tdp.destroy_process_group()


def test_graph_capture_replays_bitwise():
    torch.manual_seed(0)
    m = tdp.nn.StdConv2d(8, 16, 3, padding=1, bias=False).cuda()
    xs = torch.zeros(2, 8, 6, 6, device="cuda").contiguous(memory_format=torch.channels_last)
    xs.requires_grad_()
    gs = torch.zeros(2, 16, 6, 6, device="cuda").contiguous(memory_format=torch.channels_last)

    def step():
        y = m(xs)
        return (y,) + torch.autograd.grad(y, (xs, m.weight), gs)

    def load():
        with torch.no_grad():
            xs.copy_(torch.randn_like(xs))
            gs.copy_(torch.randn_like(gs))
            m.weight.copy_(torch.randn_like(m.weight))  # in place: w_hat must follow it

    load()
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        step()  # warm-up on the capture stream
    torch.cuda.current_stream().wait_stream(side)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph, stream=side):
        outs = step()
    for _ in range(3):
        load()
        graph.replay()
        torch.cuda.synchronize()
        got = [o.clone() for o in outs]
        for p, q in zip(got, step()):
            assert torch.equal(p, q)


def test_errors():
    w = torch.randn(8, 4, 3, 3, device="cuda")
    with pytest.raises(TypeError, match="float32"):
        ops.weight_standardize(w.double())
    with pytest.raises(TypeError, match="float32"):
        ops.weight_standardize(w.bfloat16())
    with pytest.raises(ValueError, match="dense"):
        ops.weight_standardize(w[:, :2])
    with pytest.raises(ValueError, match="4-D"):
        ops.weight_standardize(w[0])
