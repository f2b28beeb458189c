"""tdp.autocast on CPU tensors: ops.conv2d runs the bf16 contract in torch math -- operands rounded
once per pass, the ReLU mask and the bias gradient from the unrounded output gradient."""
import pytest
import torch
import torch.nn.functional as F

import tutorial_torch_distributed_data_parallel_amd as tdp
from tutorial_torch_distributed_data_parallel_amd import ops
from tutorial_torch_distributed_data_parallel_amd.ops import conv as convmod


def _r(t):
    return t.bfloat16().float()


def _tensors(N=2, Cin=8, H=9, W=7, Cout=12, R=3, s=1, p=1, seed=0):
    g = torch.Generator().manual_seed(seed)
    P, Q = (H + 2 * p - R) // s + 1, (W + 2 * p - R) // s + 1
    return (torch.randn(N, Cin, H, W, generator=g), torch.randn(Cout, Cin, R, R, generator=g),
            torch.randn(Cout, generator=g), torch.randn(N, Cout, P, Q, generator=g))


@pytest.mark.parametrize("s,p", [(1, 1), (2, 0)])
def test_forward_is_conv_of_rounded_operands(s, p):
    x, w, b, _ = _tensors(s=s, p=p)
    with tdp.autocast():
        y = ops.conv2d(x, w, b, s, p)
        yr = ops.conv2d(x, w, b, s, p, relu=True)
    assert y.dtype == torch.float32
    assert torch.equal(y, F.conv2d(_r(x), _r(w), b, s, p))
    assert torch.equal(yr, F.relu(y))
    assert not torch.equal(y, ops.conv2d(x, w, b, s, p))
    assert torch.equal(ops.conv2d(x, w, b, s, p), F.conv2d(x, w, b, s, p))


@pytest.mark.parametrize("s,p", [(1, 1), (2, 1)])
def test_gradients_follow_the_contract(s, p):
    x, w, b, dy = _tensors(s=s, p=p)
    x.requires_grad_()
    w.requires_grad_()
    b.requires_grad_()
    with tdp.autocast():
        y = ops.conv2d(x, w, b, s, p, relu=True)
    y.backward(dy)  # outside the region: the op was chosen in forward
    g = dy * (y.detach() > 0)
    gr = _r(g)
    assert not torch.equal(g, gr)
    dx = torch.nn.grad.conv2d_input(x.shape, _r(w.detach()), gr, s, p)
    dw = torch.nn.grad.conv2d_weight(_r(x.detach()), w.shape, gr, s, p)
    assert torch.equal(x.grad, dx)
    assert torch.equal(w.grad, dw)
    assert torch.equal(b.grad, g.sum(dim=(0, 2, 3)))          # unrounded g
    assert not torch.equal(b.grad, gr.sum(dim=(0, 2, 3)))
    assert all(t.grad.dtype == torch.float32 for t in (x, w, b))


def test_nested_disable_and_switch_restore_fp32():
    x, w, b, _ = _tensors()
    ref = F.conv2d(x, w, b, 1, 1)
    with tdp.autocast():
        with tdp.autocast(enabled=False):
            assert torch.equal(ops.conv2d(x, w, b, 1, 1), ref)
        assert not torch.equal(ops.conv2d(x, w, b, 1, 1), ref)
        convmod.AUTOCAST_FP32_CONV = True
        try:
            assert torch.equal(ops.conv2d(x, w, b, 1, 1), ref)
        finally:
            convmod.AUTOCAST_FP32_CONV = False
    assert torch.equal(ops.conv2d(x, w, b, 1, 1), ref)


def test_odd_shapes():
    # on the CPU every float32 shape follows the contract (there is no NHWC eligibility), and a
    # float64 tensor is left alone
    x, w, b, _ = _tensors(Cin=5, Cout=7, H=9, W=11)
    with tdp.autocast():
        assert torch.equal(ops.conv2d(x, w, b, 1, 1), F.conv2d(_r(x), _r(w), b, 1, 1))
        yd = ops.conv2d(x.double(), w.double(), b.double(), (2, 1), (0, 1))
    assert yd.dtype == torch.float64
    assert torch.equal(yd, F.conv2d(x.double(), w.double(), b.double(), (2, 1), (0, 1)))


def test_module_under_autocast():
    torch.manual_seed(0)
    m = tdp.nn.Conv2d(4, 8, 3, padding=1, relu=True)
    x = torch.randn(2, 4, 6, 6)
    with tdp.autocast():
        y = m(x)
    assert torch.equal(y, F.relu(F.conv2d(_r(x), _r(m.weight.detach()), m.bias.detach(), 1, 1)))
