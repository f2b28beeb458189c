"""Stochastic depth on the GPU, and the EfficientNet pieces that have no gfx950 kernel yet.

The per-sample scale kernel (csrc/excite.hip) is tested bitwise. SiLU (stand-alone and as
BatchNorm's activation kind 3) and the squeeze-excitation gate run on CPU tensors only: the
kernels written for them were withheld (profiles/r19/efficientnet_b0.md), so on a GPU tensor they
raise instead of falling back to ATen -- pinned here, as tests/test_layernorm_gelu_gpu.py does
for LayerNorm and GELU."""
import pytest
import torch

import tutorial_torch_distributed_data_parallel_amd as tdp
from tutorial_torch_distributed_data_parallel_amd import ops

pytestmark = pytest.mark.gpu
CL = torch.channels_last
U = 2.0 ** -24


def test_stochastic_depth():
    x = torch.randn(5, 8, 3, 3, device="cuda")
    dy = torch.randn(5, 8, 3, 3, device="cuda")
    # torchvision's arithmetic: the kept samples are multiplied by the fp32 scale 1 / 0.6 (the
    # Bernoulli draw divided by the survival rate), which is what `x / 0.6` means here
    inv = torch.ones((), device="cuda").div_(0.6)
    torch.testing.assert_close(x * inv, x / 0.6, rtol=2 * U, atol=0)
    kept_total = 0
    for seed in range(8):
        g = torch.Generator(device="cuda").manual_seed(seed)
        g2 = torch.Generator(device="cuda").manual_seed(seed)
        keep = torch.empty(5, device="cuda").bernoulli_(0.6, generator=g2).bool()
        for fmt in (torch.contiguous_format, CL):
            g.manual_seed(seed)
            xx = x.detach().contiguous(memory_format=fmt).clone().requires_grad_()
            y = ops.stochastic_depth(xx, 0.4, True, generator=g)
            y.backward(dy)
            for n in range(5):  # every sample: exactly 0, or exactly x / 0.6
                if keep[n]:
                    assert torch.equal(y[n], x[n] * inv) and torch.equal(xx.grad[n], dy[n] * inv)
                else:
                    assert not y[n].any() and not xx.grad[n].any()
        kept_total += int(keep.sum())
    assert 0 < kept_total < 40  # both outcomes occurred
    assert ops.stochastic_depth(x, 0.0, True) is x
    assert ops.stochastic_depth(x, 0.4, False) is x
    sd = tdp.nn.StochasticDepth(0.4).eval()
    assert sd(x) is x
    z = ops.stochastic_depth(x, 1.0, True)
    assert z.shape == x.shape and not z.any()
    with pytest.raises(NotImplementedError):
        ops.stochastic_depth(x, 0.4, True, mode="batch")
    with pytest.raises(NotImplementedError):
        tdp.nn.StochasticDepth(0.4, mode="batch")
    with pytest.raises(TypeError):
        ops.stochastic_depth(x.double(), 0.4, True)
    empty = ops.stochastic_depth(x[:0], 0.4, True)  # an empty batch, as on the CPU
    assert empty.shape == (0, 8, 3, 3)


def test_stochastic_depth_tails_and_sizes():
    """An odd per-sample size and an unaligned view take the element-by-element form; a tensor
    of more than one block and a ragged last group of 4 take the vector body and its tail."""
    for shape, p in (((3, 5), 0.5), ((2, 3, 5, 7), 0.5), ((4, 16, 9, 9), 0.25), ((7, 4099), 0.5)):
        x = torch.randn(shape, device="cuda")
        g = torch.Generator(device="cuda").manual_seed(1)
        g2 = torch.Generator(device="cuda").manual_seed(1)
        scale = torch.empty(shape[0], device="cuda").bernoulli_(1 - p, generator=g2).div_(1 - p)
        y = ops.stochastic_depth(x, p, True, generator=g)
        assert torch.equal(y, x * scale.view((-1,) + (1,) * (x.dim() - 1)))
    base = torch.randn(4 * 8 + 1, device="cuda")
    xu = base[1:].view(4, 8)  # starts 4 bytes into its storage
    assert xu.data_ptr() % 16 == 4
    g = torch.Generator(device="cuda").manual_seed(2)
    g2 = torch.Generator(device="cuda").manual_seed(2)
    scale = torch.empty(4, device="cuda").bernoulli_(0.5, generator=g2).div_(0.5)
    assert torch.equal(ops.stochastic_depth(xu, 0.5, True, generator=g), xu * scale[:, None])


def test_kernels_withheld_raise_on_gpu_tensors():
    x = torch.randn(2, 8, 5, 5, device="cuda").contiguous(memory_format=CL)
    with pytest.raises(NotImplementedError, match="silu"):
        ops.silu(x)
    with pytest.raises(NotImplementedError, match="silu"):
        tdp.nn.SiLU()(x)
    with pytest.raises(NotImplementedError, match="silu"):
        ops.batch_norm(x, None, None, training=True, silu=True)
    with pytest.raises(NotImplementedError, match="silu"):
        ops.batch_norm(x, torch.zeros(8, device="cuda"), torch.ones(8, device="cuda"),
                       training=False, silu=True)
    with pytest.raises(NotImplementedError, match="se_scale"):
        ops.se_scale(x, torch.randn(2, 8, device="cuda"))
    # the flag errors come first, as on the CPU
    with pytest.raises(ValueError):
        ops.batch_norm(x, None, None, training=True, relu=True, silu=True)
    with pytest.raises(ValueError):
        ops.batch_norm(x, None, None, training=True, silu=True, residual=x)
    bn = tdp.nn.BatchNorm2d(8, silu=True, device="cuda")
    with pytest.raises(NotImplementedError, match="silu"):
        bn(x)
    # the other activation kinds are untouched
    y = ops.batch_norm(x, None, None, training=True, relu6=True)
    assert y.shape == x.shape and y.min().item() == 0.0
