"""Weight standardisation without a GPU: the op's CPU composition against the formula in
float64, ``StdConv2d`` against ``F.conv2d`` on the composed weight, checkpoints both ways with
``Conv2d``, ``resnet50_gn_ws`` against ``resnet50_gn``, the registry, and a two-rank gloo DDP
step against the full-batch step."""
import pytest
import torch
import torch.nn as nn
import torch.nn.functional as F

import tutorial_torch_distributed_data_parallel_amd as tdp
from tutorial_torch_distributed_data_parallel_amd import ops
from tutorial_torch_distributed_data_parallel_amd.models.registry import build_model
from tutorial_torch_distributed_data_parallel_amd.models.resnet import resnet50_gn, resnet50_gn_ws
from tutorial_torch_distributed_data_parallel_amd.parallel.launcher import spawn

import weight_std_workers as W  # noqa: E402  (tests/ is on sys.path via conftest)

LAYOUTS = [((8, 4, 3, 3), torch.channels_last), ((8, 3, 7, 7), torch.contiguous_format)]


@pytest.mark.parametrize("shape, fmt", LAYOUTS)
def test_op_and_gradient_match_the_formula_in_float64(shape, fmt):
    g = torch.Generator().manual_seed(0)
    w = (0.3 + torch.randn(shape, generator=g, dtype=torch.float64)).contiguous(memory_format=fmt)
    dy = torch.randn(shape, generator=g, dtype=torch.float64)
    w.requires_grad_()
    y = ops.weight_standardize(w)
    assert y.stride() == w.stride()
    torch.testing.assert_close(y, W.compose(w), rtol=1e-12, atol=1e-12)
    # the issue's closed form of the gradient, written out
    h, K = y.detach(), w[0].numel()
    rstd = torch.rsqrt(w.detach().var(dim=(1, 2, 3), unbiased=False, keepdim=True) + 1e-5)
    want = rstd * (dy - dy.mean(dim=(1, 2, 3), keepdim=True)
                   - h * (dy * h).sum(dim=(1, 2, 3), keepdim=True) / K)
    torch.testing.assert_close(torch.autograd.grad(y, w, dy)[0], want, rtol=1e-9, atol=1e-9)
    assert torch.autograd.gradcheck(ops.weight_standardize, (w,))


@pytest.mark.parametrize("kw", [dict(stride=2, padding=1), dict(padding=1, groups=2, relu=True)])
def test_stdconv2d_is_conv2d_on_the_composed_weight(kw):
    torch.manual_seed(1)
    m = tdp.nn.StdConv2d(8, 12, 3, eps=1e-4, **kw).double()  # float64: the orders of summation
    assert m.weight.is_contiguous(memory_format=torch.channels_last) and "eps=0.0001" in repr(m)
    x = torch.randn(2, 8, 9, 9, dtype=torch.float64, requires_grad=True)
    y = m(x)
    ref = F.conv2d(x, W.compose(m.weight, 1e-4), m.bias, kw.get("stride", 1), 1, 1,
                   kw.get("groups", 1))
    ref = F.relu(ref) if kw.get("relu") else ref
    torch.testing.assert_close(y, ref, rtol=1e-10, atol=1e-10)
    got = torch.autograd.grad(y.square().sum(), (x, m.weight, m.bias))
    want = torch.autograd.grad(ref.square().sum(), (x, m.weight, m.bias))
    for a, b in zip(got, want):  # differ by no more than rounding
        torch.testing.assert_close(a, b, rtol=1e-9, atol=1e-9)


def test_state_dict_moves_between_conv2d_and_stdconv2d():
    a, b = tdp.nn.Conv2d(4, 8, 3), tdp.nn.StdConv2d(4, 8, 3)
    assert list(a.state_dict()) == list(b.state_dict()) == ["weight", "bias"]
    b.load_state_dict(a.state_dict())
    assert torch.equal(b.weight, a.weight)
    a2 = tdp.nn.Conv2d(4, 8, 3)
    a2.load_state_dict(b.state_dict())
    assert torch.equal(a2.weight, b.weight) and torch.equal(a2.bias, b.bias)


def test_resnet50_gn_ws_is_resnet50_gn_with_standardised_convolutions():
    torch.manual_seed(0)
    m = resnet50_gn_ws()
    torch.manual_seed(0)
    r = resnet50_gn()
    sd, rd = m.state_dict(), r.state_dict()
    assert list(sd) == list(rd) and len(list(m.parameters())) == 161
    assert all(sd[k].shape == rd[k].shape and sd[k].stride() == rd[k].stride() and
               torch.equal(sd[k], rd[k]) for k in sd)  # also the same initial values
    convs = [c for c in m.modules() if isinstance(c, nn.Conv2d)]
    assert len(convs) == 53 and all(type(c) is tdp.nn.StdConv2d and not c.bn_stats for c in convs)
    assert all(type(c) is tdp.nn.Conv2d for c in r.modules() if isinstance(c, nn.Conv2d))
    assert resnet50_gn_ws(groups=16).layer2[1].bn2.num_groups == 16
    assert not hasattr(m, "_conv_layer")


@pytest.mark.parametrize("name", ["resnet50_gn_ws", "resnet-50-gn-ws"])
def test_registry_builds_the_model(name):
    m = build_model(name, num_classes=7).eval()
    assert type(m.conv1) is tdp.nn.StdConv2d and type(m.layer1[0].downsample[0]) is tdp.nn.StdConv2d
    with torch.no_grad():
        y = m(torch.randn(2, 3, 32, 32))
    assert y.shape == (2, 7) and bool(torch.isfinite(y).all())


def test_ddp_step_on_two_gloo_ranks_equals_the_full_batch_step():
    spawn(W.split_batch_step, 2, grace=5.0)
