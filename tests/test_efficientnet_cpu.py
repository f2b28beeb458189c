"""EfficientNet-B0, SiLU in the BatchNorm op, squeeze-and-excitation and stochastic depth on the
CPU: parameter count, state_dict interchange with the plain torch.nn twin, forward / gradient
equality, the flags and their errors, the conversion to SyncBatchNorm, the registry and a
two-rank gloo step."""
import copy

import pytest
import torch
import torch.nn as nn
import torch.nn.functional as F

import tutorial_torch_distributed_data_parallel_amd as tdp
from tutorial_torch_distributed_data_parallel_amd import ops
from tutorial_torch_distributed_data_parallel_amd.models.efficientnet import (EfficientNet, MBConv,
                                                                               efficientnet_b0)
from tutorial_torch_distributed_data_parallel_amd.models.registry import build_model, input_shape
from tutorial_torch_distributed_data_parallel_amd.parallel.launcher import spawn

import efficientnet_workers as W  # noqa: E402  (tests/ is on sys.path via conftest)
from efficientnet_twin import (TwinEfficientNetB0, TwinSqueezeExcitation, check_grads_rule,
                               check_rule)


def _count(m):
    return sum(p.numel() for p in m.parameters())


def test_parameter_count():
    """5,288,548 is torchvision's efficientnet_b0 count; if the twin disagrees, the twin is
    wrong."""
    assert _count(TwinEfficientNetB0(1000)) == 5_288_548
    assert _count(efficientnet_b0(num_classes=1000)) == 5_288_548
    assert len(list(efficientnet_b0().parameters())) == 213


def test_state_dict_keys_and_shapes_are_the_twins():
    m, t = efficientnet_b0(), TwinEfficientNetB0()
    sd, td = m.state_dict(), t.state_dict()
    assert list(sd) == list(td)
    assert all(sd[k].shape == td[k].shape for k in sd)
    for k in ("features.0.0.weight", "features.0.1.running_var",
              "features.1.0.block.0.0.weight", "features.1.0.block.1.fc1.weight",
              "features.1.0.block.1.fc2.bias", "features.1.0.block.2.1.weight",
              "features.2.0.block.0.1.weight", "features.2.1.block.1.0.weight",
              "features.2.0.block.2.fc1.bias", "features.2.0.block.3.1.num_batches_tracked",
              "features.7.0.block.3.0.weight", "features.8.0.weight", "features.8.1.bias",
              "classifier.1.weight", "classifier.1.bias"):
        assert k in sd, k
    assert "features.1.0.block.3.0.weight" not in sd  # the expand = 1 block has three parts
    assert sd["features.2.0.block.2.fc1.weight"].shape == (4, 96, 1, 1)
    assert sd["features.3.0.block.2.fc1.weight"].shape == (6, 144, 1, 1)
    assert sd["features.3.0.block.1.0.weight"].shape == (144, 1, 5, 5)
    assert sd["features.8.0.weight"].shape == (1280, 320, 1, 1)
    t.load_state_dict(sd, strict=True)
    m.load_state_dict(td, strict=True)


def test_layer_flags():
    """Every convolution feeding a BatchNorm has bn_stats and no bias; every SE convolution has
    a bias; the activations are fused SiLUs; block b drops with probability 0.2 b / 16."""
    m = efficientnet_b0()
    se = [s for s in m.modules() if isinstance(s, tdp.nn.SqueezeExcitation)]
    assert len(se) == 16
    assert [s.fc1.out_channels for s in se] == [8, 4, 6, 6, 10, 10, 20, 20, 20, 28, 28, 28,
                                                48, 48, 48, 48]
    se_convs = {id(c) for s in se for c in (s.fc1, s.fc2)}
    convs = [c for c in m.modules() if isinstance(c, nn.Conv2d)]
    assert len(convs) == 81 and len(se_convs) == 32
    for c in convs:
        if id(c) in se_convs:
            assert c.bias is not None and not c.bn_stats and isinstance(c, tdp.nn.Conv2d)
        else:
            assert c.bias is None and c.bn_stats
    for seq in (s for s in m.modules() if isinstance(s, nn.Sequential) and len(s) == 2
                and isinstance(s[1], tdp.nn.BatchNorm2d)):
        assert isinstance(seq[0], tdp.nn.Conv2d) and seq[0].bn_stats
    bns = [b for b in m.modules() if isinstance(b, tdp.nn.BatchNorm2d)]
    assert len(bns) == 49 and sum(b.silu for b in bns) == 33
    assert all(b.eps == 1e-5 and b.momentum == 0.1 and not (b.relu or b.relu6) for b in bns)
    assert "silu=True" in repr(m.features[0][1])
    assert "silu" not in repr(m.features[2][0].block[3][1])
    blocks = [b for b in m.modules() if isinstance(b, MBConv)]
    assert [b.stochastic_depth.p for b in blocks] == [0.2 * i / 16 for i in range(16)]
    assert sum(b.use_res_connect for b in blocks) == 9
    assert m.classifier[0].p == 0.2 and efficientnet_b0(dropout=0.5).classifier[0].p == 0.5


def test_initialisation_is_torchvisions():
    torch.manual_seed(0)
    m = efficientnet_b0(num_classes=1000)
    w = m.features[8][0].weight  # fan_out = 1280: std = sqrt(2 / 1280)
    assert abs(w.std().item() / (2.0 / 1280) ** 0.5 - 1) < 0.02
    lin = m.classifier[1]
    r = 1.0 / 1000 ** 0.5
    assert lin.weight.abs().max().item() <= r and abs(lin.weight.std().item() / (r / 3 ** 0.5) - 1) < 0.02
    assert not lin.bias.any()
    se = m.features[5][0].block[2]
    assert not se.fc1.bias.any() and not se.fc2.bias.any()
    bn = m.features[5][1].block[3][1]
    assert bool((bn.weight == 1).all()) and not bn.bias.any()


def _pair(fused, dtype=torch.float32):
    torch.manual_seed(0)
    m = EfficientNet(stochastic_depth_prob=0.0, dropout=0.0)
    t = TwinEfficientNetB0(stochastic_depth_prob=0.0, dropout=0.0)
    t.load_state_dict(m.state_dict())
    for b in m.modules():
        if isinstance(b, MBConv):
            b._fused_join = fused
    return m.to(dtype), t.to(dtype)


@pytest.mark.parametrize("fused", [True, False])
def test_model_matches_its_twin(fused):
    """Forward and every gradient against the twin in train mode at assert_close's defaults, in
    float64 (rtol = atol = 1e-7), on an 8x3x64x64 batch. In fp32 the untrained 49-BatchNorm
    network is too ill-conditioned for the fp32 defaults (rtol 1.3e-6): model and twin, which
    differ only in summation order, are 8e-5 apart on the logits, as the MobileNetV2 test found
    for its network. The float64 run tests the topology at the strictest defaults; fp32 is held
    to the project's float64 rule in the next test."""
    m, t = _pair(fused, torch.float64)
    x = torch.randn(8, 3, 64, 64, dtype=torch.float64)
    xm, xt = x.clone().requires_grad_(), x.clone().requires_grad_()
    y, yt = m(xm), t(xt)
    torch.testing.assert_close(y, yt)
    y.square().sum().backward()
    yt.square().sum().backward()
    for (n, p), q in zip(m.named_parameters(), t.parameters()):
        torch.testing.assert_close(p.grad, q.grad, msg=lambda s: f"{n}: {s}")
    torch.testing.assert_close(xm.grad, xt.grad)
    for a, b in zip(m.buffers(), t.buffers()):
        torch.testing.assert_close(a, b)


@pytest.mark.parametrize("fused", [True, False])
def test_model_fp32_against_float64_twin(fused):
    """The same comparison in fp32: e_model <= 4 e_torch + 2 * 2^-24 * scale against the float64
    twin, e_torch the fp32 twin's own error (the rule and c of tests/test_hard_inputs_gpu.py)."""
    m, t = _pair(fused)
    t64 = copy.deepcopy(t).double()
    x = torch.randn(8, 3, 64, 64)
    xs = [x.clone().requires_grad_(), x.clone().requires_grad_(), x.double().requires_grad_()]
    ys = [m(xs[0]), t(xs[1]), t64(xs[2])]
    for y in ys:
        y.square().sum().backward()
    check_rule("y", ys[0], ys[1], ys[2], ys[2].abs().max().item())
    check_rule("dx", xs[0].grad, xs[1].grad, xs[2].grad, xs[2].grad.abs().max().item())
    check_grads_rule("", m, t, t64)


def test_stochastic_depth_branch_and_eval():
    """With a probability > 0 a training block runs x + stochastic_depth(block(x)); in eval it
    is the plain residual."""
    torch.manual_seed(0)
    blk = MBConv(24, 24, 1, 3, 6, sd_prob=0.5)
    x = torch.randn(6, 24, 8, 8)
    blk.eval()
    with torch.no_grad():
        ref = x + blk.block(x)
        torch.testing.assert_close(blk(x), ref)
        blk.train()
        torch.manual_seed(1)
        y = blk(x)
        torch.manual_seed(1)
        branch = blk.block(x)
    d = y - x
    kinds = set()
    for n in range(6):
        if not d[n].any():
            kinds.add(0)
        else:
            torch.testing.assert_close(d[n], branch[n] * 2.0)
            kinds.add(1)
    assert kinds == {0, 1}


@pytest.mark.parametrize("shape", [(37, 16), (4, 8, 5, 5), (3, 6, 7, 5)])
def test_batch_norm_silu_matches_torch_under_autograd(shape):
    g = torch.Generator().manual_seed(0)
    C = shape[1]
    x = torch.randn(shape, generator=g)
    w = torch.empty(C).uniform_(2, 4, generator=g)
    b = torch.empty(C).uniform_(1, 4, generator=g)
    dy = torch.randn(shape, generator=g)
    leaves = [t.clone().requires_grad_() for t in (x, w, b)]
    refs = [t.clone().requires_grad_() for t in (x, w, b)]
    rm, rv, rm2, rv2 = torch.zeros(C), torch.ones(C), torch.zeros(C), torch.ones(C)
    y = ops.batch_norm(leaves[0], rm, rv, leaves[1], leaves[2], training=True, silu=True)
    yr = F.silu(F.batch_norm(refs[0], rm2, rv2, refs[1], refs[2], training=True))
    torch.testing.assert_close(y, yr, rtol=1e-5, atol=1e-5)
    y.backward(dy)
    yr.backward(dy)
    for a, r in zip(leaves, refs):
        torch.testing.assert_close(a.grad, r.grad, rtol=1e-4, atol=1e-5)
    torch.testing.assert_close(rm, rm2, rtol=1e-5, atol=1e-6)
    torch.testing.assert_close(rv, rv2, rtol=1e-5, atol=1e-6)
    # eval, with and without a differentiated input
    for grad in (False, True):
        xa, xr = x.clone().requires_grad_(grad), x.clone().requires_grad_(grad)
        y = ops.batch_norm(xa, rm, rv, w, b, training=False, silu=True)
        yr = F.silu(F.batch_norm(xr, rm, rv, w, b, training=False))
        torch.testing.assert_close(y, yr, rtol=1e-5, atol=1e-5)
        if grad:
            y.backward(dy)
            yr.backward(dy)
            torch.testing.assert_close(xa.grad, xr.grad, rtol=1e-5, atol=1e-6)


def test_silu_flag_errors():
    x = torch.randn(4, 8)
    with pytest.raises(ValueError, match="mutually exclusive"):
        ops.batch_norm(x, None, None, training=True, relu=True, silu=True)
    with pytest.raises(ValueError, match="mutually exclusive"):
        ops.batch_norm(x, None, None, training=True, relu6=True, silu=True)
    with pytest.raises(ValueError, match="residual"):
        ops.batch_norm(x, None, None, training=True, silu=True, residual=x)
    with pytest.raises(ValueError, match="mutually exclusive"):
        tdp.nn.BatchNorm2d(8, relu6=True, silu=True)


def test_modules_and_conversion_carry_silu():
    for cls, shape in ((tdp.nn.BatchNorm1d, (6, 8)), (tdp.nn.BatchNorm2d, (3, 8, 4, 4)),
                       (tdp.nn.SyncBatchNorm, (3, 8, 4, 4))):
        torch.manual_seed(0)
        bn = cls(8, silu=True)
        assert "silu=True" in repr(bn) and "relu" not in repr(bn)
        nn.init.uniform_(bn.weight, 2, 4)
        x = torch.randn(shape)
        ref = F.batch_norm(x, None, None, bn.weight, bn.bias, training=True)
        torch.testing.assert_close(bn(x), F.silu(ref), rtol=1e-5, atol=1e-5)
        torch.testing.assert_close(bn(x, relu=False), ref, rtol=1e-5, atol=1e-5)
    assert "silu" not in repr(tdp.nn.BatchNorm2d(8))
    seq = nn.Sequential(tdp.nn.BatchNorm2d(8, silu=True), tdp.nn.BatchNorm2d(8, relu6=True),
                        nn.BatchNorm2d(8))
    conv = tdp.nn.convert_sync_batchnorm(seq)
    assert all(isinstance(m, tdp.nn.SyncBatchNorm) for m in conv)
    assert [(m.relu6, m.silu) for m in conv] == [(False, True), (True, False), (False, False)]
    net = tdp.nn.convert_sync_batchnorm(efficientnet_b0())
    assert sum(getattr(b, "silu", False) for b in net.modules()) == 33


def test_standalone_ops_on_cpu():
    assert {"silu", "se_scale", "stochastic_depth"} <= set(ops.__all__)
    assert {"SiLU", "SqueezeExcitation", "StochasticDepth"} <= set(tdp.nn.__all__)
    assert isinstance(tdp.nn.SiLU(), nn.SiLU)
    x = torch.tensor([-1e4, -90.0, -1.0, -0.0, 0.0, 2.0, 1e4], requires_grad=True)
    y = tdp.nn.SiLU()(x)
    assert torch.equal(y, F.silu(x.detach()))
    # se_scale, both shapes of t, against the expression
    g = torch.Generator().manual_seed(0)
    a = torch.randn(2, 6, 3, 3, generator=g).requires_grad_()  # any C on the CPU
    t = (torch.randn(2, 6, generator=g) * 3).requires_grad_()
    y = ops.se_scale(a, t)
    torch.testing.assert_close(y, a * torch.sigmoid(t)[:, :, None, None])
    torch.testing.assert_close(ops.se_scale(a, t.reshape(2, 6, 1, 1)), y)
    y.sum().backward()
    s = torch.sigmoid(t.detach())
    torch.testing.assert_close(t.grad, s * (1 - s) * a.detach().sum((2, 3)))
    with pytest.raises(ValueError):
        ops.se_scale(a, torch.randn(2, 5))
    # the module against its twin
    se, tw = tdp.nn.SqueezeExcitation(24, 6), TwinSqueezeExcitation(24, 6)
    tw.load_state_dict(se.state_dict())
    h = torch.randn(3, 24, 5, 5, generator=g)
    torch.testing.assert_close(se(h), tw(h))
    # stochastic depth
    z = torch.randn(5, 8, 3, 3)
    assert ops.stochastic_depth(z, 0.0, True) is z and ops.stochastic_depth(z, 0.4, False) is z
    assert not ops.stochastic_depth(z, 1.0, True).any()
    out = ops.stochastic_depth(z, 0.4, True, generator=torch.Generator().manual_seed(0))
    inv = torch.ones(()).div_(0.6)
    assert all((not out[n].any()) or torch.equal(out[n], z[n] * inv) for n in range(5))
    with pytest.raises(NotImplementedError):
        ops.stochastic_depth(z, 0.4, True, mode="batch")
    with pytest.raises(NotImplementedError):
        tdp.nn.StochasticDepth(0.4, mode="batch")


def test_registry_and_settings(tmp_path):
    from tutorial_torch_distributed_data_parallel_amd.utils import config

    for name in ("efficientnet_b0", "efficientnetb0", "EfficientNet_B0"):
        m = build_model(name)
        assert isinstance(m, EfficientNet) and m.classifier[1].out_features == 10
    assert input_shape("efficientnet_b0") == (3, 224, 224)
    from tutorial_torch_distributed_data_parallel_amd import models
    assert models.efficientnet_b0 is efficientnet_b0
    path = tmp_path / "settings.yaml"
    path.write_text("train:\n  model: efficientnet_b0\n")
    cfg = config.load_settings(str(path))
    assert cfg["train"]["model"] == "efficientnet_b0"
    m = build_model(cfg["train"]["model"], num_classes=7).eval()
    with torch.no_grad():
        y = m(torch.randn(2, 3, 32, 32))
    assert y.shape == (2, 7) and bool(torch.isfinite(y).all())


def test_efficientnet_gloo_ddp_step_matches_torch_ddp(tmp_path):
    spawn(W.efficientnet_ddp_step_matches_torch_ddp, 2, args=(str(tmp_path),), grace=5.0)
