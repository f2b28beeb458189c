"""LayerNorm, GELU and the MLP-Mixer without a GPU: the modules against torch's, the model's
parameter counts and registry entries, and a two-rank gloo DDP run of the small Mixer."""
import pytest
import torch
import torch.nn as nn

import tutorial_torch_distributed_data_parallel_amd as tdp
from tutorial_torch_distributed_data_parallel_amd.models.mixer import (MlpMixer, mixer_b16,
                                                                      mixer_s16)
from tutorial_torch_distributed_data_parallel_amd.models.registry import build_model, input_shape
from tutorial_torch_distributed_data_parallel_amd.parallel.launcher import spawn

import mixer_workers as W  # noqa: E402  (tests/ is on sys.path via conftest)
from mixer_twin import B16, S16, SMALL, TwinMixer


def _count(m):
    return sum(p.numel() for p in m.parameters())


@pytest.mark.parametrize("kw", [dict(), dict(elementwise_affine=False), dict(bias=False),
                                dict(eps=1e-3)], ids=["affine", "plain", "nobias", "eps"])
@pytest.mark.parametrize("shape,ns", [((5, 12), 12), ((2, 3, 4, 6), (4, 6))])
def test_layernorm_module_matches_torch(kw, shape, ns):
    torch.manual_seed(0)
    ours, ref = tdp.nn.LayerNorm(ns, **kw), nn.LayerNorm(ns, **kw)
    assert repr(ours) == repr(ref)
    assert list(ours.state_dict()) == list(ref.state_dict())
    with torch.no_grad():
        for p in ref.parameters():
            p.copy_(torch.randn_like(p))
    ours.load_state_dict(ref.state_dict())  # torch's -> ours
    back = nn.LayerNorm(ns, **kw)
    back.load_state_dict(ours.state_dict())  # ours -> torch's
    for p, q in zip(back.parameters(), ref.parameters()):
        assert torch.equal(p, q)
    x = torch.randn(shape, requires_grad=True)
    xr = x.detach().clone().requires_grad_()
    dy = torch.randn(shape)
    y, yr = ours(x), ref(xr)
    y.backward(dy)
    yr.backward(dy)
    assert torch.equal(y, yr) and torch.equal(x.grad, xr.grad)
    for p, q in zip(ours.parameters(), ref.parameters()):
        assert torch.equal(p.grad, q.grad)


def test_layernorm_rejects_a_wrong_trailing_shape():
    with pytest.raises(ValueError, match="normalized_shape"):
        tdp.ops.layer_norm(torch.randn(3, 5), 4)


@pytest.mark.parametrize("approximate", ["none", "tanh"])
def test_gelu_module_matches_torch(approximate):
    ours, ref = tdp.nn.GELU(approximate), nn.GELU(approximate)
    assert repr(ours) == repr(ref) and not ours.state_dict()
    x = (torch.randn(7, 9) * 3).requires_grad_()
    xr = x.detach().clone().requires_grad_()
    dy = torch.randn(7, 9)
    y, yr = ours(x), ref(xr)
    y.backward(dy)
    yr.backward(dy)
    assert torch.equal(y, yr) and torch.equal(x.grad, xr.grad)
    with pytest.raises(ValueError, match="approximate"):
        tdp.ops.gelu(x, approximate="erf")


def test_layernorm_applied_twice_sums_its_gradients():
    torch.manual_seed(1)
    ln, ref = tdp.nn.LayerNorm(8), nn.LayerNorm(8).double()
    with torch.no_grad():
        ln.weight.copy_(torch.randn(8))
        ln.bias.copy_(torch.randn(8))
    ref.load_state_dict(ln.state_dict())
    x = torch.randn(4, 8)
    ln(ln(x) * 2).square().sum().backward()
    ref(ref(x.double()) * 2).square().sum().backward()
    torch.testing.assert_close(ln.weight.grad.double(), ref.weight.grad, rtol=1e-4, atol=1e-4)
    torch.testing.assert_close(ln.bias.grad.double(), ref.bias.grad, rtol=1e-4, atol=1e-4)


def test_parameter_counts():
    """59,880,472 is the published Mixer-B/16 count (1000 classes); the others come from the
    plain torch twin of the published architecture. Exact conditions."""
    assert _count(mixer_b16(num_classes=1000)) == 59_880_472
    assert _count(mixer_b16(num_classes=10)) == 59_119_162
    assert _count(mixer_s16(num_classes=1000)) == 18_528_264
    assert _count(TwinMixer(**B16, num_classes=1000)) == 59_880_472
    assert _count(TwinMixer(**S16, num_classes=1000)) == 18_528_264
    assert _count(mixer_s16(num_classes=10)) == _count(TwinMixer(**S16, num_classes=10))
    assert _count(mixer_b16(num_classes=10)) == _count(TwinMixer(**B16, num_classes=10))


def test_small_mixer_matches_its_twin_and_loads_both_ways():
    torch.manual_seed(0)
    m, t = MlpMixer(**SMALL), TwinMixer(**SMALL)
    assert list(m.state_dict()) == list(t.state_dict())
    t.load_state_dict(m.state_dict())
    m.load_state_dict(t.state_dict())
    x = torch.randn(4, 3, 32, 32)
    y, yt = m(x), t(x)
    torch.testing.assert_close(y, yt, rtol=1e-5, atol=1e-6)
    y.square().sum().backward()
    yt.square().sum().backward()
    for (n, p), q in zip(m.named_parameters(), t.parameters()):
        torch.testing.assert_close(p.grad, q.grad, rtol=1e-4, atol=1e-6, msg=lambda s: f"{n}: {s}")
    with pytest.raises(ValueError, match="multiple of patch"):
        MlpMixer(image_size=30, patch=8, dim=8, depth=1, tokens_mlp=4, channels_mlp=8)


def test_registry_and_settings(tmp_path):
    from tutorial_torch_distributed_data_parallel_amd.utils import config

    for name, kw in (("mixer_s16", S16), ("mixer_b16", B16)):
        m = build_model(name)
        assert isinstance(m, MlpMixer) and len(m.blocks) == kw["depth"]
        assert m.head.out_features == 10 and m.stem.out_channels == kw["dim"]
        assert input_shape(name) == (3, 224, 224)
    with pytest.raises(ValueError, match="unknown model"):
        build_model("mixer_xl")
    path = tmp_path / "settings.yaml"
    path.write_text("train:\n  model: mixer_s16\n")
    cfg = config.load_settings(str(path))
    assert cfg["train"]["model"] == "mixer_s16"
    assert cfg["train"]["train_batch_size"] == config.TRAIN_DEFAULTS["train_batch_size"]
    assert isinstance(build_model(cfg["train"]["model"]), MlpMixer)


def test_mixer_gloo_ddp_matches_torch_ddp(tmp_path):
    spawn(W.mixer_ddp_matches_torch, 2, args=(str(tmp_path),), grace=5.0)
