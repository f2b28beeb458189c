"""bf16 mixed precision without a GPU: the autocast flag, the CPU twin of the bf16 Linear, the
Accelerator keyword, two gloo ranks and the CLI key."""
import os
import subprocess
import sys
import threading

import pytest
import torch
import torch.nn.functional as F
import yaml

import tutorial_torch_distributed_data_parallel_amd as tdp
from tutorial_torch_distributed_data_parallel_amd.accelerate import Accelerator
from tutorial_torch_distributed_data_parallel_amd.models import ToyMLP
from tutorial_torch_distributed_data_parallel_amd.parallel.arena import flatten_module
from tutorial_torch_distributed_data_parallel_amd.parallel.launcher import spawn

import autocast_workers as W  # noqa: E402  (tests/ is on sys.path via conftest)
from autocast_workers import bf

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(autouse=True)
def _no_process_group_left_behind():
    """Accelerator(cpu=True) joins a one-process gloo group: later test modules start clean."""
    yield
    if tdp.parallel.is_initialized():
        tdp.destroy_process_group()


# ------------------------------------------------------------------------------- the flag
def test_flag_nesting_decorator_and_disable():
    assert not tdp.is_autocast_enabled()
    ctx = tdp.autocast()
    with ctx:
        assert tdp.is_autocast_enabled()
        with ctx:  # re-entrant
            assert tdp.is_autocast_enabled()
            with tdp.autocast(enabled=False):
                assert not tdp.is_autocast_enabled()
            assert tdp.is_autocast_enabled()
        assert tdp.is_autocast_enabled()
    assert not tdp.is_autocast_enabled()

    @tdp.autocast()
    def inside():
        return tdp.is_autocast_enabled()

    assert inside() and not tdp.is_autocast_enabled()
    assert tdp.ops.autocast is tdp.autocast


def test_flag_restored_after_exception_and_thread_local():
    with pytest.raises(KeyError):
        with tdp.autocast():
            raise KeyError("x")
    assert not tdp.is_autocast_enabled()
    seen = []
    with tdp.autocast():
        t = threading.Thread(target=lambda: seen.append(tdp.is_autocast_enabled()))
        t.start()
        t.join()
    assert seen == [False]


def test_other_dtypes_raise():
    with pytest.raises(ValueError):
        tdp.autocast(dtype=torch.float16)
    with pytest.raises(ValueError):
        tdp.autocast(dtype=torch.float32)


# ------------------------------------------------------------------------------- CPU twin
def test_cpu_linear_equals_rounded_operand_math_and_fills_arena_slots():
    torch.manual_seed(0)
    net = torch.nn.Sequential(tdp.nn.Linear(96, 72, relu=True), tdp.nn.Linear(72, 10))
    arena = flatten_module(net)
    x = torch.randn(24, 96, requires_grad=True)
    dy = torch.randn(24, 10)
    with tdp.autocast():
        y = net(x)
    y.backward(dy)  # the flag is off again: backward follows the forward
    W1, b1, W2, b2 = [p.detach() for p in net.parameters()]
    h = F.relu(F.linear(bf(x.detach()), bf(W1), b1))
    assert torch.equal(y, F.linear(bf(h), bf(W2), b2))
    g1 = (bf(dy) @ bf(W2)) * (h > 0)
    assert torch.equal(net[1].weight.grad, bf(dy).t() @ bf(h))
    assert torch.equal(net[1].bias.grad, dy.sum(0))  # from the unrounded g
    assert torch.equal(net[0].weight.grad, bf(g1).t() @ bf(x.detach()))
    assert torch.equal(net[0].bias.grad, g1.sum(0))
    assert torch.equal(x.grad, bf(g1) @ bf(W1))
    for i in range(len(arena.params)):
        assert arena.is_arena_grad(i)
    # autocast off: the fp32 path, bit for bit
    y32 = net(x.detach())
    assert torch.equal(y32, F.linear(F.relu(F.linear(x.detach(), W1, b1)), W2, b2))
    assert not torch.equal(y32, y)


def test_factored_weight_is_refused():
    lin = tdp.nn.Linear(8, 4)
    owner = type("Owner", (), {})()
    lin.weight._tdp_factor = lambda: owner
    with tdp.autocast(), pytest.raises(RuntimeError, match="factor_sync=False"):
        lin(torch.randn(2, 8))


# ------------------------------------------------------------------------------- Accelerator
def _mlp():
    torch.manual_seed(3)
    return ToyMLP(in_features=24, hidden=(16, 16), num_classes=5)


def test_accelerator_bf16(monkeypatch):
    monkeypatch.delenv("ACCELERATE_MIXED_PRECISION", raising=False)
    acc = Accelerator(cpu=True, mixed_precision="bf16")
    assert acc.mixed_precision == "bf16"
    assert acc.ddp_kwargs["factor_sync"] is False
    assert not tdp.is_autocast_enabled()
    with acc.autocast():
        assert tdp.is_autocast_enabled()
    model = acc.prepare(_mlp())
    x = torch.randn(8, 24)
    out = model(x)  # the prepared forward runs under autocast
    assert not tdp.is_autocast_enabled()
    ref = _mlp()
    with tdp.autocast():
        want = ref(x)
    assert torch.equal(out, want)
    assert not torch.equal(out, ref(x))
    for bad in ("fp16", "fp8"):
        with pytest.raises(ValueError, match="bf16"):
            Accelerator(cpu=True, mixed_precision=bad)
    # explicit ddp_kwargs win
    assert Accelerator(cpu=True, mixed_precision="bf16",
                       ddp_kwargs={"factor_sync": True}).ddp_kwargs["factor_sync"] is True


def test_accelerator_reads_the_environment(monkeypatch):
    monkeypatch.setenv("ACCELERATE_MIXED_PRECISION", "bf16")
    assert Accelerator(cpu=True).mixed_precision == "bf16"
    assert Accelerator(cpu=True, mixed_precision="no").mixed_precision == "no"
    monkeypatch.delenv("ACCELERATE_MIXED_PRECISION")
    assert Accelerator(cpu=True).mixed_precision == "no"


@pytest.mark.parametrize("kw", [{}, {"mixed_precision": "no"}])
def test_accelerator_without_mixed_precision_is_the_fp32_path(monkeypatch, kw):
    monkeypatch.delenv("ACCELERATE_MIXED_PRECISION", raising=False)
    acc = Accelerator(cpu=True, **kw)
    assert acc.mixed_precision == "no" and "factor_sync" not in acc.ddp_kwargs
    with acc.autocast():
        assert not tdp.is_autocast_enabled()
    model = acc.prepare(_mlp())
    assert "forward" not in vars(model)  # not wrapped
    x = torch.randn(8, 24)
    y = torch.randint(0, 5, (8,))
    ref = _mlp()
    flatten_module(ref)
    out = model(x)
    assert torch.equal(out, ref(x))
    tdp.ops.cross_entropy(out, y).backward()
    tdp.ops.cross_entropy(ref(x), y).backward()
    for a, b in zip(model.parameters(), ref.parameters()):
        assert torch.equal(a.grad, b.grad)


# ------------------------------------------------------------------------------- two ranks
def test_two_gloo_ranks_under_autocast(tmp_path):
    spawn(W.amp_ddp_step, 2, args=(str(tmp_path),), grace=5.0)


# ------------------------------------------------------------------------------- CLI
def _settings(tmp_path, **train):
    s = {"script_path": os.path.join(ROOT, "scripts", "train_ddp.py"),
         "out_dir": str(tmp_path / "out"),
         "optional_args": {"set_epoch": True, "print_rand": False},
         "local": {"device": "cuda", "condor": {"num_gpus": 1}},
         "train": dict(model="toy_mlp", n_train=16, n_test=10, train_batch_size=8,
                       test_batch_size=10, num_epochs=1, checkpoint_epoch=1, lr=1e-3,
                       max_steps_per_epoch=1, **train)}
    p = tmp_path / "local_settings.yaml"
    p.write_text(yaml.safe_dump(s))
    return p, s


def _run(script, p):
    env = dict(os.environ, CUDA_VISIBLE_DEVICES="", HIP_VISIBLE_DEVICES="")
    return subprocess.run([sys.executable, os.path.join(ROOT, "scripts", script),
                           "--settings_file", str(p)], capture_output=True, text=True, env=env,
                          timeout=300, cwd=ROOT)


def test_cli_train_ddp_bf16(tmp_path):
    p, s = _settings(tmp_path, mixed_precision="bf16")
    r = _run("train_ddp.py", p)
    assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-3000:]
    assert "Epoch 1/1, Train Loss:" in r.stdout
    sd = torch.load(os.path.join(s["out_dir"], "ckpt_0.pt"), map_location="cpu",
                    weights_only=True)
    assert all(v.dtype == torch.float32 for v in sd.values() if v.is_floating_point())


def test_cli_rejects_unknown_mixed_precision(tmp_path):
    from tutorial_torch_distributed_data_parallel_amd.utils.config import load_settings

    p, _ = _settings(tmp_path, mixed_precision="fp16")
    with pytest.raises(ValueError, match="no, bf16"):
        load_settings(str(p))
    r = _run("train_ddp.py", p)
    assert r.returncode != 0 and "no, bf16" in r.stderr
    p, _ = _settings(tmp_path)
    assert load_settings(str(p))["train"]["mixed_precision"] == "no"
    p.write_text(p.read_text() + "\n")
    (tmp_path / "bare.yaml").write_text("out_dir: x\ntrain:\n  mixed_precision: no\n")
    assert load_settings(str(tmp_path / "bare.yaml"))["train"]["mixed_precision"] == "no"
