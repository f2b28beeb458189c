"""tdp.optim.LAMB / LARS without a GPU: the CPU path against the float64 oracle of
tests/layerwise_oracle.py, state_dict round trip, constructor validation, skip_1d, the CLI and
Accelerator plumbing, and a two-rank gloo DDP run against a single-process twin.

The CPU path is plain torch code: it rounds where the kernels fuse (``m + a*d`` is two roundings,
an fma one), always at a value whose magnitude the bound already carries, which the factor 2 of
the bound covers. Its norms come from ``torch.linalg.vector_norm``, whose summation order is
unspecified, so the ratio check passes the worst-case depth n. Every test prints max(error/bound).
"""
import copy

import pytest
import torch

import layerwise_oracle as O
import tutorial_torch_distributed_data_parallel_amd as tdp
from tutorial_torch_distributed_data_parallel_amd.parallel.launcher import spawn

SHAPES = [(7, 5), (33,), (3, 4, 2, 2), (1,)]


def _params(seed):
    gen = torch.Generator().manual_seed(seed)
    return [torch.nn.Parameter(torch.randn(*s, generator=gen)) for s in SHAPES]


def _grads(ps, seed):
    gen = torch.Generator().manual_seed(seed)
    for p in ps:
        p.grad = 0.1 * torch.randn(p.shape, generator=gen)


def _snap(opt, ps, keys):
    return [{"p": p.detach().clone(), "g": p.grad.clone(),
             **{k: opt.state[p][k].clone() for k in keys if k in opt.state[p]}} for p in ps]


@pytest.mark.parametrize("flags", [dict(), dict(maximize=True, grad_scale=0.25),
                                   dict(weight_decay=0.0), dict(skip_1d=False)])
def test_lamb_cpu_matches_oracle(flags):
    h = O.lamb_hyper(**{k: v for k, v in flags.items() if k != "skip_1d"})
    ps = _params(1)
    opt = tdp.optim.LAMB(ps, lr=h["lr"], betas=(h["beta1"], h["beta2"]), eps=h["eps"],
                         weight_decay=h["weight_decay"], maximize=h["maximize"],
                         grad_scale=h["grad_scale"], skip_1d=flags.get("skip_1d", True))
    worst = 0.0
    for t in (1, 2, 3):
        _grads(ps, 10 + t)
        if t == 1:
            snap = [{"p": p.detach().clone(), "g": p.grad.clone(), "exp_avg": torch.zeros_like(p),
                     "exp_avg_sq": torch.zeros_like(p)} for p in ps]
        else:
            snap = _snap(opt, ps, ("exp_avg", "exp_avg_sq"))
        opt.step()
        ws, order = opt.trust_ratios()
        assert [id(p) for p in order] == [id(p) for p in ps]
        bc1, bc2 = O.bias_corrections(h["beta1"], h["beta2"], t)
        for i, (p, s) in enumerate(zip(ps, snap)):
            skip = flags.get("skip_1d", True) and p.dim() <= 1
            out, bound = O.lamb_step(s["p"], s["g"], s["exp_avg"], s["exp_avg_sq"], h, bc1, bc2,
                                     float(ws[2, i]), skip=skip)
            st = opt.state[p]
            assert int(st["step"].item()) == t
            n = p.numel()
            np_, e_np = O.norm_e(s["p"], n)
            nu, e_nu = O.norm_e(out["u"], n, bound["u"])
            r, rb = O.lamb_ratio(np_, e_np, nu, e_nu, skip=skip)
            worst = max(worst, O.error_ratio(p, out["p"], bound["p"]),
                        O.error_ratio(st["exp_avg"], out["m"], bound["m"]),
                        O.error_ratio(st["exp_avg_sq"], out["v"], bound["v"]),
                        O.scalar_ratio(ws[2, i], r, rb),
                        O.scalar_ratio(ws[0, i], np_, O.SLACK * e_np),
                        O.scalar_ratio(ws[1, i], nu, O.SLACK * e_nu))
    print(f"LAMB cpu {flags}: max(error/bound) = {worst:.3f}")
    assert worst <= 1.0


@pytest.mark.parametrize("flags", [
    dict(), dict(momentum=0.0), dict(nesterov=True, weight_decay=0.1),
    dict(dampening=0.25, weight_decay=0.1), dict(maximize=True, grad_scale=0.25,
                                                 weight_decay=0.1),
    dict(skip_1d=False, weight_decay=0.1)])
def test_lars_cpu_matches_oracle(flags):
    h = O.lars_hyper(**{k: v for k, v in flags.items() if k != "skip_1d"})
    ps = _params(2)
    opt = tdp.optim.LARS(ps, skip_1d=flags.get("skip_1d", True), **h)
    worst = 0.0
    for t in (1, 2, 3):
        _grads(ps, 20 + t)
        snap = _snap(opt, ps, ("momentum_buffer",))
        opt.step()
        ws, _ = opt.trust_ratios()
        for i, (p, s) in enumerate(zip(ps, snap)):
            skip = flags.get("skip_1d", True) and p.dim() <= 1
            out, bound = O.lars_step(s["p"], s["g"], s.get("momentum_buffer"), h,
                                     float(ws[2, i]), first_step=t == 1, skip=skip)
            n = p.numel()
            np_, e_np = O.norm_e(s["p"], n)
            ng, e_ng = O.norm_e(out["gp"], n, bound["gp"])
            q, qb = O.lars_ratio(np_, e_np, ng, e_ng, h, skip=skip)
            worst = max(worst, O.error_ratio(p, out["p"], bound["p"]),
                        O.scalar_ratio(ws[2, i], q, qb))
            if h["momentum"]:
                worst = max(worst, O.error_ratio(opt.state[p]["momentum_buffer"], out["buf"],
                                                 bound["buf"]))
            else:
                assert "momentum_buffer" not in opt.state[p]
    print(f"LARS cpu {flags}: max(error/bound) = {worst:.3f}")
    assert worst <= 1.0


def test_zero_tensors_take_ratio_one():
    """An all-zero parameter or an all-zero gradient gives the ratio exactly 1. (LAMB's condition
    is on ||u||, and u = wd * p under a zero gradient: exactly 1 needs weight_decay = 0 there.)"""
    for make in (lambda ps: tdp.optim.LAMB(ps, lr=0.01, weight_decay=0.0),
                 lambda ps: tdp.optim.LARS(ps, lr=0.1, weight_decay=0.1)):
        ps = [torch.nn.Parameter(torch.zeros(4, 3)), torch.nn.Parameter(torch.ones(4, 3)),
              torch.nn.Parameter(torch.ones(2, 3))]
        ps[0].grad, ps[1].grad = torch.ones(4, 3), torch.zeros(4, 3)
        ps[2].grad = torch.ones(2, 3)
        opt = make(ps)
        opt.step()
        ws, _ = opt.trust_ratios()
        assert ws[2, 0] == 1.0 and ws[2, 1] == 1.0 and ws[2, 2] != 1.0


@pytest.mark.parametrize("name", ["lamb", "lars"])
def test_skip_1d(name):
    """ndim <= 1: ratio 1 and no weight decay -- the step of the same optimizer with
    weight_decay = 0 on that tensor and a ratio forced to 1 (plain Adam / SGD direction)."""
    def make(ps, **kw):
        if name == "lamb":
            return tdp.optim.LAMB(ps, lr=0.01, weight_decay=0.1, **kw)
        return tdp.optim.LARS(ps, lr=0.1, weight_decay=0.1, momentum=0.9, **kw)

    a, b = _params(3), _params(3)
    oa, ob = make(a), make(b, skip_1d=False)
    for t in range(2):
        _grads(a, 30 + t)
        _grads(b, 30 + t)
        oa.step()
        ob.step()
    wa, wb = oa.trust_ratios()[0], ob.trust_ratios()[0]
    for i, (p, q) in enumerate(zip(a, b)):
        if p.dim() <= 1:
            assert wa[2, i] == 1.0 and wb[2, i] != 1.0 and not torch.equal(p, q)
        else:
            assert wa[2, i] == wb[2, i] and torch.equal(p, q)
    # the skipped bias moved exactly like torch SGD with momentum / like Adam without decay
    if name == "lars":
        ref = torch.nn.Parameter(_params(3)[1].detach().clone())
        ropt = torch.optim.SGD([ref], lr=0.1, momentum=0.9)
        for t in range(2):
            tmp = _params(3)
            _grads(tmp, 30 + t)
            ref.grad = tmp[1].grad
            ropt.step()
        torch.testing.assert_close(a[1].detach(), ref.detach(), rtol=1e-6, atol=1e-7)


@pytest.mark.parametrize("name", ["lamb", "lars"])
def test_state_dict_round_trip(name):
    def make(ps):
        if name == "lamb":
            return tdp.optim.LAMB(ps, lr=0.01)
        return tdp.optim.LARS(ps, lr=0.1, momentum=0.9, weight_decay=1e-2)

    a = _params(4)
    oa = make(a)
    for t in range(2):
        _grads(a, 40 + t)
        oa.step()
    sd = copy.deepcopy(oa.state_dict())  # as a checkpoint: no tensor shared with oa
    keys = {"exp_avg", "exp_avg_sq", "step"} if name == "lamb" else {"momentum_buffer"}
    assert all(set(s) == keys for s in sd["state"].values())
    b = [torch.nn.Parameter(p.detach().clone()) for p in a]
    ob = make(b)
    ob.load_state_dict(sd)
    _grads(a, 50)
    _grads(b, 50)
    oa.step()
    ob.step()
    for p, q in zip(a, b):
        assert torch.equal(p, q)
    if name == "lamb":
        assert all(int(ob.state[q]["step"].item()) == 3 for q in b)
    assert ob.state_dict()["param_groups"][0]["skip_1d"] is True


def test_flat_arena_cpu_step_and_step_counter():
    """Over a CPU arena (flatten_module) the step is the CPU path on the arena views."""
    from tutorial_torch_distributed_data_parallel_amd.models import ToyMLP
    from tutorial_torch_distributed_data_parallel_amd.parallel.arena import flatten_module

    torch.manual_seed(0)
    m1 = ToyMLP(in_features=12, hidden=(8,), num_classes=3)
    m2 = ToyMLP(in_features=12, hidden=(8,), num_classes=3)
    m2.load_state_dict(m1.state_dict())
    flatten_module(m1)
    o1, o2 = tdp.optim.LAMB(m1.parameters(), lr=0.01), tdp.optim.LAMB(m2.parameters(), lr=0.01)
    x, y = torch.randn(6, 12), torch.randint(0, 3, (6,))
    for _ in range(2):
        for m, o in ((m1, o1), (m2, o2)):
            o.zero_grad()
            torch.nn.functional.cross_entropy(m(x), y).backward()
            o.step()
    for p, q in zip(m1.parameters(), m2.parameters()):
        assert torch.equal(p, q)


def test_constructor_validation():
    p = [torch.nn.Parameter(torch.zeros(2, 2))]
    for kw in (dict(lr=-1.0), dict(eps=-1.0), dict(weight_decay=-0.1), dict(betas=(1.0, 0.9)),
               dict(betas=(0.9, -0.1))):
        with pytest.raises(ValueError):
            tdp.optim.LAMB(p, **kw)
    for kw in (dict(lr=-1.0), dict(lr=0.1, momentum=-0.1), dict(lr=0.1, weight_decay=-1.0),
               dict(lr=0.1, eps=-1.0), dict(lr=0.1, trust_coefficient=0.0),
               dict(lr=0.1, nesterov=True, momentum=0.0),
               dict(lr=0.1, nesterov=True, dampening=0.5)):
        with pytest.raises(ValueError):
            tdp.optim.LARS(p, **kw)
    with pytest.raises(TypeError):
        tdp.optim.LARS(p)  # lr is required
    half = [torch.nn.Parameter(torch.zeros(2, 2, dtype=torch.float64))]
    with pytest.raises(TypeError):
        tdp.optim.LAMB(half)
    with pytest.raises(TypeError):
        tdp.optim.LARS(half, lr=0.1)
    # neither is an Adam or an SGD: DDP's in-reduction fusion accepts those by isinstance
    assert not isinstance(tdp.optim.LAMB(p), (tdp.optim.Adam, tdp.optim.SGD))
    assert not isinstance(tdp.optim.LARS(p, lr=0.1), (tdp.optim.Adam, tdp.optim.SGD))
    d = tdp.optim.LAMB(p).defaults
    assert (d["lr"], d["betas"], d["eps"], d["weight_decay"]) == (1e-3, (0.9, 0.999), 1e-6, 0.01)
    d = tdp.optim.LARS(p, lr=0.1).defaults
    assert (d["momentum"], d["dampening"], d["weight_decay"], d["nesterov"],
            d["trust_coefficient"], d["eps"]) == (0.9, 0.0, 0.0, False, 1e-3, 1e-8)


def test_cli_optimizer_names():
    from tutorial_torch_distributed_data_parallel_amd import cli

    p = [torch.nn.Parameter(torch.zeros(2, 2))]
    t = {"optimizer": "LAMB", "lr": 0.002, "momentum": 0.8}
    o = cli._optimizer(t, p)
    assert type(o) is tdp.optim.LAMB and o.defaults["lr"] == 0.002
    t["optimizer"] = "lars"
    o = cli._optimizer(t, p)
    assert type(o) is tdp.optim.LARS and o.defaults["lr"] == 0.002
    assert o.defaults["momentum"] == 0.8
    dev = torch.device("cuda")  # only its .type is read
    assert not cli._want_fused({"optimizer": "lars", "fused_optimizer": True}, dev)
    assert not cli._want_fused({"optimizer": "lamb"}, dev)
    assert cli._want_fused({"optimizer": "adam"}, dev)


def test_fuse_optimizer_is_false_on_a_cpu_process():
    from tutorial_torch_distributed_data_parallel_amd.accelerate import Accelerator
    from tutorial_torch_distributed_data_parallel_amd.models import ToyMLP

    try:
        acc = Accelerator(cpu=True)
        m = ToyMLP(in_features=6, hidden=(4,), num_classes=3)
        for o in (tdp.optim.LAMB(m.parameters()), tdp.optim.LARS(m.parameters(), lr=0.1)):
            assert acc.fuse_optimizer(m, o) is False
    finally:
        if tdp.parallel.is_initialized():
            tdp.destroy_process_group()


def test_two_rank_ddp_matches_single_process_twin(tmp_path):
    """Also: register_fused_optimizer raises TypeError for both, Accelerator.fuse_optimizer
    returns False for both on a real DDP (tests/layerwise_workers.py)."""
    import layerwise_workers as W

    spawn(W.ddp_matches_twin, 2, args=(str(tmp_path),), grace=5.0)
