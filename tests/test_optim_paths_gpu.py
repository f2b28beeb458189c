"""The host state machine around the optimizer kernels (optim/fused.py), on the GPU: which of
FLAT / MULTI a step takes, the device hyper block's life (created, synced, dropped), the flat
step counter against torch's per-parameter ``state[p]["step"]``, the momentum first-step flag,
and load_state_dict. The kernels' arithmetic has its own tests (test_optim_gpu.py,
test_layerwise_optim_gpu.py); the CPU path never enters this code.

The model is Linear(8, 12) + Linear(12, 4) through ``flatten_module``: four tensors, two of them
1-D, numels 96 / 12 / 48 / 4. Gradients are seeded and written into the arena's grad views.

Reference and rule. Every GPU step is compared with the SAME class's CPU path on a CPU twin fed
the same gradients, by the rule of tests/optim_oracle.py: ONE step from the kernel's own fp32
state. Before each step the twin's parameters and state TENSORS are overwritten with the GPU's
(an exact copy); its bookkeeping -- step counts, whether a momentum buffer exists -- is never
touched, so it runs uninterrupted and a GPU step that used a wrong count, re-initialised an
adopted buffer or missed a hyper-parameter is a whole update off. The bound is the oracle's own
(``sgd_step`` / ``adam_step`` / ``lamb_step`` / ``lars_step``) for that snapshot; no tolerance is
introduced here. The twin's result stands where the float64 value stood: each of the two lies
within the propagated first-order error e of float64, the bound is 2e. LAMB's and LARS's trust
ratio is an input of their bound; the twin's own is taken (a MULTI step with mixed step counts
keeps only its last launch's workspace on the GPU).

Hyper-parameters the CPU paths of SGD and Adam hold as Python doubles while the kernels hold
floats (optim_oracle.py, "Contract difference to torch") are chosen exactly representable in
fp32 here (powers of two, 0.875, 1 - 2^-10), or enter torch only as a scalar operand of an fp32
tensor operation, which rounds them to fp32 as the kernel does (momentum 0.9). Step counts and
flags are compared exactly. Every test prints max(error/bound); a value above 1 fails.

Tensor-parallel SGD (``TensorParallel._begin_fused_step``) has no in-process one-rank fixture in
test_tensor_parallel_gpu.py (its world-size-1 case is a spawned worker), so it has no case here.
"""
import copy

import pytest
import torch

import layerwise_oracle as LO
import optim_oracle as O
import tutorial_torch_distributed_data_parallel_amd as tdp
from tutorial_torch_distributed_data_parallel_amd.parallel.arena import flatten_module

pytestmark = pytest.mark.gpu

LR, B1, B2, EPS, WD = 2.0 ** -6, 0.875, 1.0 - 2.0 ** -10, 2.0 ** -10, 0.125

# name -> (class, constructor arguments, the oracle's hyper dict)
CASES = {
    "adam": ("Adam", dict(lr=LR, betas=(B1, B2), eps=EPS),
             O.adam_hyper(lr=LR, beta1=B1, beta2=B2, eps=EPS)),
    "adamw_amsgrad": ("AdamW", dict(lr=LR, betas=(B1, B2), eps=EPS, weight_decay=WD, amsgrad=True),
                      O.adam_hyper(lr=LR, beta1=B1, beta2=B2, eps=EPS, weight_decay=WD,
                                   amsgrad=True, decoupled=True)),
    "lamb": ("LAMB", dict(lr=LR, betas=(B1, B2), eps=EPS, weight_decay=WD),
             LO.lamb_hyper(lr=LR, beta1=B1, beta2=B2, eps=EPS, weight_decay=WD)),
    "sgd_nesterov": ("SGD", dict(lr=0.0625, momentum=0.9, nesterov=True),
                     O.sgd_hyper(lr=0.0625, momentum=0.9, nesterov=True)),
    "lars": ("LARS", dict(lr=0.5, momentum=0.9, weight_decay=2.0 ** -10, trust_coefficient=0.02),
             LO.lars_hyper(lr=0.5, momentum=0.9, weight_decay=2.0 ** -10,
                           trust_coefficient=0.02)),
}
STATE_OF = {"buf": "momentum_buffer", "m": "exp_avg", "v": "exp_avg_sq", "vmax": "max_exp_avg_sq"}


class Pair:
    """A GPU optimizer over the flat arena and its CPU twin."""

    def __init__(self, name):
        self.name = name
        self.cls, self.kw, self.h = CASES[name]
        self.kw, self.h = dict(self.kw), dict(self.h)
        torch.manual_seed(7)
        twin = torch.nn.Sequential(torch.nn.Linear(8, 12), torch.nn.Linear(12, 4))
        model = copy.deepcopy(twin).cuda()
        self.arena = flatten_module(model)
        self.ps, self.cs = list(model.parameters()), list(twin.parameters())
        self.opt, self.ref = self.make(self.ps), self.make(self.cs)
        self.t = [0] * len(self.ps)  # the step count each parameter should be at
        self.worst = 0.0

    def make(self, params):
        return getattr(tdp.optim, self.cls)(params, **self.kw)

    def set_lr(self, lr):
        self.h["lr"] = lr
        for o in (self.opt, self.ref):
            o.param_groups[0]["lr"] = lr

    def step(self, k, without=None):
        """Step ``k`` of the sequence (the seed of its gradients) on both; parameter ``without``
        gets no gradient. Compares what the step wrote and returns nothing."""
        gen = torch.Generator().manual_seed(100 + k)
        snap = []
        for i, (p, c) in enumerate(zip(self.ps, self.cs)):
            g = 0.1 * torch.randn(p.shape, generator=gen)
            with torch.no_grad():
                c.copy_(p)
            for key, val in self.opt.state[p].items():
                if key != "step":
                    self.ref.state[c][key].copy_(val)
            if i == without:
                p.grad = c.grad = None
            else:
                v = self.arena.grad_view(self.arena.index(p))
                v.copy_(g)
                p.grad, c.grad = v, g
                assert self.arena.is_arena_grad(self.arena.index(p))
            snap.append({"p": c.detach().clone(), "g": g,
                         **{s: self.ref.state[c][key].clone() for s, key in STATE_OF.items()
                            if key in self.ref.state[c]}})
        self.opt.step()
        self.ref.step()
        torch.cuda.synchronize()
        for i, (p, c, s) in enumerate(zip(self.ps, self.cs, snap)):
            if i == without:
                assert torch.equal(p.detach().cpu(), s["p"])
                continue
            self.t[i] += 1
            bound = self.bound(i, c, s)
            for key, b in bound.items():
                got = p if key == "p" else self.opt.state[p][STATE_OF[key]]
                want = c if key == "p" else self.ref.state[c][STATE_OF[key]]
                self.worst = max(self.worst, O.error_ratio(got, want.detach().double(), b))

    def bound(self, i, c, s):
        h, t = self.h, self.t[i]
        z = torch.zeros_like(s["p"])
        if self.cls == "SGD":
            return O.sgd_step(s["p"], s["g"], s.get("buf"), h, first_step=t == 1)[1]
        if self.cls in ("Adam", "AdamW"):
            bc1, bc2 = O.bias_corrections(h["beta1"], h["beta2"], t, fp32_betas=True)
            return O.adam_step(s["p"], s["g"], s.get("m", z), s.get("v", z), s.get("vmax", z), h,
                               O.f32(bc1), O.f32(bc2))[1]
        ws, order = self.ref.trust_ratios()
        ratio = float(ws[2, [id(q) for q in order].index(id(c))])
        skip = c.dim() <= 1
        if self.cls == "LAMB":
            bc1, bc2 = LO.bias_corrections(h["beta1"], h["beta2"], t)
            bound = LO.lamb_step(s["p"], s["g"], s.get("m", z), s.get("v", z), h, bc1, bc2, ratio,
                                 skip=skip)[1]
            return {k: bound[k] for k in ("p", "m", "v")}
        bound = LO.lars_step(s["p"], s["g"], s.get("buf"), h, ratio, first_step=t == 1,
                             skip=skip)[1]
        return {k: bound[k] for k in ("p", "buf")}

    def steps_of(self, opt=None):
        opt = opt or self.opt
        params = self.cs if opt is self.ref else self.ps
        return [int(opt.state[p]["step"]) for p in params]

    def saved_steps(self, opt=None):
        st = (opt or self.opt).state_dict()["state"]
        return [int(st[i]["step"]) for i in range(len(self.ps))]

    def done(self, what):
        print(f"{what} {self.name}: max(error/bound) = {self.worst:.3f}")
        assert self.worst <= 1.0


def _slot(opt, name):
    return float(opt.hyper_block(0).cpu()[tdp.optim.fused.hyper_slots()[name]])


@pytest.mark.parametrize("name", ["adam", "adamw_amsgrad", "lamb"])
def test_flat_multi_flat_step_bookkeeping(name):
    """Two flat steps, one without a gradient for parameter 2 (the group leaves the flat path:
    block dropped, counter written back), one more with every gradient (the counts differ now,
    so the group stays on MULTI)."""
    pr = Pair(name)
    opt, key = pr.opt, id(pr.arena)
    pr.step(1)
    pr.step(2)
    assert opt._flat_step == {key: 2} and opt.device_step(0) == 2
    assert pr.saved_steps() == [2, 2, 2, 2]
    pr.step(3, without=2)
    assert opt.device_step(0) is None, "the block outlived the flat path"
    assert not opt._flat_step
    assert pr.steps_of() == [3, 3, 2, 3] and pr.saved_steps() == [3, 3, 2, 3]
    pr.step(4)
    assert not opt._flat_step and opt.device_step(0) is None
    assert pr.steps_of() == [4, 4, 3, 4] and pr.saved_steps() == [4, 4, 3, 4]
    assert pr.steps_of(pr.ref) == [4, 4, 3, 4]
    pr.done("flat -> multi -> flat")


@pytest.mark.parametrize("name", ["sgd_nesterov", "lars"])
def test_momentum_first_step_flag(name):
    """The first flat step initialises the buffer with the direction, the second follows the
    recurrence (both: the twin's own bookkeeping), and a fresh optimizer that loaded the state
    adopts the buffers: its block is created with no first-step request."""
    pr = Pair(name)
    pr.step(1)
    assert _slot(pr.opt, "first") == 1.0 and _slot(pr.opt, "first_next") == 0.0
    pr.step(2)
    assert _slot(pr.opt, "first") == 0.0 and _slot(pr.opt, "first_next") == 0.0
    before = [pr.opt.state[p]["momentum_buffer"].clone() for p in pr.ps]
    fresh = pr.make(pr.ps)
    fresh.load_state_dict(pr.opt.state_dict())
    assert fresh.device_step(0) is None
    for p, b in zip(pr.ps, before):
        assert torch.equal(fresh.state[p]["momentum_buffer"], b)
    pr.opt = fresh
    pr.step(3)
    assert _slot(fresh, "first") == 0.0 and _slot(fresh, "first_next") == 0.0
    bufs = fresh._flat_bufs[id(pr.arena)]["momentum_buffer"]
    for i, p in enumerate(pr.arena.params):  # state[p] are views of the adopted flat buffer
        assert fresh.state[p]["momentum_buffer"].data_ptr() == \
            pr.arena.state_view(bufs, i).data_ptr()
    pr.done("momentum first-step flag")


@pytest.mark.parametrize("name", ["adam", "lamb"])
def test_load_state_dict_on_the_flat_path(name):
    """Three flat steps, load into a fresh optimizer over the same arena: its first step creates
    the block with step count 3 and advances it to 4."""
    pr = Pair(name)
    for k in (1, 2, 3):
        pr.step(k)
    assert pr.opt.device_step(0) == 3
    fresh = pr.make(pr.ps)
    fresh.load_state_dict(pr.opt.state_dict())
    assert fresh.device_step(0) is None and not fresh._flat_step
    assert pr.steps_of(fresh) == [3, 3, 3, 3]
    pr.opt = fresh
    pr.step(4)
    assert fresh.device_step(0) == 4 and fresh._flat_step == {id(pr.arena): 4}
    assert pr.saved_steps() == [4, 4, 4, 4] and pr.steps_of(pr.ref) == [4, 4, 4, 4]
    pr.done("load_state_dict, flat")


@pytest.mark.parametrize("name", ["sgd_nesterov", "adam", "lamb", "lars"])
def test_lr_change_reaches_the_block(name):
    """A learning rate changed between two flat steps is in the block (as fp32) after the
    second, and the second used it (the twin did)."""
    pr = Pair(name)
    pr.step(1)
    lr0 = pr.h["lr"]
    assert _slot(pr.opt, "lr") == O.f32(lr0)
    blk = pr.opt.hyper_block(0)
    pr.set_lr(0.75 * lr0)
    pr.step(2)
    assert pr.opt.hyper_block(0) is blk, "the block was re-created instead of synced"
    assert _slot(pr.opt, "lr") == O.f32(0.75 * lr0)
    pr.done("lr change")
