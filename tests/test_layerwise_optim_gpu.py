"""tdp.optim.LAMB / LARS on the GPU (csrc/optim_layerwise.hip) against the float64 oracle of
tests/layerwise_oracle.py: norms and trust ratios with the bound derived from the kernels'
summation shape, the element update given the read-back ratio, memory (arena gaps, the gradient
arena, sentinels around unaligned views), determinism, a captured step and DDP at world size 1.
Every oracle test prints max(error/bound); a value above 1 fails. Shapes are tiny on purpose:
what can go wrong depends on the chunk length C and the small-chunk threshold, not on size.

One point where the text of the request and the formula part: an all-zero GRADIENT gives LAMB the
direction u = wd * p, whose norm is not zero, so the formula's ratio is ||p|| / ||wd p||, not 1.
The case asserts exactly 1 for LARS and for LAMB with weight_decay = 0, and the formula's value
(through the oracle) for LAMB with weight decay.
"""
import pytest
import torch

import layerwise_oracle as O
import tutorial_torch_distributed_data_parallel_amd as tdp
from tutorial_torch_distributed_data_parallel_amd._native import native
from tutorial_torch_distributed_data_parallel_amd.parallel.arena import ParamArena

pytestmark = pytest.mark.gpu


def _consts():
    c = native().layerwise_consts()
    return int(c["chunk"]), int(c["small"])


def _shapes():
    """numel 1, 3, 63, 64, 65, C-1, C, C+1, 2C+5 (2-D, so not skipped), SMALL and SMALL+1 (the
    wave / workgroup threshold), an all-zero parameter (index 11), an all-zero gradient (12), a
    1-D tensor (13, skipped under skip_1d) and a channels_last 4-D weight (14)."""
    C, S = _consts()
    ns = [1, 3, 63, 64, 65, C - 1, C, C + 1, 2 * C + 5, S, S + 1]
    return [(1, n) for n in ns] + [(5, 7), (6, 5), (100,), (8, 4, 3, 3)]


ZERO_P, ZERO_G, ONE_D, CL = 11, 12, 13, 14


def _make(seed, wide=True):
    """fp32 CPU (p, g) per tensor; with ``wide`` each tensor is scaled by a power of two in
    2^-40 .. 2^40 (p and g independently)."""
    gen = torch.Generator().manual_seed(seed)
    out = []
    for i, s in enumerate(_shapes()):
        kp = int(torch.randint(-40, 41, (1,), generator=gen)) if wide else 0
        kg = int(torch.randint(-40, 41, (1,), generator=gen)) if wide else -3
        p = torch.randn(*s, generator=gen) * 2.0 ** kp
        g = torch.randn(*s, generator=gen) * 2.0 ** kg
        if i == ZERO_P:
            p.zero_()
        if i == ZERO_G:
            g.zero_()
        out.append((p, g))
    return out


def _flat(data):
    """The tensors in one arena, gradients as arena views. Returns (params, arena)."""
    ps = []
    for i, (p, _) in enumerate(data):
        t = p.cuda()
        if i == CL:
            t = t.contiguous(memory_format=torch.channels_last)
        ps.append(torch.nn.Parameter(t))
    arena = ParamArena(ps)
    for i, (_, g) in enumerate(data):
        v = arena.grad_view(i)
        v.copy_(g.cuda())
        ps[i].grad = v
        assert arena.is_arena_grad(i)
    return ps, arena


def _multi(data):
    """The same tensors as views alloc[1 : 1 + n] (4-byte aligned only) between sentinels."""
    ps, allocs = [], []
    for i, (p, g) in enumerate(data):
        if i == CL:  # storage order of the channels_last weight
            p, g = p.permute(0, 2, 3, 1).contiguous(), g.permute(0, 2, 3, 1).contiguous()
        n = p.numel()
        ap = torch.full((n + 2,), 7.5, device="cuda")
        ag = torch.full((n + 2,), -7.5, device="cuda")
        ap[1:1 + n].copy_(p.reshape(-1).cuda())
        ag[1:1 + n].copy_(g.reshape(-1).cuda())
        q = torch.nn.Parameter(ap[1:1 + n].view(p.shape))
        q.grad = ag[1:1 + n].view(p.shape)
        ps.append(q)
        allocs.append((ap, ag))
    return ps, allocs


def _lamb(ps, h, **kw):
    return tdp.optim.LAMB(ps, lr=h["lr"], betas=(h["beta1"], h["beta2"]), eps=h["eps"],
                          weight_decay=h["weight_decay"], maximize=h["maximize"],
                          grad_scale=h["grad_scale"], **kw)


def _slices(arena, buf):
    return [buf[o:o + n].detach().clone().cpu() for o, n in zip(arena.offsets, arena.numels)]


def _gap_mask(arena):
    m = torch.ones(arena.numel, dtype=torch.bool, device=arena.data.device)
    for o, n in zip(arena.offsets, arena.numels):
        m[o:o + n] = False
    return m


def _check_norms(kind, h, ws, i, p0, x, e_x, skip):
    """Norms and ratio of tensor i against float64 with the summation-shape bound."""
    C, S = _consts()
    D = O.kernel_depth(p0.numel(), C, S)
    np_, e_np = O.norm_e(p0, D)
    nx, e_nx = O.norm_e(x, D, e_x)
    if kind == "lamb":
        r, rb = O.lamb_ratio(np_, e_np, nx, e_nx, skip=skip)
    else:
        r, rb = O.lars_ratio(np_, e_np, nx, e_nx, h, skip=skip)
    return max(O.scalar_ratio(ws[0, i], np_, O.SLACK * e_np),
               O.scalar_ratio(ws[1, i], nx, O.SLACK * e_nx), O.scalar_ratio(ws[2, i], r, rb))


@pytest.mark.parametrize("wd", [0.1, 0.0])
def test_lamb_flat_norms_ratio_and_elements(wd):
    """Steps t = 1 and t = 2 over the flat arena: norms, ratio, p, m, v; gaps stay zero and the
    gradient arena is bitwise unchanged."""
    h = O.lamb_hyper(weight_decay=wd, grad_scale=0.5, maximize=True)
    data = _make(1)
    ps, arena = _flat(data)
    opt = _lamb(ps, h)
    gaps = _gap_mask(arena)
    worst = 0.0
    for t in (1, 2):
        if t == 2:
            arena.grad.mul_(0.75)  # another gradient, still inside the arena
        g_before = arena.grad.clone()
        p0, g0 = _slices(arena, arena.data), _slices(arena, arena.grad)
        if t == 1:
            m0 = v0 = [torch.zeros_like(x) for x in p0]
        else:
            bufs = opt._flat_bufs[id(arena)]
            m0, v0 = _slices(arena, bufs["exp_avg"]), _slices(arena, bufs["exp_avg_sq"])
        opt.step()
        torch.cuda.synchronize()
        assert torch.equal(arena.grad, g_before)
        bufs = opt._flat_bufs[id(arena)]
        for buf in (arena.data, bufs["exp_avg"], bufs["exp_avg_sq"]):
            assert not buf[gaps].any(), "an arena gap was written"
        ws = opt.trust_ratios()[0].cpu()
        blk = opt.hyper_block(0).cpu()
        S = tdp.optim.fused.hyper_slots()
        assert int(blk.view(torch.int32)[S["step"]]) == t
        bc1, bc2 = float(blk[S["bc1"]]), float(blk[S["bc2"]])
        p1, m1 = _slices(arena, arena.data), _slices(arena, bufs["exp_avg"])
        v1 = _slices(arena, bufs["exp_avg_sq"])
        for i in range(len(ps)):
            skip = i == ONE_D
            out, bound = O.lamb_step(p0[i], g0[i], m0[i], v0[i], h, bc1, bc2, float(ws[2, i]),
                                     skip=skip)
            worst = max(worst, O.error_ratio(p1[i], out["p"], bound["p"]),
                        O.error_ratio(m1[i], out["m"], bound["m"]),
                        O.error_ratio(v1[i], out["v"], bound["v"]),
                        _check_norms("lamb", h, ws, i, p0[i], out["u"], bound["u"], skip))
        assert ws[2, ONE_D] == 1.0
        if t == 1:  # the first step moves the parameter off zero
            assert ws[0, ZERO_P] == 0.0 and ws[2, ZERO_P] == 1.0
        if wd == 0.0 and t == 1:
            assert ws[2, ZERO_G] == 1.0  # u = 0: see the module docstring
        assert ws[2, CL] != 1.0
    print(f"LAMB flat wd={wd}: max(error/bound) = {worst:.3f}")
    assert worst <= 1.0


LARS_FLAGS = {
    "momentum": dict(weight_decay=0.1),
    "nesterov": dict(nesterov=True, weight_decay=0.1, trust_coefficient=0.02),
    "dampening_maximize": dict(dampening=0.25, weight_decay=0.1, maximize=True, grad_scale=0.5),
    "no_momentum": dict(momentum=0.0, weight_decay=0.1),
}


@pytest.mark.parametrize("name", sorted(LARS_FLAGS))
def test_lars_flat_norms_ratio_and_elements(name):
    """Two steps (the first initialises the buffer) over the flat arena."""
    h = O.lars_hyper(**LARS_FLAGS[name])
    data = _make(2)
    ps, arena = _flat(data)
    opt = tdp.optim.LARS(ps, **h)
    gaps = _gap_mask(arena)
    mom = h["momentum"] != 0
    worst = 0.0
    for t in (1, 2):
        if t == 2:
            arena.grad.mul_(-1.5)
        g_before = arena.grad.clone()
        p0, g0 = _slices(arena, arena.data), _slices(arena, arena.grad)
        b0 = _slices(arena, opt._flat_bufs[id(arena)]["momentum_buffer"]) \
            if (mom and t == 2) else [None] * len(ps)
        opt.step()
        torch.cuda.synchronize()
        assert torch.equal(arena.grad, g_before)
        assert not arena.data[gaps].any()
        if mom:
            assert not opt._flat_bufs[id(arena)]["momentum_buffer"][gaps].any()
        ws = opt.trust_ratios()[0].cpu()
        p1 = _slices(arena, arena.data)
        b1 = _slices(arena, opt._flat_bufs[id(arena)]["momentum_buffer"]) if mom else None
        for i in range(len(ps)):
            skip = i == ONE_D
            out, bound = O.lars_step(p0[i], g0[i], b0[i], h, float(ws[2, i]), first_step=t == 1,
                                     skip=skip)
            worst = max(worst, O.error_ratio(p1[i], out["p"], bound["p"]),
                        _check_norms("lars", h, ws, i, p0[i], out["gp"], bound["gp"], skip))
            if mom:
                worst = max(worst, O.error_ratio(b1[i], out["buf"], bound["buf"]))
        assert ws[2, ZERO_G] == 1.0 and ws[2, ONE_D] == 1.0 and ws[2, CL] != 1.0
        if t == 1:  # the first step moves the parameter off zero
            assert ws[0, ZERO_P] == 0.0 and ws[2, ZERO_P] == 1.0
    print(f"LARS flat {name}: max(error/bound) = {worst:.3f}")
    assert worst <= 1.0


def _make_opt(kind, ps):
    if kind == "lamb":
        return _lamb(ps, O.lamb_hyper())
    return tdp.optim.LARS(ps, **O.lars_hyper(weight_decay=0.1, nesterov=True))


@pytest.mark.parametrize("kind", ["lamb", "lars"])
def test_multi_path_on_unaligned_views_equals_flat(kind):
    """The multi path (scalar instantiation: views at alloc[1:]) leaves the sentinels intact and
    gives bitwise the flat path's ratios, norms and parameters; two flat runs from equal state
    are bitwise equal too."""
    data = _make(3)
    runs = []
    for _ in range(2):
        ps, arena = _flat(data)
        opt = _make_opt(kind, ps)
        for _ in range(2):
            opt.step()
        torch.cuda.synchronize()
        runs.append((opt.trust_ratios()[0].clone(), _slices(arena, arena.data)))
    assert torch.equal(runs[0][0], runs[1][0])
    assert all(torch.equal(a, b) for a, b in zip(runs[0][1], runs[1][1]))
    ps, allocs = _multi(data)
    opt = _make_opt(kind, ps)
    for _ in range(2):
        opt.step()
    torch.cuda.synchronize()
    assert all(getattr(p, "_tdp_arena", None) is None for p in ps)
    for ap, ag in allocs:
        assert ap[0] == 7.5 and ap[-1] == 7.5 and ag[0] == -7.5 and ag[-1] == -7.5
    for (_, g), (_, ag) in zip(data, allocs):
        if g.dim() != 4:
            assert torch.equal(ag[1:-1].cpu(), g.reshape(-1))  # gradients untouched
    assert torch.equal(opt.trust_ratios()[0], runs[0][0])
    for q, ref in zip(ps, runs[0][1]):
        assert torch.equal(q.detach().reshape(-1).cpu(), ref)


@pytest.fixture(scope="module")
def pg():
    if not tdp.parallel.is_initialized():
        tdp.init_process_group("nccl", rank=0, world_size=1, local_rank=0)
    yield tdp
    tdp.destroy_process_group()


def _mlp(seed):
    from tutorial_torch_distributed_data_parallel_amd.models import ToyMLP

    torch.manual_seed(seed)
    return ToyMLP(in_features=64, hidden=(32,), num_classes=10, device="cuda")


def _ddp_opt(kind, d):
    if kind == "lamb":
        return tdp.optim.LAMB(d.parameters(), lr=0.02, weight_decay=0.01)
    return tdp.optim.LARS(d.parameters(), lr=0.5, momentum=0.9, weight_decay=1e-3,
                          trust_coefficient=0.02)


@pytest.mark.parametrize("kind", ["lamb", "lars"])
def test_captured_step_equals_eager(pg, kind):
    """ToyMLP 64-32-10, batch 8: three replays of a CapturedStep are bitwise the three eager
    steps, with the LR changed between replays (to 0: the parameters must not move; then to
    another value) through sync_all_hyper."""
    from tutorial_torch_distributed_data_parallel_amd.train.graph import CapturedStep

    X = torch.randn(64, 64, device="cuda")
    Y = torch.randint(0, 10, (64,), device="cuda")
    idx = torch.zeros(8, dtype=torch.long, device="cuda")

    def build():
        m = _mlp(3)
        d = tdp.DDP(m, device_ids=[0])
        return m, d, _ddp_opt(kind, d)

    def make_step(d, opt):
        def step():
            x, y = X.index_select(0, idx), Y.index_select(0, idx)
            opt.zero_grad(set_to_none=True)
            loss = tdp.ops.cross_entropy(d(x), y)
            loss.backward()
            opt.step()
            return loss
        return step

    m1, d1, o1 = build()
    m2, d2, o2 = build()
    eager = make_step(d1, o1)
    gen = torch.Generator().manual_seed(0)
    orders = [torch.randperm(64, generator=gen)[:8].cuda() for _ in range(4)]
    idx.copy_(orders[0])
    for _ in range(3):
        eager()
    graph = CapturedStep(make_step(d2, o2), warmup=3)
    lr0 = o1.param_groups[0]["lr"]
    for k, lr in enumerate((lr0, 0.0, 0.5 * lr0)):
        idx.copy_(orders[k + 1])
        for o in (o1, o2):
            o.param_groups[0]["lr"] = lr
        before = [p.detach().clone() for p in m2.parameters()]
        le, lg = eager(), graph.replay()
        torch.cuda.synchronize()
        assert torch.equal(le, lg)
        for a, b, c in zip(m1.parameters(), m2.parameters(), before):
            assert torch.equal(a, b)
            assert torch.equal(b, c) == (lr == 0.0), f"lr={lr} not honoured by the replay"
    assert torch.equal(o1.trust_ratios()[0], o2.trust_ratios()[0])
    if kind == "lamb":
        assert o2.device_step() == 6 and o1.device_step() == 6
        assert int(next(iter(o2.state_dict()["state"].values()))["step"]) == 6
    del graph, d1, d2


@pytest.mark.parametrize("kind", ["lamb", "lars"])
def test_ddp_world1_three_steps_match_float64_twin(pg, kind):
    """DDP at world size 1, backward then opt.step(), three steps. The float64 twin carries its
    own state from the common start and is fed the fp32 gradients and the read-back ratios of
    the run; the bound is the oracle's, accumulated step by step (each step's propagation
    starts from the error the state already carries)."""
    m = _mlp(4)
    d = tdp.DDP(m, device_ids=[0])
    opt = _ddp_opt(kind, d)
    g0 = opt.param_groups[0]
    arena = d.arena
    if kind == "lamb":
        h = O.lamb_hyper(lr=g0["lr"], eps=g0["eps"], weight_decay=g0["weight_decay"])
    else:
        h = O.lars_hyper(**{k: g0[k] for k in ("lr", "momentum", "weight_decay",
                                               "trust_coefficient")})
    x = torch.randn(8, 64, device="cuda")
    y = torch.randint(0, 10, (8,), device="cuda")
    n = len(arena.params)
    st = [{"p": s.double()} for s in _slices(arena, arena.data)]
    err = [dict() for _ in range(n)]
    worst = 0.0
    for t in (1, 2, 3):
        opt.zero_grad(set_to_none=True)
        tdp.ops.cross_entropy(d(x), y).backward()
        grads = _slices(arena, arena.grad)
        opt.step()
        torch.cuda.synchronize()
        ws = opt.trust_ratios()[0].cpu()
        params = opt.trust_ratios()[1]
        assert [id(p) for p in params] == [id(p) for p in arena.params]
        bufs = opt._flat_bufs[id(arena)]
        p1 = _slices(arena, arena.data)
        if kind == "lamb":
            blk, S = opt.hyper_block(0).cpu(), tdp.optim.fused.hyper_slots()
            bc1, bc2 = float(blk[S["bc1"]]), float(blk[S["bc2"]])
        for i in range(n):
            skip = arena.params[i].dim() <= 1
            if kind == "lamb":
                z = torch.zeros_like(st[i]["p"])
                out, bound = O.lamb_step(st[i]["p"], grads[i], st[i].get("m", z),
                                         st[i].get("v", z), h, bc1, bc2, float(ws[2, i]),
                                         skip=skip, e_in=err[i])
                keys = (("m", "exp_avg"), ("v", "exp_avg_sq"))
            else:
                out, bound = O.lars_step(st[i]["p"], grads[i], st[i].get("buf"), h,
                                         float(ws[2, i]), first_step=t == 1, skip=skip,
                                         e_in=err[i])
                keys = (("buf", "momentum_buffer"),)
            worst = max(worst, O.error_ratio(p1[i], out["p"], bound["p"]))
            for k, name in keys:
                got = _slices(arena, bufs[name])[i]
                worst = max(worst, O.error_ratio(got, out[k], bound[k]))
            st[i] = {k: out[k] for k in ("p",) + tuple(k for k, _ in keys)}
            err[i] = {k: bound[k] / O.SLACK for k in st[i]}
    print(f"{kind} DDP world 1, 3 steps: max(error/accumulated bound) = {worst:.3f}")
    assert worst <= 1.0
    del d
