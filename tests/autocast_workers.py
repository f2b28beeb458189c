"""Shared pieces of the autocast tests: the contract oracle in torch math, and the gloo worker
(run under parallel.launcher.spawn)."""
import torch
import torch.nn.functional as F


def bf(t, dt=torch.float32):
    """Round every element to bf16 (RNE), back in ``dt``."""
    return t.bfloat16().to(dt)


def mlp_contract(Ws, bs, x, y, dt=torch.float32, scales=None):
    """Loss and gradients of a Linear(+ReLU)... Linear MLP with mean cross-entropy under the
    mixed-precision contract: every GEMM operand rounded to bf16, products and sums in ``dt``,
    the bias gradient from the unrounded g, the loss in ``dt``. Returns (loss, dWs, dbs); a
    ``scales`` list receives per layer (|bf g|^T |bf a|, sum |g|), the magnitudes the rounding
    errors of dW and db are relative to."""
    acts = [x.to(dt)]
    n = len(Ws)
    for i, (W, b) in enumerate(zip(Ws, bs)):
        z = F.linear(bf(acts[-1], dt), bf(W, dt), b.to(dt))
        acts.append(F.relu(z) if i < n - 1 else z)
    logits = acts[-1].detach().requires_grad_(True)
    loss = F.cross_entropy(logits, y)
    g, = torch.autograd.grad(loss, logits)
    dWs, dbs = [None] * n, [None] * n
    for i in reversed(range(n)):
        a = acts[i]
        dWs[i] = bf(g, dt).t() @ bf(a, dt)
        dbs[i] = g.sum(0)
        if scales is not None:
            scales.insert(0, (bf(g, dt).abs().t() @ bf(a, dt).abs(), g.abs().sum(0)))
        if i > 0:
            g = (bf(g, dt) @ bf(Ws[i], dt)) * (a > 0)
    return loss.detach(), dWs, dbs


def amp_ddp_step(rank, out_dir):
    """Two gloo ranks: a DDP step under autocast (factor_sync=False) averages the ranks'
    rounded-operand gradients and keeps the replicas identical."""
    import torch.distributed as dist

    import tutorial_torch_distributed_data_parallel_amd as tdp
    from tutorial_torch_distributed_data_parallel_amd.models import ToyMLP
    from tutorial_torch_distributed_data_parallel_amd.parallel import runtime as rt

    tdp.init_process_group("gloo")
    r, ws = rt.get_rank(), rt.get_world_size()

    def gather(obj):
        out = [None] * ws
        dist.all_gather_object(out, obj)
        return out

    torch.manual_seed(100 + r)
    model = ToyMLP(in_features=24, hidden=(16, 16), num_classes=5)
    ddp = tdp.DDP(model, bucket_cap_mb=0.0005, factor_sync=False)
    g = torch.Generator().manual_seed(7 + r)
    x = torch.randn(8, 24, generator=g)
    y = torch.randint(0, 5, (8,), generator=g)
    fcs = [model.fc1, model.fc2, model.fc3]
    _, dWs, dbs = mlp_contract([m.weight.detach() for m in fcs], [m.bias.detach() for m in fcs],
                               x, y)
    with tdp.autocast():
        loss = tdp.ops.cross_entropy(ddp(x), y)
    loss.backward()  # outside the region: backward follows the forward's choice
    for i in range(len(ddp.arena.params)):
        assert ddp.arena.is_arena_grad(i)
    alls = gather((dWs, dbs))
    for i, m in enumerate(fcs):
        mw = sum(a[0][i] for a in alls) / ws
        mb = sum(a[1][i] for a in alls) / ws
        torch.testing.assert_close(m.weight.grad, mw, atol=1e-6, rtol=1e-5)
        torch.testing.assert_close(m.bias.grad, mb, atol=1e-6, rtol=1e-5)
    # and it is not the fp32 gradient
    ref = ToyMLP(in_features=24, hidden=(16, 16), num_classes=5)
    ref.load_state_dict(model.state_dict())
    F.cross_entropy(ref(x), y).backward()
    assert not torch.equal(ref.fc1.weight.grad, dWs[0])
    opt = tdp.optim.SGD(ddp.parameters(), lr=0.1, momentum=0.9)
    for _ in range(2):
        opt.zero_grad()
        with tdp.autocast():
            tdp.ops.cross_entropy(ddp(x), y).backward()
        opt.step()
    allp = gather([p.detach().clone() for p in model.parameters()])
    for other in allp:
        for a, b in zip(other, allp[0]):
            assert torch.equal(a, b)
    tdp.destroy_process_group()
