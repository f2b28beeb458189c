"""Two-rank gloo workers of tests/test_layerwise_optim_cpu.py (run under parallel.launcher.spawn)."""
import torch
import torch.distributed as dist

import tutorial_torch_distributed_data_parallel_amd as tdp
from tutorial_torch_distributed_data_parallel_amd.models import ToyMLP
from tutorial_torch_distributed_data_parallel_amd.parallel import runtime as rt

SHAPE = dict(in_features=24, hidden=(16, 16), num_classes=5)


def _make(name, params):
    if name == "lamb":
        return tdp.optim.LAMB(params, lr=0.02, weight_decay=0.01)
    return tdp.optim.LARS(params, lr=0.5, momentum=0.9, weight_decay=1e-3,
                          trust_coefficient=0.02)


def _batch(step, rank):
    g = torch.Generator().manual_seed(1000 + 10 * step + rank)
    return torch.randn(8, 24, generator=g), torch.randint(0, 5, (8,), generator=g)


def ddp_matches_twin(rank, out_dir):
    """Three steps of DDP (backward, then opt.step() on the averaged arena gradient) at two
    ranks == one process on the concatenated batch; replicas stay bitwise equal; the fused
    registration is refused (TypeError) and Accelerator.fuse_optimizer answers False."""
    from tutorial_torch_distributed_data_parallel_amd.accelerate import Accelerator

    acc = Accelerator(cpu=True)  # joins the gloo group
    r, ws = rt.get_rank(), rt.get_world_size()
    assert ws == 2
    for name in ("lamb", "lars"):
        torch.manual_seed(5)
        model, twin = ToyMLP(**SHAPE), ToyMLP(**SHAPE)
        twin.load_state_dict(model.state_dict())
        ddp = tdp.DDP(model)
        opt, topt = _make(name, ddp.parameters()), _make(name, twin.parameters())
        try:
            ddp.register_fused_optimizer(opt)
            raise AssertionError("register_fused_optimizer accepted " + name)
        except TypeError:
            pass
        for step in range(3):
            x, y = _batch(step, r)
            opt.zero_grad(set_to_none=True)
            tdp.ops.cross_entropy(ddp(x), y).backward()
            opt.step()
            xs, ys = zip(*[_batch(step, k) for k in range(ws)])
            topt.zero_grad(set_to_none=True)
            torch.nn.functional.cross_entropy(twin(torch.cat(xs)), torch.cat(ys)).backward()
            topt.step()
        worst = max((p.detach() - q.detach()).abs().max().item()
                    for p, q in zip(model.parameters(), twin.parameters()))
        print(f"[layerwise ddp] {name} rank {r}: max |ddp - twin| after 3 steps = {worst:.3e}",
              flush=True)
        for p, q in zip(model.parameters(), twin.parameters()):
            torch.testing.assert_close(p.detach(), q.detach(), rtol=1e-4, atol=1e-5)
        mine = [p.detach().clone() for p in model.parameters()]
        every = [None] * ws
        dist.all_gather_object(every, mine)
        for other in every:
            for a, b in zip(other, every[0]):
                assert torch.equal(a, b), "replicas diverged"
        del ddp
    for name in ("lamb", "lars"):
        m = ToyMLP(**SHAPE)
        o = _make(name, m.parameters())
        m, o = acc.prepare(m, o)
        assert acc.ddp_of(m) is not None
        assert acc.fuse_optimizer(m, o) is False
    if tdp.parallel.is_initialized():
        tdp.destroy_process_group()
