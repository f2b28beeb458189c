"""Worker for the two-rank gloo test of MobileNetV2; runs under parallel.launcher.spawn."""
import copy

import torch
import torch.nn.functional as F

import tutorial_torch_distributed_data_parallel_amd as tdp
from tutorial_torch_distributed_data_parallel_amd.models.mobilenet import MobileNetV2
from tutorial_torch_distributed_data_parallel_amd.parallel import runtime as rt

from mobilenet_twin import TwinMobileNetV2, check_grads_rule, check_rule


def mobilenet_syncbn_ddp_matches_full_batch(rank, out_dir):
    """MobileNetV2 with SyncBatchNorm (fused ReLU6 carried across by the conversion) under
    tdp.DDP, each rank on its half of a batch, against the plain torch.nn twin on the whole batch
    in one process -- what torch's DDP + SyncBatchNorm computes (torch's SyncBatchNorm itself
    takes no CPU tensors, as in ddp_workers.syncbn_parity). Sum-reduced loss: DDP's averaged
    gradients times the world size are the full-batch gradients. Logits and gradients follow the
    project's float64 rule (mobilenet_twin.check_rule): a sum-reduced loss through 52 BatchNorms
    gives gradients of very different magnitudes per tensor, which one atol cannot serve.
    Dropout is off (p = 0): the ranks would draw other masks than the single process."""
    torch.set_num_threads(4)  # two ranks share one host: no oversubscribed spinning
    tdp.init_process_group("gloo")
    r, ws = rt.get_rank(), rt.get_world_size()
    torch.manual_seed(0)
    model = MobileNetV2(num_classes=10, dropout=0.0)
    twin = TwinMobileNetV2(num_classes=10, dropout=0.0)
    twin.load_state_dict(model.state_dict())
    t64 = copy.deepcopy(twin).double()
    model = tdp.nn.convert_sync_batchnorm(model)
    assert sum(getattr(m, "relu6", False) for m in model.modules()) == 35
    assert all(isinstance(m, tdp.nn.SyncBatchNorm) for m in model.modules()
               if isinstance(m, torch.nn.modules.batchnorm._BatchNorm))
    ddp = tdp.DDP(model)
    g = torch.Generator().manual_seed(7)
    X = torch.randn(8, 3, 64, 64, generator=g)
    Y = torch.randint(0, 10, (8,), generator=g)
    per = 8 // ws
    out = ddp(X[r * per:(r + 1) * per])
    tdp.ops.cross_entropy(out, Y[r * per:(r + 1) * per], reduction="sum").backward()
    rout, rout64 = twin(X), t64(X.double())
    F.cross_entropy(rout, Y, reduction="sum").backward()
    F.cross_entropy(rout64, Y, reduction="sum").backward()
    sl = slice(r * per, (r + 1) * per)
    check_rule("logits", out, rout[sl], rout64[sl], rout64.abs().max().item())
    for p in model.parameters():
        p.grad.mul_(ws)
    check_grads_rule("ddp", model, twin, t64)
    tdp.destroy_process_group()
