"""Worker for the two-rank gloo test of EfficientNet-B0; runs under parallel.launcher.spawn."""
import copy

import torch
import torch.nn.functional as F
from torch.nn.parallel import DistributedDataParallel as TorchDDP

import tutorial_torch_distributed_data_parallel_amd as tdp
from tutorial_torch_distributed_data_parallel_amd.models.efficientnet import EfficientNet
from tutorial_torch_distributed_data_parallel_amd.parallel import runtime as rt

from efficientnet_twin import TwinEfficientNetB0, check_grads_rule, check_rule


def efficientnet_ddp_step_matches_torch_ddp(rank, out_dir):
    """One step of EfficientNet-B0 (fused SiLU BatchNorms, squeeze-excitation, fused residual
    joins) under tdp.DDP over gloo, each rank on its half of a batch, against torch's own
    DistributedDataParallel on the plain torch.nn twin over the same process group: per-rank
    BatchNorm statistics on both sides, gradients averaged over the ranks by both. Logits and
    averaged gradients follow the project's float64 rule (mobilenet_twin.check_rule), the
    float64 reference being a second torch-DDP twin. Stochastic depth and dropout are off
    (p = 0): each side would draw other masks."""
    torch.set_num_threads(4)  # two ranks share one host: no oversubscribed spinning
    tdp.init_process_group("gloo")
    r, ws = rt.get_rank(), rt.get_world_size()
    torch.manual_seed(0)
    model = EfficientNet(num_classes=10, stochastic_depth_prob=0.0, dropout=0.0)
    twin = TwinEfficientNetB0(num_classes=10, stochastic_depth_prob=0.0, dropout=0.0)
    twin.load_state_dict(model.state_dict())
    t64 = copy.deepcopy(twin).double()
    assert sum(getattr(m, "silu", False) for m in model.modules()) == 33
    ddp = tdp.DDP(model)
    tddp, tddp64 = TorchDDP(twin), TorchDDP(t64)
    g = torch.Generator().manual_seed(7)
    X = torch.randn(8, 3, 64, 64, generator=g)
    Y = torch.randint(0, 10, (8,), generator=g)
    per = 8 // ws
    sl = slice(r * per, (r + 1) * per)
    out = ddp(X[sl])
    tdp.ops.cross_entropy(out, Y[sl]).backward()
    rout, rout64 = tddp(X[sl]), tddp64(X[sl].double())
    F.cross_entropy(rout, Y[sl]).backward()
    F.cross_entropy(rout64, Y[sl]).backward()
    check_rule("logits", out, rout, rout64, rout64.abs().max().item())
    check_grads_rule("ddp", model, twin, t64)
    tdp.destroy_process_group()
