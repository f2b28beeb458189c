"""GroupNorm micro-benchmark on one MI355X (profiles/r20/groupnorm.md).

Per distinct GroupNorm geometry of ``resnet50_gn`` (32 groups) at batch 32, 224 x 224 input, on
channels_last tensors with a fused ReLU (event timing, the median of REPEATS interleaved runs of
REPS launches, every side in the same process after a warm-up):
  ours   ops.group_norm(relu=True): csrc/groupnorm.hip, NHWC form
  torch  F.relu(F.group_norm(.)) on channels_last tensors
  bn     ops.batch_norm(relu=True, training): the project's BatchNorm kernels at the same shape,
         the bandwidth yardstick
forward and backward (input, weight and bias gradients) separately. GB/s counts the tensor-sized
passes the GroupNorm kernels make: forward 3 (statistics read x; normalise reads x, writes y),
backward 5 (reduce reads dy, x; elementwise reads dy, x, writes dx), 4 bytes per element.
--step times the eager SGD step of resnet50_gn next to a plain torch.nn twin (channels_last,
torch.optim.SGD) and to the project's BatchNorm resnet50.
"""
import argparse
import json
import statistics
import sys

import torch
import torch.nn as nn
import torch.nn.functional as F

sys.path.insert(0, __file__.rsplit("/scripts/", 1)[0])
import tutorial_torch_distributed_data_parallel_amd as tdp  # noqa: E402
from tutorial_torch_distributed_data_parallel_amd import ops  # noqa: E402

dev = "cuda"
CL = torch.channels_last
REPEATS = 7
REPS = 20
GROUPS = 32
# (channels, extent) of every distinct GroupNorm input of ResNet-50 at 224 x 224
GEOMS = [(64, 112), (64, 56), (256, 56), (128, 56), (128, 28), (512, 28), (256, 28), (256, 14),
         (1024, 14), (512, 14), (512, 7), (2048, 7)]


def timeit(fn, reps):
    ev = [torch.cuda.Event(enable_timing=True) for _ in range(2)]
    fn()
    torch.cuda.synchronize()
    ev[0].record()
    for _ in range(reps):
        fn()
    ev[1].record()
    torch.cuda.synchronize()
    return ev[0].elapsed_time(ev[1]) / reps * 1000.0


def warm():
    x = torch.randn(4096, 4096, device=dev)
    for _ in range(40):
        torch.mm(x, x)
    torch.cuda.synchronize()


def bench_geoms(batch):
    rows = []
    for ch, h in GEOMS:
        x = torch.randn(batch, ch, h, h, device=dev).contiguous(memory_format=CL).requires_grad_()
        dy = torch.randn(batch, ch, h, h, device=dev).contiguous(memory_format=CL)
        w = torch.rand(ch, device=dev).add_(0.5).requires_grad_()
        b = torch.randn(ch, device=dev).requires_grad_()

        fwd = {"ours": lambda: ops.group_norm(x, GROUPS, w, b, relu=True),
               "torch": lambda: F.relu(F.group_norm(x, GROUPS, w, b)),
               "bn": lambda: ops.batch_norm(x, None, None, w, b, training=True, relu=True)}
        outs = {k: f() for k, f in fwd.items()}

        def bwd_of(y):
            return lambda: torch.autograd.grad(y, (x, w, b), dy, retain_graph=True)

        sides = {f"{k}_fwd": f for k, f in fwd.items()}
        sides.update({f"{k}_bwd": bwd_of(y) for k, y in outs.items()})
        t = {k: [] for k in sides}
        for _ in range(REPEATS):
            for k, fn in sides.items():
                t[k].append(timeit(fn, REPS))
        mb = 4.0 * x.numel() / 1e6
        row = {"geom": f"{ch}@{h}x{h} Cg={ch // GROUPS}", "MB": round(mb, 1)}
        for k, v in t.items():
            med = statistics.median(v)
            passes = 3 if k.endswith("fwd") else 5
            row[f"{k}_us"] = round(med, 1)
            row[f"{k}_GBs"] = round(passes * mb / 1e3 / (med * 1e-6))
        print(json.dumps(row), flush=True)
        rows.append(row)
    return rows


class _Block(nn.Module):
    def __init__(self, inp, planes, stride, ds):
        super().__init__()
        self.body = nn.Sequential(
            nn.Conv2d(inp, planes, 1, bias=False), nn.GroupNorm(GROUPS, planes), nn.ReLU(),
            nn.Conv2d(planes, planes, 3, stride, 1, bias=False), nn.GroupNorm(GROUPS, planes),
            nn.ReLU(), nn.Conv2d(planes, planes * 4, 1, bias=False),
            nn.GroupNorm(GROUPS, planes * 4))
        self.ds = ds

    def forward(self, x):
        return F.relu(self.body(x) + (x if self.ds is None else self.ds(x)))


def stock_resnet50_gn(num_classes=10):
    layers = [nn.Conv2d(3, 64, 7, 2, 3, bias=False), nn.GroupNorm(GROUPS, 64), nn.ReLU(),
              nn.MaxPool2d(3, 2, 1)]
    inp = 64
    for planes, blocks, stride in ((64, 3, 1), (128, 4, 2), (256, 6, 2), (512, 3, 2)):
        for i in range(blocks):
            s = stride if i == 0 else 1
            ds = None
            if s != 1 or inp != planes * 4:
                ds = nn.Sequential(nn.Conv2d(inp, planes * 4, 1, s, bias=False),
                                   nn.GroupNorm(GROUPS, planes * 4))
            layers.append(_Block(inp, planes, s, ds))
            inp = planes * 4
    return nn.Sequential(*layers, nn.AdaptiveAvgPool2d(1), nn.Flatten(),
                         nn.Linear(2048, num_classes))


def bench_step(batch):
    from tutorial_torch_distributed_data_parallel_amd.models.registry import build_model

    torch.manual_seed(0)
    x = torch.randn(batch, 3, 224, 224, device=dev).contiguous(memory_format=CL)
    y = torch.randint(0, 10, (batch,), device=dev)

    def ours(name):
        m = build_model(name, device=dev).train()
        opt = tdp.optim.SGD(m.parameters(), lr=0.01, momentum=0.9)

        def run():
            opt.zero_grad(set_to_none=True)
            tdp.ops.cross_entropy(m(x), y).backward()
            opt.step()
        return run

    twin = stock_resnet50_gn().to(dev).to(memory_format=CL).train()
    topt = torch.optim.SGD(twin.parameters(), lr=0.01, momentum=0.9)

    def step_torch():
        topt.zero_grad(set_to_none=True)
        F.cross_entropy(twin(x), y).backward()
        topt.step()

    sides = {"resnet50_gn": ours("resnet50_gn"), "torch_gn_twin": step_torch,
             "resnet50_bn": ours("resnet50")}
    for fn in sides.values():
        for _ in range(3):
            fn()
    t = {k: [] for k in sides}
    for _ in range(REPEATS):
        for k, fn in sides.items():
            t[k].append(timeit(fn, 5))
    row = {"step": f"sgd b{batch} 224 eager"}
    for k, v in t.items():
        row[f"{k}_ms"] = round(statistics.median(v) / 1e3, 2)
        row[f"{k}_spread_ms"] = round((max(v) - min(v)) / 1e3, 2)
    print(json.dumps(row), flush=True)
    return row


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=32)
    ap.add_argument("--step", action="store_true", help="also time the eager SGD step")
    ap.add_argument("--json", default=None, help="write every row to this file")
    a = ap.parse_args()
    warm()
    out = {"geoms": bench_geoms(a.batch)}
    if a.step:
        out["step"] = bench_step(a.batch)
    if a.json:
        with open(a.json, "w") as f:
            json.dump(out, f, indent=1)


if __name__ == "__main__":
    main()
