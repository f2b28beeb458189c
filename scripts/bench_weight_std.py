"""Weight-standardisation micro-benchmark on one MI355X (profiles/r23/weight_std.md).

Per distinct convolution-weight geometry of ResNet-50 (the layout ``tdp.nn.Conv2d`` keeps it in),
call time by device events -- back-to-back launches, so launch overhead is in the figure -- as
the median of REPEATS interleaved runs of REPS calls, every side in the same process after a
warm-up:
  ours   ops.weight_standardize (csrc/weight_std.hip), forward and backward (one launch each)
  torch  the ATen composition (mean, subtract, square, mean, rsqrt, multiply) and its autograd
         chain on the same tensors
GB/s counts the passes the register form makes: forward reads w and writes w_hat (2), backward
reads g and w_hat and writes dw (3), 4 bytes per element.
--step times the eager SGD step of resnet50_gn_ws next to resnet50_gn (the cost of the feature)
and to a plain torch.nn twin with the composition in every convolution.
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
from tutorial_torch_distributed_data_parallel_amd.models.registry import build_model  # noqa: E402

from bench_groupnorm import stock_resnet50_gn, timeit, warm  # noqa: E402  (scripts/ is sys.path[0])

dev = "cuda"
CL = torch.channels_last
REPEATS = 7
REPS = 200


def compose(w, eps=1e-5):
    mean = w.mean(dim=(1, 2, 3), keepdim=True)
    var = (w - mean).square().mean(dim=(1, 2, 3), keepdim=True)
    return (w - mean) * torch.rsqrt(var + eps)


class TorchStdConv2d(nn.Conv2d):
    def forward(self, x):
        return self._conv_forward(x, compose(self.weight), self.bias)


def bench_geoms():
    model = build_model("resnet50_gn_ws", device=dev)
    seen, rows = {}, []
    for m in model.modules():
        if isinstance(m, nn.Conv2d):
            seen.setdefault(tuple(m.weight.shape), m.weight)
    for shape, p in seen.items():
        w = p.detach().clone(memory_format=torch.preserve_format).requires_grad_()
        g = torch.empty_like(w).normal_()
        fwd = {"ours": lambda: ops.weight_standardize(w), "torch": lambda: compose(w)}
        outs = {k: f() for k, f in fwd.items()}
        sides = {f"{k}_fwd": f for k, f in fwd.items()}
        sides.update({f"{k}_bwd": (lambda y=y: torch.autograd.grad(y, w, g, retain_graph=True))
                      for k, y in outs.items()})
        t = {k: [] for k in sides}
        for _ in range(REPEATS):
            for k, fn in sides.items():
                t[k].append(timeit(fn, REPS))
        K = w[0].numel()
        row = {"weight": "x".join(map(str, shape)), "K": K, "KB": round(4 * w.numel() / 1e3, 1),
               "layout": "channels_last" if shape[1] % 4 == 0 else "contiguous"}
        for k, v in t.items():
            med = statistics.median(v)
            row[f"{k}_us"] = round(med, 2)
            if k.startswith("ours"):
                passes = 2 if k.endswith("fwd") else 3
                row[f"{k}_GBs"] = round(passes * 4 * w.numel() / 1e9 / (med * 1e-6), 1)
        print(json.dumps(row), flush=True)
        rows.append(row)
    return rows


def bench_step(batch):
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

    twin = stock_resnet50_gn()
    for c in twin.modules():
        if type(c) is nn.Conv2d:
            c.__class__ = TorchStdConv2d
    twin = twin.to(dev).to(memory_format=CL).train()
    topt = torch.optim.SGD(twin.parameters(), lr=0.01, momentum=0.9)

    def step_torch():
        topt.zero_grad(set_to_none=True)
        F.cross_entropy(twin(x), y).backward()
        topt.step()

    sides = {"resnet50_gn_ws": ours("resnet50_gn_ws"), "resnet50_gn": ours("resnet50_gn"),
             "torch_gn_ws_twin": step_torch}
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
    if not torch.cuda.is_available():
        raise SystemExit("bench_weight_std: needs a GPU")
    warm()
    out = {"geoms": bench_geoms()}
    if a.step:
        out["step"] = bench_step(a.batch)
    if a.json:
        with open(a.json, "w") as f:
            json.dump(out, f, indent=1)


if __name__ == "__main__":
    main()
