"""Attention micro-benchmark on one MI355X (profiles/r22/attention.md).

ViT-S/16 and ViT-B/16 geometry (S = 197, D = 64, H = 6 / 12) at batch 32 and 128, on the packed
``[B, S, 3E]`` projection output, fp32 tensors (event timing, the median of REPEATS interleaved
runs of REPS launches, every side in the same process after a warm-up):
  ours   ops.attention_qkvpacked: csrc/attention.hip
  comp   the plain torch composition softmax((q @ k^T) * scale) @ v on the strided views
  sdpa   F.scaled_dot_product_attention on the same fp32 views
forward, and forward + backward (gradient of the packed input) separately.
"""
import argparse
import json
import statistics
import sys

import torch
import torch.nn.functional as F

sys.path.insert(0, __file__.rsplit("/scripts/", 1)[0])
from tutorial_torch_distributed_data_parallel_amd import ops  # noqa: E402

dev = "cuda"
REPEATS = 7
REPS = 10
GEOMS = [("vit_s16", 6, 32), ("vit_s16", 6, 128), ("vit_b16", 12, 32), ("vit_b16", 12, 128)]
S, D = 197, 64


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


def _views(qkv, H):
    return qkv.unflatten(2, (3, H, D)).permute(2, 0, 3, 1, 4).unbind(0)


def bench(name, H, batch):
    qkv = torch.randn(batch, S, 3 * H * D, device=dev, requires_grad=True)
    dy = torch.randn(batch, S, H * D, device=dev)

    def flat(o):
        return o.transpose(1, 2).reshape(batch, S, H * D)

    def comp():
        q, k, v = _views(qkv, H)
        return flat(torch.softmax((q @ k.transpose(-1, -2)) * D ** -0.5, dim=-1) @ v)

    fwd = {"ours": lambda: ops.attention_qkvpacked(qkv, H), "comp": comp,
           "sdpa": lambda: flat(F.scaled_dot_product_attention(*_views(qkv, H)))}
    sides = {}
    for k, f in fwd.items():
        def nograd(f=f):
            with torch.no_grad():
                return f()
        sides[f"{k}_fwd"] = nograd
        sides[f"{k}_fwdbwd"] = lambda f=f: torch.autograd.grad(f(), (qkv,), dy)
    t = {k: [] for k in sides}
    for _ in range(REPEATS):
        for k, fn in sides.items():
            t[k].append(timeit(fn, REPS))
    # 4 S^2 D flops per (b, h) forward (two GEMMs), 10 S^2 D more in the backward (five GEMMs)
    gf = batch * H * S * S * D / 1e9
    row = {"geom": f"{name} H={H} B={batch}"}
    for k, v in t.items():
        med = statistics.median(v)
        row[f"{k}_us"] = round(med, 1)
        row[f"{k}_spread_us"] = round(max(v) - min(v), 1)
        if k.startswith("ours"):
            row[f"{k}_TFLOPs"] = round((4 if k.endswith("_fwd") else 14) * gf / med * 1e3, 1)
    print(json.dumps(row), flush=True)
    return row


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--json", default=None, help="write every row to this file")
    a = ap.parse_args()
    warm()
    rows = [bench(*g) for g in GEOMS]
    if a.json:
        with open(a.json, "w") as f:
            json.dump(rows, f, indent=1)


if __name__ == "__main__":
    main()
