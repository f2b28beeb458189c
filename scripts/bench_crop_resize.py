"""Time image_crop_resize (csrc/image_crop.hip) on one GPU at batch 128, channels_last, C = 3:

  pad32      32x32 source, RandomCrop(32, padding=4) boxes -> 32x32
  up64       64x64 source, full-image boxes -> 224x224
  rrc256     256x256 source, RandomResizedCrop boxes -> 224x224

against ``image_transform`` (csrc/image.hip: whole-image 2-tap bilinear, no crop) at the same
output size, and against the torch chain on the device (gather each crop from the padded batch,
F.interpolate(antialias=True) per sample, flip, normalise). Event timing: each side runs
``--iters`` launches between two events, the sides alternate over ``--rounds`` rounds after a
warm-up of every shape, and the median round is reported with the max - min spread. GB/s counts
the float output written once (B * C * Ho * Wo * 4 bytes): the output bandwidth achieved.

Usage: python scripts/bench_crop_resize.py [--iters 200] [--rounds 7] [--json PATH]"""
from __future__ import annotations

import argparse
import json
import os
import statistics
import sys

import torch
import torch.nn.functional as F

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from tutorial_torch_distributed_data_parallel_amd.data import (CIFAR_MEAN, CIFAR_STD,  # noqa: E402
                                                               ImageTransform, crop_resize,
                                                               pad_crop_boxes, resized_crop_boxes)

B = 128


def torch_chain(x, boxes_host, flip, size, pad):
    xp = F.pad(x.permute(0, 3, 1, 2).float(), (pad,) * 4)
    y = torch.cat([F.interpolate(xp[b:b + 1, :, t + pad:t + pad + h, l + pad:l + pad + w],
                                 size=size, mode="bilinear", antialias=True, align_corners=False)
                   for b, (t, l, h, w) in enumerate(boxes_host)]).round()
    y = torch.where(flip.bool().view(-1, 1, 1, 1), y.flip(-1), y)
    m = torch.tensor(CIFAR_MEAN, device=x.device).view(1, -1, 1, 1)
    s = torch.tensor(CIFAR_STD, device=x.device).view(1, -1, 1, 1)
    return ((y / 255.0 - m) / s).contiguous(memory_format=torch.channels_last)


def timed(fn, iters):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(iters):
        fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b) * 1e3 / iters  # us per call


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=200)
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--json", default=None)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_crop_resize.py needs a GPU: times from a CPU say nothing here")
    g = torch.Generator().manual_seed(0)
    cases = {
        "pad32": (32, 32, pad_crop_boxes(B, 32, 32, 32, 4, g), 4),
        "up64": (64, 224, torch.tensor([[0, 0, 64, 64]], dtype=torch.int32).repeat(B, 1), 0),
        "rrc256": (256, 224, resized_crop_boxes(B, 256, 256, generator=g), 0),
    }
    results = {}
    for name, (hs, ho, boxes, pad) in cases.items():
        x = torch.randint(0, 256, (B, hs, hs, 3), generator=g, dtype=torch.uint8).cuda()
        flip = (torch.rand(B, generator=g) < 0.5).to(torch.uint8).cuda()
        dbox, hbox, size = boxes.cuda(), boxes.tolist(), (ho, ho)
        tf = ImageTransform(size=ho)
        sides = {
            "crop_resize": lambda: crop_resize(x, dbox, flip, size, CIFAR_MEAN, CIFAR_STD),
            "image_transform": lambda: tf(x, flip),
            "torch_chain": lambda: torch_chain(x, hbox, flip, size, pad),
        }
        # crop_resize with device boxes reads them back to validate: time the launch path the
        # loader uses (host boxes, validated before a non-blocking upload) as a side of its own
        pinned = torch.empty_like(boxes, pin_memory=True).copy_(boxes)
        sides["crop_resize_host_boxes"] = lambda: crop_resize(x, pinned, flip, size, CIFAR_MEAN,
                                                              CIFAR_STD)
        d = (sides["crop_resize"]() - sides["torch_chain"]()).abs()
        for fn in sides.values():  # warm every side at this shape
            timed(fn, 3)
        torch.cuda.synchronize()
        t = {k: [] for k in sides}
        for _ in range(a.rounds):
            for k, fn in sides.items():
                t[k].append(timed(fn, a.iters if k != "torch_chain" else max(2, a.iters // 10)))
        out_bytes = B * 3 * ho * ho * 4
        results[name] = {
            "output_mb": out_bytes / 1e6,
            "max_abs_diff_vs_torch_chain": float(d.max()),
            "share_differing_vs_torch_chain": float((d > 1e-4).float().mean()),
            **{k: {"us": statistics.median(v), "spread_us": max(v) - min(v),
                   "out_gbps": out_bytes / statistics.median(v) / 1e3} for k, v in t.items()}}
        print(name, json.dumps(results[name]), flush=True)
    if a.json:
        os.makedirs(os.path.dirname(os.path.abspath(a.json)), exist_ok=True)
        with open(a.json, "w") as f:
            json.dump(results, f, indent=1)


if __name__ == "__main__":
    main()
