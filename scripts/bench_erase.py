"""Crop -> augment -> normalise + erase micro-benchmark on one MI355X (profiles/r26/erase.md).

Call time by device events -- back-to-back calls, so launch overhead and the host's draws,
validation and pinned uploads are in the figure -- as the median, with the smallest and the
largest, of REPEATS interleaved runs, every side in the same process after a warm-up, at
128 x 256 x 256 x 3 -> 224 x 224 and 128 x 32 x 32 x 3 -> 32 x 32:
  a_augment_then_crop   AugmentedTransform(TrivialAugment, CropTransform): the augmentation on the
                        source image, then the one-launch float crop
  b_crop_augment_erase  CropTransform(augment=TrivialAugment, erase=RandomErasing(p)): uint8 crop,
                        augmentation on the crop, normalize_erase (torchvision's order)
  c_crop_float          crop_resize to float32 alone (device boxes, no read-back)
  c_crop_u8_finish      crop_resize(out_dtype=uint8) + normalize_erase without boxes: the price
                        of the extra launch when only erasing is wanted
  d_normalize_erase     normalize_erase on the uint8 crop with one box per sample (p = 1),
                        value 0 and value "random"
  d_torch_loop          the eager composition on GPU tensors: ToTensor + Normalize on the batch,
                        then a per-sample loop that assigns the box (torchvision's RandomErasing)
GB/s of normalize_erase counts the bytes it must move: the uint8 batch read, the float32 written.
"""
import argparse
import json
import statistics
import sys

import torch

sys.path.insert(0, __file__.rsplit("/scripts/", 1)[0])
from tutorial_torch_distributed_data_parallel_amd.data import (AugmentedTransform, CropTransform,  # noqa: E402
                                                               RandomErasing, TrivialAugment,
                                                               erase_boxes, normalize_erase,
                                                               reference_normalize_erase)
from tutorial_torch_distributed_data_parallel_amd.data.host import _crop_resize  # noqa: E402

from bench_groupnorm import timeit, warm  # noqa: E402  (scripts/ is sys.path[0])

dev = "cuda"
REPEATS = 5
MEAN, STD = (0.485, 0.456, 0.406), (0.229, 0.224, 0.225)


def _medians(sides):
    t = {k: [] for k in sides}
    for _ in range(REPEATS):
        for k, (fn, reps) in sides.items():
            t[k].append(timeit(fn, reps))
    return {k: (statistics.median(v), min(v), max(v)) for k, v in t.items()}


def torch_loop(u8, boxes_list, mean, std, value):
    y = ((u8.permute(0, 3, 1, 2).float() / 255.0 - mean) / std).contiguous(
        memory_format=torch.channels_last)
    for n, (t, l, h, w) in enumerate(boxes_list):
        if h and w:
            if value == "random":
                y[n, :, t:t + h, l:l + w] = torch.empty(3, h, w, device=y.device).normal_()
            else:
                y[n, :, t:t + h, l:l + w] = value
    return y


def bench(N, Hs, size, reps):
    g = torch.Generator().manual_seed(Hs)
    x = torch.randint(0, 256, (N, Hs, Hs, 3), dtype=torch.uint8, generator=g).to(dev)
    flip = torch.randint(0, 2, (N,), dtype=torch.uint8, generator=g).to(dev)
    old = AugmentedTransform(TrivialAugment(), CropTransform(size=size, mean=MEAN, std=STD))
    new = CropTransform(size=size, mean=MEAN, std=STD, augment=TrivialAugment(),
                        erase=RandomErasing(p=0.1))
    new_p1 = CropTransform(size=size, mean=MEAN, std=STD, augment=TrivialAugment(),
                           erase=RandomErasing(p=1.0))
    for t in (old, new, new_p1):
        t.start_epoch(1)
    cb = new.boxes(N, Hs, Hs).to(dev)
    crop = lambda dt: _crop_resize(x, cb, flip, size, MEAN, STD, True, True, 0.0, dt, False)  # noqa: E731
    u8 = crop(torch.uint8)
    assert torch.equal(normalize_erase(u8, MEAN, STD), crop(torch.float32))
    eb = erase_boxes(N, size, size, p=1.0, generator=g)
    ebd, ebl = eb.to(dev), eb.tolist()
    assert torch.equal(normalize_erase(u8, MEAN, STD, ebd, 0.0),
                       reference_normalize_erase(u8, MEAN, STD, eb, 0.0))
    m = torch.tensor(MEAN, device=dev).view(1, 3, 1, 1)
    s = torch.tensor(STD, device=dev).view(1, 3, 1, 1)
    sides = {
        "a_augment_then_crop": (lambda: old(x, flip), reps),
        "b_crop_augment_erase_p0.1": (lambda: new(x, flip), reps),
        "b_crop_augment_erase_p1": (lambda: new_p1(x, flip), reps),
        "c_crop_float": (lambda: crop(torch.float32), reps),
        "c_crop_u8_finish": (lambda: normalize_erase(crop(torch.uint8), MEAN, STD), reps),
        "c_crop_u8": (lambda: crop(torch.uint8), reps),
        "d_normalize_only": (lambda: normalize_erase(u8, MEAN, STD), reps),
        "d_normalize_erase_0": (lambda: normalize_erase(u8, MEAN, STD, ebd, 0.0), reps),
        "d_normalize_erase_random": (lambda: normalize_erase(u8, MEAN, STD, ebd, "random", 7), reps),
        "d_normalize_erase_0_planar": (lambda: normalize_erase(u8, MEAN, STD, ebd, 0.0,
                                                               channels_last=False), reps),
        "d_torch_loop_0": (lambda: torch_loop(u8, ebl, m, s, 0.0), 10),
        "d_torch_loop_random": (lambda: torch_loop(u8, ebl, m, s, "random"), 10),
    }
    med = _medians(sides)
    r = {"shape": f"{N}x{Hs}x{Hs}x3->{size}"}
    for k, (mid, lo, hi) in med.items():
        r[f"{k}_us"], r[f"{k}_minmax"] = round(mid, 1), [round(lo, 1), round(hi, 1)]
    r["d_normalize_only_GBs"] = round(5 * u8.numel() / 1e9 / (med["d_normalize_only"][0] * 1e-6), 1)
    print(json.dumps(r), flush=True)
    return r


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--json", default=None, help="write every row to this file")
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_erase: needs a GPU")
    warm()
    out = [bench(128, 256, 224, 300), bench(128, 32, 32, 1000)]
    if a.json:
        with open(a.json, "w") as f:
            json.dump(out, f, indent=1)


if __name__ == "__main__":
    main()
