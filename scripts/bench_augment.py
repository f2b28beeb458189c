"""TrivialAugmentWide micro-benchmark on one MI355X (profiles/r25/augment.md).

Call time by device events -- back-to-back calls, so launch overhead and, for host params, the
host's validation and pinned upload are in the figure -- as the median, with the smallest and the
largest, of REPEATS interleaved runs (2000 calls each for ours and the copy, 200 for torch_flat, 5
for torch), every side in the same process after a warm-up, at 128 x 256 x 256 x 3 and
128 x 32 x 32 x 3:
  ours        tdp.data.augment_batch with device params (statistics + apply launch, always both)
  ours_host   the same with host params (validated, uploaded through a pinned buffer; the
              statistics launch is skipped when no sample needs it): what TrivialAugment runs
  copy        x.clone(), the bandwidth floor of an out-of-place uint8 pass
  torch       reference_augment on the GPU tensors: the eager composition of the same rules,
              sample by sample as a mixed batch needs it
  torch_flat  for the pointwise ops only (Brightness, Color, Posterize, Solarize), the same rules
              on the whole batch viewed as one image -- what a batch of one op could launch
One batch per op (the same params for every sample) and one TrivialAugment draw. GB/s counts the
bytes the kernels must move: the batch read and written, plus one more read for a statistics op.
"""
import argparse
import json
import statistics
import sys

import torch

sys.path.insert(0, __file__.rsplit("/scripts/", 1)[0])
from tutorial_torch_distributed_data_parallel_amd.data import (TrivialAugment, affine_params,  # noqa: E402
                                                               augment_batch, reference_augment)
from tutorial_torch_distributed_data_parallel_amd.data import augment as A  # noqa: E402

from bench_groupnorm import timeit, warm  # noqa: E402  (scripts/ is sys.path[0])

dev = "cuda"
REPEATS = 5
REPS = 2000  # calls per timed window of ours / copy: 20-200 ms of device work
fb = A.float_bits
OPS = {"identity": [A.IDENTITY], "rotate30": [A.AFFINE] + affine_params("rotate", 30),
       "brightness": [A.BRIGHTNESS, fb(1.5)], "color": [A.COLOR, fb(1.5)],
       "contrast": [A.CONTRAST, fb(1.5)], "sharpness": [A.SHARPNESS, fb(1.5)],
       "posterize": [A.POSTERIZE, 4], "solarize": [A.SOLARIZE, fb(128.0)],
       "autocontrast": [A.AUTOCONTRAST], "equalize": [A.EQUALIZE]}
POINTWISE = ("brightness", "color", "posterize", "solarize")


def _medians(sides):
    t = {k: [] for k in sides}
    for _ in range(REPEATS):
        for k, (fn, reps) in sides.items():
            t[k].append(timeit(fn, reps))
    return {k: (statistics.median(v), min(v), max(v)) for k, v in t.items()}


def bench(N, H, W, C=3):
    x = torch.randint(0, 256, (N, H, W, C), dtype=torch.uint8,
                      generator=torch.Generator().manual_seed(H))
    xh, x = x, x.to(dev)  # the CPU reference checks every timed case first
    ta = TrivialAugment()
    ta.start_epoch(1)
    cases = {k: A.make_params([row] * N) for k, row in OPS.items()}
    cases["trivial_augment"] = ta.draw(N, H, W)
    rows = []
    for name, p in cases.items():
        pd = p.to(dev)
        assert torch.equal(augment_batch(x, pd).cpu(), reference_augment(xh, p)), name
        sides = {"ours": (lambda: augment_batch(x, pd), REPS),
                 "ours_host": (lambda: augment_batch(x, p), REPS),
                 "copy": (lambda: x.clone(), REPS),
                 "torch": (lambda: reference_augment(x, p), 5)}
        if name in POINTWISE:
            flat, row = x.view(N * H, W, C), p[0].tolist()
            sides["torch_flat"] = (lambda: A._reference_one(flat, row), 200)
        med = _medians(sides)
        passes = 3 if name in ("contrast", "autocontrast", "equalize") else 2
        r = {"case": name, "shape": f"{N}x{H}x{W}x{C}"}
        for k, (mid, lo, hi) in med.items():
            r[f"{k}_us"], r[f"{k}_minmax"] = round(mid, 1), [round(lo, 1), round(hi, 1)]
        r["ours_GBs"] = round(passes * x.numel() / 1e9 / (med["ours"][0] * 1e-6), 1)
        print(json.dumps(r), flush=True)
        rows.append(r)
    return rows


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--json", default=None, help="write every row to this file")
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_augment: needs a GPU")
    warm()
    out = bench(128, 256, 256) + bench(128, 32, 32)
    if a.json:
        with open(a.json, "w") as f:
            json.dump(out, f, indent=1)


if __name__ == "__main__":
    main()
