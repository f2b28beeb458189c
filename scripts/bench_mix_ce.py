"""MixUp / CutMix micro-benchmark on one MI355X (profiles/r24/mix_ce.md).

Call time by device events -- back-to-back launches, so launch overhead is in the figure -- as the
median of REPEATS interleaved runs of REPS calls, every side in the same process after a warm-up:
  loss  forward + backward with the unit seed (ops.backward's cached seed on our side, so our
        backward launches nothing; autograd's own seed on torch's), B x 1000 logits:
          dense  ops.cross_entropy(logits, probs)           (csrc/loss_soft.hip)
          pair   ops.cross_entropy_pair(logits, ya, yb, lam)
          torch  F.cross_entropy(logits, probs) on the GPU, the dense target already built
          torch+target  the same plus building the dense target from (ya, yb, lam)
  mix   tdp.data.mix_batch (csrc/mix.hip) against the ATen composition (gather, lerp, where) for
        MixUp (empty boxes, lam = 0.3) and CutMix (lam = 1, a 112 x 112 box), 128 x 3 x 224 x 224
        in both layouts. GB/s counts the bytes the kernel moves: MixUp reads x and the partner and
        writes out (3 passes); CutMix reads one source per element and writes it (2 passes).
"""
import argparse
import json
import statistics
import sys

import torch
import torch.nn.functional as F

sys.path.insert(0, __file__.rsplit("/scripts/", 1)[0])
import tutorial_torch_distributed_data_parallel_amd as tdp  # noqa: E402
from tutorial_torch_distributed_data_parallel_amd import ops  # noqa: E402
from tutorial_torch_distributed_data_parallel_amd.data.mix import reference_mix  # noqa: E402
from tutorial_torch_distributed_data_parallel_amd.ops.loss import pair_target  # noqa: E402

from bench_groupnorm import timeit, warm  # noqa: E402  (scripts/ is sys.path[0])

dev = "cuda"
REPEATS = 7
REPS = 200


def _median_rows(sides, reps):
    for fn in sides.values():
        for _ in range(3):
            fn()
    t = {k: [] for k in sides}
    for _ in range(REPEATS):
        for k, fn in sides.items():
            t[k].append(timeit(fn, reps))
    return {k: statistics.median(v) for k, v in t.items()}


def bench_loss(B, C=1000, eps=0.1):
    gen = torch.Generator().manual_seed(B)
    z = torch.randn(B, C, generator=gen).to(dev).requires_grad_()
    ya, yb = (torch.randint(0, C, (B,), generator=gen).to(dev) for _ in range(2))
    lam = torch.rand(B, generator=gen).to(dev)
    probs = pair_target(ya, yb, lam, C)

    def ours(loss_fn):
        def run():
            z.grad = None
            ops.backward(loss_fn())
        return run

    def torch_side(build):
        def run():
            z.grad = None
            F.cross_entropy(z, pair_target(ya, yb, lam, C) if build else probs,
                            label_smoothing=eps).backward()
        return run

    sides = {"dense": ours(lambda: ops.cross_entropy(z, probs, label_smoothing=eps)),
             "pair": ours(lambda: ops.cross_entropy_pair(z, ya, yb, lam, eps)),
             "torch": torch_side(False), "torch+target": torch_side(True)}
    row = {"loss": f"{B}x{C} eps={eps} fwd+bwd"}
    row.update({f"{k}_us": round(v, 2) for k, v in _median_rows(sides, REPS).items()})
    print(json.dumps(row), flush=True)
    return row


def bench_mix(channels_last, N=128, C=3, H=224, W=224):
    gen = torch.Generator().manual_seed(1)
    x = torch.randn(N, C, H, W, generator=gen).to(dev)
    if channels_last:
        x = x.contiguous(memory_format=torch.channels_last)
    perm = torch.randperm(N, generator=gen).to(dev)
    modes = {"mixup": (torch.full((N,), 0.3), [0, 0, 0, 0]),
             "cutmix": (torch.ones(N), [40, 60, 112, 112])}
    rows = []
    for name, (lam, box) in modes.items():
        lam = lam.to(dev)
        boxes = torch.tensor([box] * N, dtype=torch.int32).to(dev)
        sides = {"ours": lambda: tdp.data.mix_batch(x, perm, lam, boxes),
                 "torch": lambda: reference_mix(x, perm, lam, boxes)}
        med = _median_rows(sides, 20)
        passes = 3 if name == "mixup" else 2
        row = {"mix": f"{name} {N}x{C}x{H}x{W}",
               "layout": "channels_last" if channels_last else "contiguous",
               "ours_us": round(med["ours"], 1), "torch_us": round(med["torch"], 1),
               "ours_GBs": round(passes * 4 * x.numel() / 1e9 / (med["ours"] * 1e-6), 1)}
        print(json.dumps(row), flush=True)
        rows.append(row)
    return rows


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--json", default=None, help="write every row to this file")
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_mix_ce: needs a GPU")
    warm()
    out = {"loss": [bench_loss(B) for B in (128, 256)],
           "mix": bench_mix(False) + bench_mix(True)}
    if a.json:
        with open(a.json, "w") as f:
            json.dump(out, f, indent=1)


if __name__ == "__main__":
    main()
