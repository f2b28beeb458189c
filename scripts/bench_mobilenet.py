"""MobileNetV2 micro-benchmark on one MI355X (profiles/r18/mobilenet_v2.md).

Per depthwise layer of the network at batch 32, 224 x 224 input (event timing, the median of
REPEATS interleaved runs of REPS launches, both sides in the same process after a warm-up):
  fwd        the depthwise forward alone (csrc/conv_grouped.hip)
  fwd+mom    forward, then BatchNorm's moments pass over its output (what runs today)
  fwd_stats  forward with the statistics epilogue, then the merge of its [T, 3, C] partials
  torch      F.conv2d(groups=C) on channels_last tensors (MIOpen)
GB/s counts the input and the output tensor once each.
--step times the eager SGD step of the whole model with ops.conv.DW_BN_STATS off and on, next
to a plain torch.nn twin on channels_last tensors with torch.optim.SGD.
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
from tutorial_torch_distributed_data_parallel_amd._native import native  # noqa: E402
from tutorial_torch_distributed_data_parallel_amd.ops import conv as convmod  # noqa: E402

C = native()
dev = "cuda"
CL = torch.channels_last
REPEATS = 7
REPS = 20
# the distinct depthwise 3x3 layers of MobileNetV2 at width 1.0: (channels, input extent, stride)
LAYERS = [(32, 112, 1), (96, 112, 2), (144, 56, 1), (144, 56, 2), (192, 28, 1), (192, 28, 2),
          (384, 14, 1), (576, 14, 1), (576, 14, 2), (960, 7, 1)]
SETTING = ((1, 16, 1, 1), (6, 24, 2, 2), (6, 32, 3, 2), (6, 64, 4, 2), (6, 96, 3, 1),
           (6, 160, 3, 2), (6, 320, 1, 1))


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


def bench_layers(batch):
    rows = []
    for ch, h, s in LAYERS:
        x = torch.randn(batch, ch, h, h, device=dev).contiguous(memory_format=CL)
        w = torch.randn(ch, 1, 3, 3, device=dev) * 0.2
        y = C.conv_grouped_fwd(x, w, None, s, s, 1, 1, ch, False)
        n = float(y.numel() // ch)

        def fwd():
            return C.conv_grouped_fwd(x, w, None, s, s, 1, 1, ch, False)

        def fwd_mom():
            o = C.conv_grouped_fwd(x, w, None, s, s, 1, 1, ch, False)
            return C.bn_moments(o.permute(0, 2, 3, 1).reshape(-1, ch))

        def fwd_stats():
            o, part = C.conv_dw_fwd_stats(x, w, s, s, 1, 1, ch)
            return C.bn_moments_partials(part, n)

        def torch_fwd():
            return F.conv2d(x, w, None, s, 1, 1, ch)

        sides = {"fwd": fwd, "fwd_mom": fwd_mom, "fwd_stats": fwd_stats, "torch": torch_fwd}
        t = {k: [] for k in sides}
        for _ in range(REPEATS):
            for k, fn in sides.items():
                t[k].append(timeit(fn, REPS))
        gb = 4.0 * (x.numel() + y.numel()) / 1e9
        row = {"layer": f"dw3x3 {ch}@{h} s{s}", "MB": round(gb * 1e3, 1)}
        for k, v in t.items():
            med = statistics.median(v)
            row[f"{k}_us"] = round(med, 1)
            row[f"{k}_GBs"] = round(gb / (med * 1e-6))
        print(json.dumps(row), flush=True)
        rows.append(row)
    return rows


def _cbr(cin, cout, k=3, s=1, g=1):
    return nn.Sequential(nn.Conv2d(cin, cout, k, s, (k - 1) // 2, groups=g, bias=False),
                         nn.BatchNorm2d(cout), nn.ReLU6())


class _Block(nn.Module):
    def __init__(self, inp, oup, s, t):
        super().__init__()
        hid = inp * t
        self.res = s == 1 and inp == oup
        layers = [_cbr(inp, hid, 1)] if t != 1 else []
        layers += [_cbr(hid, hid, 3, s, hid), nn.Conv2d(hid, oup, 1, bias=False),
                   nn.BatchNorm2d(oup)]
        self.conv = nn.Sequential(*layers)

    def forward(self, x):
        return x + self.conv(x) if self.res else self.conv(x)


def stock_mobilenet_v2(num_classes=10):
    feats, inp = [_cbr(3, 32, 3, 2)], 32
    for t, c, n, s in SETTING:
        for i in range(n):
            feats.append(_Block(inp, c, s if i == 0 else 1, t))
            inp = c
    feats.append(_cbr(inp, 1280, 1))
    return nn.Sequential(*feats, nn.AdaptiveAvgPool2d(1), nn.Flatten(), nn.Dropout(0.2),
                         nn.Linear(1280, num_classes))


def bench_step(batch):
    from tutorial_torch_distributed_data_parallel_amd.models.registry import build_model

    torch.manual_seed(0)
    x = torch.randn(batch, 3, 224, 224, device=dev).contiguous(memory_format=CL)
    y = torch.randint(0, 10, (batch,), device=dev)
    ours = build_model("mobilenet_v2", device=dev).train()
    oopt = tdp.optim.SGD(ours.parameters(), lr=0.01, momentum=0.9)
    twin = stock_mobilenet_v2().to(dev).to(memory_format=CL).train()
    topt = torch.optim.SGD(twin.parameters(), lr=0.01, momentum=0.9)

    def step_ours(stats):
        def run():
            convmod.DW_BN_STATS = stats
            oopt.zero_grad(set_to_none=True)
            tdp.ops.cross_entropy(ours(x), y).backward()
            oopt.step()
        return run

    def step_torch():
        topt.zero_grad(set_to_none=True)
        F.cross_entropy(twin(x), y).backward()
        topt.step()

    old = convmod.DW_BN_STATS
    sides = {"ours_stats_off": step_ours(False), "ours_stats_on": step_ours(True),
             "torch": step_torch}
    for fn in sides.values():
        for _ in range(3):
            fn()
    t = {k: [] for k in sides}
    for _ in range(REPEATS):
        for k, fn in sides.items():
            t[k].append(timeit(fn, 5))
    convmod.DW_BN_STATS = old
    row = {"step": f"mobilenet_v2 sgd b{batch} 224 eager"}
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
    out = {"layers": bench_layers(a.batch)}
    if a.step:
        out["step"] = bench_step(a.batch)
    if a.json:
        with open(a.json, "w") as f:
            json.dump(out, f, indent=1)


if __name__ == "__main__":
    main()
