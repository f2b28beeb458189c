"""Grouped and depthwise convolution (csrc/conv_grouped.hip) on the grouped 3x3 geometries of
ResNeXt-50 32x4d at batch 32 (stride 1 and the stride-2 variants) and on depthwise 3x3 layers of
the MobileNet family: forward, input gradient, weight gradient. One process, device warm-up,
event timing, the median of REPEATS interleaved runs of 20 launches. Baselines, same session:
  (a) torch: torch.nn.functional.conv2d(groups=) and torch.nn.grad on channels_last tensors;
  (b) naive (grouped family only): `groups` dense native convolutions on copied channel slices,
      what the code before the grouped kernels could do.
One JSON line per (layer, pass); the depthwise rows also give achieved GB/s against the bytes
the pass must move (each operand read once, the result written once).

--step times an eager ResNeXt-50 SGD step (batch 32, 224 x 224) next to a torch.nn twin.

python scripts/bench_conv_grouped.py [--step] [--md OUT.md]"""
import argparse
import json
import statistics
import sys

import torch
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
# name, N, C, H, W, Cout, R, stride, pad, groups
LAYERS = [(f"resnext50.layer{i + 1}.3x3{'s2' if s == 2 else ''}", 32, c, h, h, c, 3, s, 1, 32)
          for i, (c, h) in enumerate([(128, 56), (256, 28), (512, 14), (1024, 7)])
          for s in (1, 2)]
LAYERS += [(f"depthwise.{c}@{h}", 32, c, h, h, c, 3, 1, 1, c)
           for c, h in [(32, 112), (96, 56), (192, 28), (576, 14)]]


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


def passes(N, Cin, H, W, Cout, R, s, p, groups):
    """{pass: {side: fn}} for one layer, and the bytes each pass must move"""
    Cg, Kg = Cin // groups, Cout // groups
    P, Q = (H + 2 * p - R) // s + 1, (W + 2 * p - R) // s + 1
    torch.manual_seed(N + Cin + H + Cout)
    x = torch.randn(N, Cin, H, W, device=dev).contiguous(memory_format=CL)
    w = torch.randn(Cout, Cg, R, R, device=dev)
    if Cg % 4 == 0:
        w = w.contiguous(memory_format=CL)
    g = torch.randn(N, Cout, P, Q, device=dev).contiguous(memory_format=CL)
    dw = torch.empty_like(w)
    geom = (s, s, p, p, groups)
    ours = {"fwd": lambda: C.conv_grouped_fwd(x, w, None, *geom),
            "dgrad": lambda: C.conv_grouped_dgrad(g, w, list(x.shape), *geom),
            "wgrad": lambda: C.conv_grouped_wgrad(g, x, dw, *geom)}
    stock = {"fwd": lambda: F.conv2d(x, w, None, s, p, 1, groups),
             "dgrad": lambda: torch.nn.grad.conv2d_input(x.shape, w, g, s, p, 1, groups),
             "wgrad": lambda: torch.nn.grad.conv2d_weight(x, w.shape, g, s, p, 1, groups)}
    out = {k: {"ours": ours[k], "torch": stock[k]} for k in ours}
    if Cg > 1:
        # the naive alternative: per group, copy the channel slices (native copy4d), run the dense
        # NHWC convolution, copy the result slice back
        xs = torch.empty(N, Cg, H, W, device=dev).contiguous(memory_format=CL)
        gs = torch.empty(N, Kg, P, Q, device=dev).contiguous(memory_format=CL)
        y = torch.empty(N, Cout, P, Q, device=dev).contiguous(memory_format=CL)
        dx = torch.empty_like(x)
        dws = torch.empty(Kg, R, R, Cg, device=dev)

        def n_fwd():
            for i in range(groups):
                C.copy4d(xs, x[:, i * Cg:(i + 1) * Cg])
                wi = w[i * Kg:(i + 1) * Kg]
                C.copy4d(y[:, i * Kg:(i + 1) * Kg],
                         C.conv_nhwc_fwd(xs, wi.permute(0, 2, 3, 1), None, R, R, s, s, p, p, False))

        def n_dgrad():
            for i in range(groups):
                C.copy4d(gs, g[:, i * Kg:(i + 1) * Kg])
                wi = w[i * Kg:(i + 1) * Kg]
                if s == 1:
                    d = C.conv_nhwc_dgrad_w(gs, wi, list(xs.shape), 1, 1, p, p)
                else:
                    d = convmod._dgrad_phases(C, gs, wi, xs.shape, R, R, s, s, p, p)
                C.copy4d(dx[:, i * Cg:(i + 1) * Cg], d)

        def n_wgrad():
            for i in range(groups):
                C.copy4d(xs, x[:, i * Cg:(i + 1) * Cg])
                C.copy4d(gs, g[:, i * Kg:(i + 1) * Kg])
                C.conv_nhwc_wgrad(gs, xs, dws, R, R, s, s, p, p, 0.0)
                C.copy4d(dw[i * Kg:(i + 1) * Kg], dws.permute(0, 3, 1, 2))

        for k, fn in (("fwd", n_fwd), ("dgrad", n_dgrad), ("wgrad", n_wgrad)):
            out[k]["naive"] = fn
    nb = {"fwd": x.numel() + w.numel() + g.numel(), "dgrad": x.numel() + w.numel() + g.numel(),
          "wgrad": x.numel() + w.numel() + g.numel()}
    return out, {k: 4.0 * v for k, v in nb.items()}


def bench_layers():
    rows = []
    for name, *geom in LAYERS:
        fns, nbytes = passes(*geom)
        depthwise = geom[8] == geom[1]
        for pname in ("fwd", "dgrad", "wgrad"):
            sides = fns[pname]
            t = {k: [] for k in sides}
            for _ in range(REPEATS):  # interleaved: drift hits every side alike
                for k, fn in sides.items():
                    t[k].append(timeit(fn, REPS))
            med = {k: statistics.median(v) for k, v in t.items()}
            row = {"layer": name, "pass": pname, "ours_us": round(med["ours"], 1),
                   "ours_spread_us": round(max(t["ours"]) - min(t["ours"]), 1),
                   "torch_us": round(med["torch"], 1),
                   "torch_spread_us": round(max(t["torch"]) - min(t["torch"]), 1),
                   "torch_over_ours": round(med["torch"] / med["ours"], 2)}
            if "naive" in med:
                row["naive_us"] = round(med["naive"], 1)
                row["naive_over_ours"] = round(med["naive"] / med["ours"], 2)
            if depthwise:
                row["gbytes_per_s"] = round(nbytes[pname] / med["ours"] / 1e3, 1)
            rows.append(row)
            print(json.dumps(row), flush=True)
    return rows


class _StockBlock(torch.nn.Module):
    def __init__(self, cin, planes, stride):
        super().__init__()
        nn = torch.nn
        width = planes * 2  # int(planes * 4 / 64) * 32
        self.conv1 = nn.Conv2d(cin, width, 1, bias=False)
        self.bn1 = nn.BatchNorm2d(width)
        self.conv2 = nn.Conv2d(width, width, 3, stride, 1, groups=32, bias=False)
        self.bn2 = nn.BatchNorm2d(width)
        self.conv3 = nn.Conv2d(width, planes * 4, 1, bias=False)
        self.bn3 = nn.BatchNorm2d(planes * 4)
        self.downsample = None
        if stride != 1 or cin != planes * 4:
            self.downsample = nn.Sequential(nn.Conv2d(cin, planes * 4, 1, stride, bias=False),
                                            nn.BatchNorm2d(planes * 4))

    def forward(self, x):
        out = F.relu(self.bn1(self.conv1(x)))
        out = F.relu(self.bn2(self.conv2(out)))
        idn = x if self.downsample is None else self.downsample(x)
        return F.relu(self.bn3(self.conv3(out)) + idn)


def stock_resnext50(num_classes=10):
    nn = torch.nn
    layers = [nn.Conv2d(3, 64, 7, 2, 3, bias=False), nn.BatchNorm2d(64), nn.ReLU(inplace=True),
              nn.MaxPool2d(3, 2, 1)]
    cin = 64
    for planes, blocks, stride in ((64, 3, 1), (128, 4, 2), (256, 6, 2), (512, 3, 2)):
        for i in range(blocks):
            layers.append(_StockBlock(cin, planes, stride if i == 0 else 1))
            cin = planes * 4
    layers += [nn.AdaptiveAvgPool2d((1, 1)), nn.Flatten(), nn.Linear(2048, num_classes)]
    return nn.Sequential(*layers)


def bench_step():
    from tutorial_torch_distributed_data_parallel_amd.models.registry import build_model

    torch.manual_seed(0)
    x = torch.randn(32, 3, 224, 224, device=dev).contiguous(memory_format=CL)
    y = torch.randint(0, 10, (32,), device=dev)
    ours = build_model("resnext50_32x4d", device=dev).train()
    oopt = tdp.optim.SGD(ours.parameters(), lr=0.01, momentum=0.9)
    twin = stock_resnext50().to(dev).to(memory_format=CL).train()
    topt = torch.optim.SGD(twin.parameters(), lr=0.01, momentum=0.9)

    def step_ours():
        oopt.zero_grad(set_to_none=True)
        tdp.ops.cross_entropy(ours(x), y).backward()
        oopt.step()

    def step_torch():
        topt.zero_grad(set_to_none=True)
        F.cross_entropy(twin(x), y).backward()
        topt.step()

    sides = {"ours": step_ours, "torch": step_torch}
    for fn in sides.values():
        for _ in range(3):
            fn()
    t = {k: [] for k in sides}
    for _ in range(REPEATS):
        for k, fn in sides.items():
            t[k].append(timeit(fn, 5))
    row = {"step": "resnext50_32x4d sgd b32 eager"}
    for k, v in t.items():
        row[f"{k}_ms"] = round(statistics.median(v) / 1e3, 2)
        row[f"{k}_spread_ms"] = round((max(v) - min(v)) / 1e3, 2)
    print(json.dumps(row), flush=True)
    return row


def write_md(path, rows, step):
    lines = ["| layer | pass | ours us (spread) | torch us (spread) | torch / ours | naive us |"
             " naive / ours | GB/s |", "|---|---|---|---|---|---|---|---|"]
    for r in rows:
        lines.append(f"| {r['layer']} | {r['pass']} | {r['ours_us']} ({r['ours_spread_us']}) | "
                     f"{r['torch_us']} ({r['torch_spread_us']}) | {r['torch_over_ours']} | "
                     f"{r.get('naive_us', '')} | {r.get('naive_over_ours', '')} | "
                     f"{r.get('gbytes_per_s', '')} |")
    slower = [f"- {r['layer']} {r['pass']}: {r['ours_us']} us against {r['torch_us']} us"
              for r in rows if r["torch_over_ours"] < 1.0]
    lines += ["", "Rows slower than torch (a):", *(slower or ["- none"])]
    if step:
        lines += ["", "Eager step: " + json.dumps(step)]
    with open(path, "w") as f:
        f.write("\n".join(lines) + "\n")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--step", action="store_true")
    ap.add_argument("--md", default=None)
    a = ap.parse_args()
    assert torch.cuda.is_available(), "bench_conv_grouped needs a GPU"
    warm()
    rows = bench_layers()
    step = bench_step() if a.step else None
    if a.md:
        write_md(a.md, rows, step)


if __name__ == "__main__":
    main()
