"""Mixed-precision convolution (csrc/conv_bf16.hip: operands rounded once to bf16, one MFMA product
per K16 step) next to the fp32 NHWC convolution (gemm_f32_fast.hip: split-bf16, six products, with
its measured plan table) on the AlexNet convolutions at batch 128 and three ResNet-50 geometries
at batch 32 (a 3x3 stride 1, a 1x1, the strided 3x3): forward, input gradient, weight gradient,
interleaved in one process: event timing, warm-up, REPEATS timed runs of each. One JSON line per
(layer, pass) with the median of each, the spread (max - min) of the fp32 runs, and whether the gap
exceeds that spread. Each side runs the calls ops/conv.py makes for that pass (stride phases, the
fp32 path's transposed weight gradient and its copy included).

--step times an eager AlexNet SGD step (batch 128) without tdp.autocast, with it, and with it
while ops.conv.AUTOCAST_FP32_CONV keeps the convolutions fp32 (the Linear contribution alone).

python scripts/bench_conv_bf16.py [--step] [--md OUT.md]"""
import argparse
import json
import statistics
import sys

import torch

sys.path.insert(0, __file__.rsplit("/scripts/", 1)[0])
import tutorial_torch_distributed_data_parallel_amd as tdp  # noqa: E402
from tutorial_torch_distributed_data_parallel_amd._native import native  # noqa: E402
from tutorial_torch_distributed_data_parallel_amd.ops import conv as convmod  # noqa: E402
from tutorial_torch_distributed_data_parallel_amd.ops import plan_db  # noqa: E402

C = native()
dev = "cuda"
CL = torch.channels_last
REPEATS = 7
# name, N, C, H, W, Cout, R, stride, pad
LAYERS = [("alexnet.features.0", 128, 3, 224, 224, 64, 11, 4, 2),
          ("alexnet.features.3", 128, 64, 27, 27, 192, 5, 1, 2),
          ("alexnet.features.6", 128, 192, 13, 13, 384, 3, 1, 1),
          ("alexnet.features.8", 128, 384, 13, 13, 256, 3, 1, 1),
          ("alexnet.features.10", 128, 256, 13, 13, 256, 3, 1, 1),
          ("resnet50.layer2.3x3", 32, 128, 28, 28, 128, 3, 1, 1),
          ("resnet50.layer3.1x1", 32, 256, 14, 14, 1024, 1, 1, 0),
          ("resnet50.layer3.3x3s2", 32, 256, 28, 28, 256, 3, 2, 1)]


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


def passes(N, Cin, H, W, Cout, R, s, p):
    """{pass: fn(bf16)} -- the native calls of ops/conv.py's _ConvNHWCFn for this layer"""
    Cp = (Cin + 3) // 4 * 4
    P, Q = (H + 2 * p - R) // s + 1, (W + 2 * p - R) // s + 1
    torch.manual_seed(N + Cin + H + Cout)
    xp = torch.randn(N, Cp, H, W, device=dev).contiguous(memory_format=CL)
    wt = torch.randn(Cout, Cp, R, R, device=dev).contiguous(memory_format=CL)
    g = torch.randn(N, Cout, P, Q, device=dev).contiguous(memory_format=CL)
    w2 = wt.permute(0, 2, 3, 1)
    dwt = torch.empty(Cout, R, R, Cp, device=dev)
    dwT = torch.empty(R, R, Cp, Cout, device=dev)
    dw = torch.empty(Cout, Cp, R, R, device=dev).contiguous(memory_format=CL)

    def fwd(bf16):
        C.conv_nhwc_fwd(xp, w2, None, R, R, s, s, p, p, False, bf16=bf16)

    def dgrad(bf16):
        if s == 1:
            C.conv_nhwc_dgrad_w(g, wt, list(xp.shape), 1, 1, p, p, bf16=bf16)
        else:
            convmod._dgrad_phases(C, g, wt, xp.shape, R, R, s, s, p, p, bf16=bf16)

    def wgrad(bf16):
        if not bf16 and C.conv_wgrad_transposed(Cout, R, R, Cp):
            C.conv_nhwc_wgrad(g, xp, dwT, R, R, s, s, p, p, 0.0)
            C.copy4d(dw, dwT.permute(3, 2, 0, 1))
        else:
            C.conv_nhwc_wgrad(g, xp, dwt, R, R, s, s, p, p, 0.0, bf16=bf16)

    out = {"fwd": fwd, "wgrad": wgrad}
    if Cin == Cp:  # the stem's input has no gradient
        out["dgrad"] = dgrad
    flops = 2.0 * N * P * Q * Cout * R * R * Cin
    return out, flops


def bench_layers():
    plan_db.ensure_loaded(C)  # the fp32 side runs its measured plans, as in training
    rows = []
    for name, *geom in LAYERS:
        fns, fl = passes(*geom)
        N, Cin, H, W, Cout, R, s, p = geom
        for pname in ("fwd", "dgrad", "wgrad"):
            if pname not in fns:
                continue
            fn = fns[pname]
            reps = 20
            t16, t32 = [], []
            for _ in range(REPEATS):  # interleaved: drift hits both alike
                t32.append(timeit(lambda: fn(False), reps))
                t16.append(timeit(lambda: fn(True), reps))
            m16, m32 = statistics.median(t16), statistics.median(t32)
            spread32 = max(t32) - min(t32)
            mode = {"fwd": 0, "dgrad": 1, "wgrad": 2}[pname]
            Cp = (Cin + 3) // 4 * 4
            row = {"layer": name, "pass": pname, "geom": geom,
                   "plan": C.conv_bf16_plan(mode, [N, Cp, H, W], Cout, R, R, s, s, p, p)
                   if not (pname == "dgrad" and s != 1) else "phases",
                   "bf16_us": round(m16, 1), "f32_us": round(m32, 1),
                   "f32_spread_us": round(spread32, 1),
                   "bf16_spread_us": round(max(t16) - min(t16), 1),
                   "speedup": round(m32 / m16, 2), "bf16_tflops": round(fl / m16 / 1e6, 1),
                   "faster_beyond_spread": bool(m32 - m16 > spread32)}
            rows.append(row)
            print(json.dumps(row), flush=True)
    return rows


def bench_step():
    from tutorial_torch_distributed_data_parallel_amd.models.registry import build_model

    x = torch.randn(128, 3, 224, 224, device=dev)
    y = torch.randint(0, 10, (128,), device=dev)

    def runner(amp, fp32_conv):
        torch.manual_seed(0)
        m = build_model("alexnet").to(dev).train()
        opt = tdp.optim.SGD(m.parameters(), lr=0.01, momentum=0.9)

        def step():
            convmod.AUTOCAST_FP32_CONV = fp32_conv
            try:
                opt.zero_grad()
                with tdp.autocast(enabled=amp):
                    loss = tdp.ops.cross_entropy(m(x), y)
                loss.backward()
                opt.step()
            finally:
                convmod.AUTOCAST_FP32_CONV = False

        return step

    modes = {"f32": runner(False, False), "autocast": runner(True, False),
             "autocast_fp32_conv": runner(True, True)}
    for s in modes.values():
        for _ in range(5):
            s()
    times = {k: [] for k in modes}
    for _ in range(REPEATS):
        for k, s in modes.items():
            times[k].append(timeit(s, 10))
    row = {"step": "alexnet_b128_sgd_eager"}
    for k, t in times.items():
        row[k + "_us"] = round(statistics.median(t), 1)
        row[k + "_spread_us"] = round(max(t) - min(t), 1)
    row["speedup_autocast"] = round(row["f32_us"] / row["autocast_us"], 2)
    row["speedup_linear_only"] = round(row["f32_us"] / row["autocast_fp32_conv_us"], 2)
    print(json.dumps(row), flush=True)
    return row


def to_md(rows, step):
    out = ["| layer | pass | splits | conv_bf16 us | fp32 us | fp32 spread us | speedup | "
           "bf16 TFLOP/s | beyond spread |", "|---|---|---|---|---|---|---|---|---|"]
    for r in rows:
        sp = r["plan"] if isinstance(r["plan"], str) else r["plan"][0]
        out.append(f"| {r['layer']} | {r['pass']} | {sp} | {r['bf16_us']} | {r['f32_us']} | "
                   f"{r['f32_spread_us']} | {r['speedup']} | {r['bf16_tflops']} | "
                   f"{'yes' if r['faster_beyond_spread'] else 'NO'} |")
    if step:
        out += ["", "| AlexNet SGD step (eager, batch 128) | median us | spread us |", "|---|---|---|"]
        for k in ("f32", "autocast", "autocast_fp32_conv"):
            out.append(f"| {k} | {step[k + '_us']} | {step[k + '_spread_us']} |")
    return "\n".join(out) + "\n"


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--step", action="store_true")
    ap.add_argument("--md", default=None)
    a = ap.parse_args()
    warm()
    rows = bench_layers()
    step = bench_step() if a.step else None
    if a.md:
        with open(a.md, "w") as f:
            f.write(to_md(rows, step))
