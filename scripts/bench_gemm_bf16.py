"""Mixed-precision GEMM (csrc/gemm_bf16.hip: operands rounded once to bf16, one MFMA product per
K16 step) next to the fp32 GEMM (gemm_f32: split-bf16, six products) on the toy-MLP / AlexNet
classifier Linears at batch 128 (forward, input gradient, weight gradient) and 4096^3, interleaved
in one process: event timing, warm-up, REPEATS timed runs of each per shape. One JSON line per
shape with the median of each, the spread (max - min) of the fp32 runs, and whether the gap
exceeds that spread.

--step times a ToyMLP 9216-4096-4096-10 SGD step (world-1 DDP, fused optimizer, batch 128) with
and without tdp.autocast; the fp32 side uses TDP_OPT_EPILOGUE=0 so both sides run the bucket-path
optimizer; the default fp32 step (optimizer epilogues) is recorded for context.

python scripts/bench_gemm_bf16.py [--step] [--md OUT.md]"""
import argparse
import json
import os
import statistics
import sys

import torch

sys.path.insert(0, __file__.rsplit("/scripts/", 1)[0])
import tutorial_torch_distributed_data_parallel_amd as tdp  # noqa: E402
from tutorial_torch_distributed_data_parallel_amd._native import native  # noqa: E402

C = native()
dev = "cuda"
REPEATS = 7
B = 128
# name, M, N, K, a_kcontig, b_kcontig, rowsum
SHAPES = []
for lname, fin, fout in (("fc1", 9216, 4096), ("fc2", 4096, 4096), ("fc3", 4096, 10)):
    SHAPES += [(f"{lname}_fwd", B, fout, fin, True, True, False),
               (f"{lname}_dgrad", B, fin, fout, True, False, False),
               (f"{lname}_wgrad", fout, fin, B, False, False, True)]
SHAPES.append(("sq4096", 4096, 4096, 4096, True, True, False))


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


def bench_shapes():
    rows = []
    for name, M, N, K, ak, bk, rs in SHAPES:
        torch.manual_seed(M + N + K)
        A = torch.randn((M, K) if ak else (K, M), device=dev)
        Bm = torch.randn((N, K) if bk else (K, N), device=dev)
        o16 = torch.empty(M, N, device=dev)
        o32 = torch.empty(M, N, device=dev)
        r16 = torch.empty(M, device=dev) if rs else None
        r32 = torch.empty(M, device=dev) if rs else None
        fl = 2.0 * M * N * K
        reps = 10 if fl > 1e11 else 50
        t16, t32 = [], []
        for _ in range(REPEATS):  # interleaved: drift hits both alike
            t32.append(timeit(lambda: C.gemm_f32(A, Bm, o32, ak, bk, rowsum=r32), reps))
            t16.append(timeit(lambda: C.gemm_bf16(A, Bm, o16, ak, bk, rowsum=r16), reps))
        m16, m32 = statistics.median(t16), statistics.median(t32)
        spread32 = max(t32) - min(t32)
        row = {"shape": name, "M": M, "N": N, "K": K, "layout": [ak, bk],
               "plan": C.gemm_bf16_plan(A, Bm, o16, ak, bk),
               "bf16_us": round(m16, 1), "f32_us": round(m32, 1),
               "f32_spread_us": round(spread32, 1), "bf16_spread_us": round(max(t16) - min(t16), 1),
               "speedup": round(m32 / m16, 2),
               "bf16_tflops": round(fl / m16 / 1e6, 1),
               # bytes both kernels must move at least once (fp32 operands + output)
               "min_gbs_bf16": round(4.0 * (M * K + N * K + M * N) / m16 / 1e3, 0),
               "faster_beyond_spread": bool(m32 - m16 > spread32)}
        rows.append(row)
        print(json.dumps(row), flush=True)
    return rows


def bench_step():
    from tutorial_torch_distributed_data_parallel_amd.models import ToyMLP

    if not tdp.parallel.is_initialized():
        tdp.init_process_group("nccl", rank=0, world_size=1, local_rank=0)
    x = torch.randn(B, 9216, device=dev)
    y = torch.randint(0, 10, (B,), device=dev)

    def runner(amp, epilogue):
        os.environ["TDP_OPT_EPILOGUE"] = "1" if epilogue else "0"
        torch.manual_seed(0)
        m = ToyMLP(device=dev)
        d = tdp.DDP(m, device_ids=[0], factor_sync=False)
        opt = tdp.optim.SGD(d.parameters(), lr=0.01, momentum=0.9)
        d.register_fused_optimizer(opt)

        def step():
            opt.zero_grad()
            with tdp.autocast(enabled=amp):
                loss = d(x, target=y)
            loss.backward()
            opt.step()

        return step

    modes = {"bf16_autocast": runner(True, False), "f32_bucket_opt": runner(False, False),
             "f32_default": runner(False, True)}
    os.environ.pop("TDP_OPT_EPILOGUE", None)
    for s in modes.values():
        for _ in range(5):
            s()
    times = {k: [] for k in modes}
    for _ in range(REPEATS):
        for k, s in modes.items():
            times[k].append(timeit(s, 20))
    row = {"step": "toy_mlp_9216_4096_4096_10_b128_eager"}
    for k, t in times.items():
        row[k + "_us"] = round(statistics.median(t), 1)
        row[k + "_spread_us"] = round(max(t) - min(t), 1)
    row["speedup_vs_bucket_opt"] = round(row["f32_bucket_opt_us"] / row["bf16_autocast_us"], 2)
    print(json.dumps(row), flush=True)
    tdp.destroy_process_group()
    return row


def to_md(rows, step):
    out = ["| shape | M | N | K | splits | gemm_bf16 us | gemm_f32 us | f32 spread us | speedup | "
           "beyond spread |", "|---|---|---|---|---|---|---|---|---|---|"]
    for r in rows:
        out.append(f"| {r['shape']} | {r['M']} | {r['N']} | {r['K']} | {r['plan'][0]} | "
                   f"{r['bf16_us']} | {r['f32_us']} | {r['f32_spread_us']} | {r['speedup']} | "
                   f"{'yes' if r['faster_beyond_spread'] else 'NO'} |")
    if step:
        out += ["", "| step (eager, batch 128) | median us | spread us |", "|---|---|---|"]
        for k in ("bf16_autocast", "f32_bucket_opt", "f32_default"):
            out.append(f"| {k} | {step[k + '_us']} | {step[k + '_spread_us']} |")
    return "\n".join(out) + "\n"


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--step", action="store_true")
    ap.add_argument("--md", default=None)
    a = ap.parse_args()
    warm()
    rows = bench_shapes()
    step = bench_step() if a.step else None
    if a.md:
        with open(a.md, "w") as f:
            f.write(to_md(rows, step))
