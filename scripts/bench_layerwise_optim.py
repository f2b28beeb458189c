#!/usr/bin/env python
"""Time the LAMB / LARS launches (csrc/optim_layerwise.hip) against adam_flat / sgd_flat and a
torch ``_foreach`` implementation of the same formulas, on arenas shaped like the toy MLP and
ResNet-50. Needs a GPU. All candidates run in one process on the same arena, warmed up and
alternated round-robin; a sample is ``--inner`` back-to-back calls between two device events.
Prints one JSON line per arena: median microseconds per call and achieved GB/s from the bytes the
algorithm needs (LAMB 24 + 16 B/elem, LARS 8 + 20, Adam 28, SGD+momentum 20; the finish launch
reads 8 B per chunk and is reported as time only).

    python scripts/bench_layerwise_optim.py [--rounds 20] [--inner 10] [--models toy_mlp resnet50]
"""
import argparse
import json
import os
import statistics
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import tutorial_torch_distributed_data_parallel_amd as tdp  # noqa: E402
from tutorial_torch_distributed_data_parallel_amd.models.registry import build_model  # noqa: E402
from tutorial_torch_distributed_data_parallel_amd.parallel.arena import ParamArena  # noqa: E402


def foreach_lamb(ps, gs, ms, vs, lr, b1, b2, eps, wd, t):
    torch._foreach_lerp_(ms, gs, 1 - b1)
    torch._foreach_mul_(vs, b2)
    torch._foreach_addcmul_(vs, gs, gs, 1 - b2)
    den = torch._foreach_sqrt(vs)
    torch._foreach_div_(den, (1 - b2 ** t) ** 0.5)
    torch._foreach_add_(den, eps)
    u = torch._foreach_div(ms, 1 - b1 ** t)
    torch._foreach_div_(u, den)
    torch._foreach_add_(u, ps, alpha=wd)
    np_, nu = torch._foreach_norm(ps), torch._foreach_norm(u)
    r = torch._foreach_div(np_, nu)  # (the zero-norm guard is left out: it only adds passes)
    torch._foreach_mul_(u, r)
    torch._foreach_add_(ps, u, alpha=-lr)


def foreach_lars(ps, gs, bs, lr, mom, wd, trust, eps):
    np_, ng = torch._foreach_norm(ps), torch._foreach_norm(gs)
    den = torch._foreach_mul(np_, wd)
    torch._foreach_add_(den, ng)
    torch._foreach_add_(den, eps)
    q = torch._foreach_mul(np_, trust)
    torch._foreach_div_(q, den)
    d = torch._foreach_add(gs, ps, alpha=wd)
    torch._foreach_mul_(d, q)
    torch._foreach_mul_(bs, mom)
    torch._foreach_add_(bs, d)
    torch._foreach_add_(ps, bs, alpha=-lr)


def bench(name, rounds, inner):
    C = tdp._native.native()
    shapes = [tuple(p.shape) for p in build_model(name, device="cpu").parameters()]
    torch.manual_seed(0)
    ps = [torch.nn.Parameter(torch.randn(*s, device="cuda") * 0.05) for s in reversed(shapes)]
    arena = ParamArena(ps)
    arena.grad.normal_(0, 1e-2)
    m, v, buf = arena.new_state(), arena.new_state(), arena.new_state()
    n = sum(arena.numels)
    sl = [slice(o, o + k) for o, k in zip(arena.offsets, arena.numels)]
    P, G = [arena.data[s] for s in sl], [arena.grad[s] for s in sl]
    M, V, B = [m[s] for s in sl], [v[s] for s in sl], [buf[s] for s in sl]
    skip = [len(s) <= 1 for s in reversed(shapes)]
    t_lamb = C.layerwise_table(P, G, M, V, skip)
    t_lars = C.layerwise_table(P, G, B, [], skip)
    ws = torch.zeros(3, len(P), device="cuda")
    lamb = lambda st: C.lamb_layerwise(t_lamb, ws, 1e-3, 0.9, 0.999, 1e-6, 0.01, False, 10,  # noqa: E731
                                       1.0, None, st)
    lars = lambda st: C.lars_layerwise(t_lars, ws, 1e-3, 0.9, 0.0, 1e-4, False, False, False,  # noqa: E731
                                       1e-3, 1e-8, 1.0, None, st)
    cands = {
        "lamb_stage1": (lambda: lamb(1), 24), "lamb_finish": (lambda: lamb(2), 0),
        "lamb_stage2": (lambda: lamb(4), 16), "lamb_step": (lambda: lamb(7), 40),
        "lars_stage1": (lambda: lars(1), 8), "lars_finish": (lambda: lars(2), 0),
        "lars_stage2": (lambda: lars(4), 20), "lars_step": (lambda: lars(7), 28),
        "adam_flat": (lambda: C.adam_flat(arena.data, arena.grad, m, v, None, 1e-3, 0.9, 0.999,
                                          1e-8, 0.0, False, False, False, 10), 28),
        "sgd_flat": (lambda: C.sgd_flat(arena.data, arena.grad, buf, 1e-3, 0.9, 0.0, 0.0, False,
                                        False, False), 20),
        "foreach_lamb": (lambda: foreach_lamb(P, G, M, V, 1e-3, 0.9, 0.999, 1e-6, 0.01, 10), 0),
        "foreach_lars": (lambda: foreach_lars(P, G, B, 1e-3, 0.9, 1e-4, 1e-3, 1e-8), 0),
    }
    for fn, _ in cands.values():  # warm-up: code objects, allocator
        for _ in range(3):
            fn()
    torch.cuda.synchronize()
    samples = {k: [] for k in cands}
    for _ in range(rounds):
        for k, (fn, _) in cands.items():
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record()
            for _ in range(inner):
                fn()
            b.record()
            b.synchronize()
            samples[k].append(a.elapsed_time(b) * 1e3 / inner)
    out = {"arena": name, "elements": n, "tensors": len(P), "chunks": t_lamb.nchunks,
           "runs": t_lamb.nruns, "rounds": rounds, "inner": inner, "us": {}, "GBps": {}}
    for k, (_, bpe) in cands.items():
        us = statistics.median(samples[k])
        out["us"][k] = round(us, 2)
        out["us"][k + "_min"] = round(min(samples[k]), 2)
        if bpe:
            out["GBps"][k] = round(bpe * n / us / 1e3, 1)
    print(json.dumps(out), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=20)
    ap.add_argument("--inner", type=int, default=10)
    ap.add_argument("--models", nargs="+", default=["toy_mlp", "resnet50"])
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_layerwise_optim needs a GPU")
    for name in a.models:
        bench(name, a.rounds, a.inner)


if __name__ == "__main__":
    main()
