#!/usr/bin/env python3
"""Time lafs_margin_softmax_ce_mix_bf16 (lambda per row, label smoothing) and lafs_margin_softmax_ce_ada_bf16 (AdaFace: a margin pair
per row, clamped cosines) against lafs_margin_softmax_ce_bf16 at the fine-tune
head's shape (B = 128, C = 205 990): all stream the fp32 logits twice and write the bf16 gradient once.  Interleaved rounds in one
process; per variant the median over rounds of the mean launch time, and the existing kernel's own round-to-round spread.  GPU box only.
usage: python tools/bench_mix_loss.py [--batch 128] [--classes 205990] [--rounds 9] [--iters 40]"""
import argparse
import json
import os
import statistics
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch

from lafs_cvpr2024_amd.ops import _p, call

ap = argparse.ArgumentParser()
ap.add_argument("--batch", type=int, default=128)
ap.add_argument("--classes", type=int, default=205990)
ap.add_argument("--rounds", type=int, default=9)
ap.add_argument("--iters", type=int, default=40)
a = ap.parse_args()
dev = torch.device("cuda", 0)
B, C = a.batch, a.classes
Cpad = (C + 127) // 128 * 128
torch.manual_seed(0)
cos = torch.rand(B, Cpad, device=dev) * 2 - 1
y1 = torch.randint(0, C, (B,), device=dev, dtype=torch.int32)
lam = torch.rand(B, device=dev)
lam1 = torch.full((1,), 0.3, device=dev)
dcos = torch.empty(B, Cpad, device=dev, dtype=torch.bfloat16)
loss, rows, part = torch.zeros(1, device=dev), torch.empty(B, device=dev), torch.empty(B * 48, device=dev)


def old():
    call("lafs_margin_softmax_ce_bf16", _p(cos), Cpad, B, C, _p(y1), None, 1.0, _p(lam1), 64.0, 0.4, 0, 1.0, _p(dcos), Cpad, _p(loss), _p(rows), _p(part))


def new(eps):
    return lambda: call("lafs_margin_softmax_ce_mix_bf16", _p(cos), Cpad, B, C, _p(y1), None, _p(lam), 1, eps, 64.0, 0.4, 0, 1.0, _p(dcos),
                        Cpad, _p(loss), _p(rows), _p(part))


# AdaFace: margins of rows whose quality proxy k runs over [-1, 1] (g_ang = -m k, g_add = m + m k), the batch's lambda at stride 0
k = torch.linspace(-1.0, 1.0, B, device=dev)
row_margin = torch.stack([-0.4 * k, 0.4 + 0.4 * k], 1).contiguous()


def ada():
    call("lafs_margin_softmax_ce_ada_bf16", _p(cos), Cpad, B, C, _p(y1), None, _p(lam1), 0, _p(row_margin), 64.0, 1.0, _p(dcos), Cpad, _p(loss),
         _p(rows), _p(part))


variants = {"margin_softmax_ce_bf16": old, "mix_bf16 eps=0": new(0.0), "mix_bf16 eps=0.1": new(0.1), "ada_bf16": ada}
times = {k: [] for k in variants}
for f in variants.values():
    for _ in range(10):
        f()
torch.cuda.synchronize()
for _ in range(a.rounds):
    for k, f in variants.items():
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(a.iters):
            f()
        e1.record()
        e1.synchronize()
        times[k].append(e0.elapsed_time(e1) * 1e3 / a.iters)
out = {"shape": f"B={B} C={C}", "rounds": a.rounds, "iters_per_round": a.iters, "bytes_streamed_MB": round((2 * B * Cpad * 4 + B * Cpad * 2) / 1e6, 1)}
for k, t in times.items():
    out[k] = {"median_us": round(statistics.median(t), 2), "min_us": round(min(t), 2), "max_us": round(max(t), 2)}
ref = times["margin_softmax_ce_bf16"]
out["existing_kernel_spread_us"] = round(max(ref) - min(ref), 2)
print(json.dumps(out))
