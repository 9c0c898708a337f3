#!/usr/bin/env python3
"""Time the k-NN search + vote (csrc/knn.hip) at the evaluation's shape, next to the torch.mm + torch.topk loop over query blocks
that DINO's eval_knn.py runs, on the same device and the same rows.

usage: tools/bench_knn.py [--queries 50000] [--bank 500000] [--dims 384,768] [--k 200] [--classes 100000] [--block 500] [--reps 2]
                          [--out profiles/knn_search.txt]

Per D one block of lines: device-event times of lafs_knn_search (whole call: scores, selection, merge) and lafs_knn_vote, the torch
loop's time, 2 Q N D / time of the search call against the fp32 MFMA peak (157.3 TFLOP/s; a whole-call rate, selection included, not
the GEMM part alone), and how many of the first block's top-1 neighbours the two agree on."""
import argparse
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from lafs_cvpr2024_amd import knn  # noqa: E402

PEAK_F32_MFMA = 157.3e12


def timed(fn, reps):
    fn()                                                   # warm-up: code objects, allocator
    torch.cuda.synchronize()
    best = float("inf")
    for _ in range(reps):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        out = fn()
        b.record()
        torch.cuda.synchronize()
        best = min(best, a.elapsed_time(b) / 1e3)
    return best, out


def torch_loop(bank, query, k, block):
    """DINO's loop: per block of queries one mm against the whole bank and one topk."""
    bt = bank.t()
    top_s, top_i = [], []
    for q0 in range(0, query.shape[0], block):
        s, i = torch.mm(query[q0:q0 + block], bt).topk(k, largest=True, sorted=True)
        top_s.append(s); top_i.append(i)
    return torch.cat(top_s), torch.cat(top_i)


def main():
    p = argparse.ArgumentParser()
    p.add_argument("--queries", default=50000, type=int)
    p.add_argument("--bank", default=500000, type=int)
    p.add_argument("--dims", default="384,768", type=str)
    p.add_argument("--k", default=200, type=int)
    p.add_argument("--classes", default=100000, type=int)
    p.add_argument("--block", default=500, type=int, help="queries per torch.mm (DINO: the test set in 100 chunks)")
    p.add_argument("--reps", default=2, type=int)
    p.add_argument("--out", default="", type=str)
    a = p.parse_args()
    dev = torch.device("cuda", 0)
    g = torch.Generator(device=dev).manual_seed(0)
    lines = [f"k-NN search + vote: {a.queries} queries x {a.bank} bank rows, k = {a.k}, {a.classes} classes, {torch.cuda.get_device_name(0)}",
             f"times: best of {a.reps} after one warm-up, device events; torch loop: mm + topk per {a.block} queries"]
    labels = torch.randint(0, a.classes, (a.bank,), device=dev, generator=g, dtype=torch.int32)
    ks = [v for v in knn.DEFAULT_KS if v <= a.k]
    for D in (int(v) for v in a.dims.split(",")):
        bank = knn.l2_normalize(torch.randn(a.bank, D, device=dev, generator=g))
        query = knn.l2_normalize(torch.randn(a.queries, D, device=dev, generator=g))
        t_search, (ts, ti) = timed(lambda: knn.knn_search(bank, query, a.k), a.reps)
        t_vote, _ = timed(lambda: knn.knn_vote(ts, ti, labels, ks, 0.07), a.reps)
        t_torch, (rs, ri) = timed(lambda: torch_loop(bank, query, a.k, a.block), a.reps)
        n = min(a.block, a.queries)
        agree = int((ti[:n, 0].long() == ri[:n, 0]).sum())
        flops = 2.0 * a.queries * a.bank * D
        lines += [f"D = {D}:",
                  f"  lafs_knn_search     {t_search * 1e3:10.1f} ms   {flops / t_search / 1e12:7.1f} TFLOP/s whole call = "
                  f"{100.0 * flops / t_search / PEAK_F32_MFMA:5.1f} % of the fp32 MFMA peak",
                  f"  lafs_knn_vote       {t_vote * 1e3:10.1f} ms   (ks = {ks})",
                  f"  torch mm + topk     {t_torch * 1e3:10.1f} ms   {flops / t_torch / 1e12:7.1f} TFLOP/s whole loop",
                  f"  search / torch      {t_search / t_torch:10.2f} x   (above 1: the kernel is slower)",
                  f"  top-1 neighbour agrees with torch for {agree} of the first {n} queries"]
        del bank, query, ts, ti, rs, ri
        torch.cuda.empty_cache()
    text = "\n".join(lines) + "\n"
    print(text, end="")
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(text)


if __name__ == "__main__":
    main()
