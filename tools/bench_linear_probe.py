#!/usr/bin/env python3
"""Time lafs_softmax_ce_rank (csrc/linear_probe.hip) against its byte count, and the linear probe's training step, on one device.

usage: tools/bench_linear_probe.py [--rows 1024] [--classes 205990] [--features 1536] [--calls 200] [--steps 50] [--reps 3]
                                   [--out profiles/linear_probe.txt]

Kernel: `calls` back-to-back calls between two device events, best of `reps` after a warm-up, for the evaluation form (no gradient:
4 B C bytes) and the training form (8 B C + 2 B lddl bytes: the gradient pass reads the logits a second time); bytes / time against
the measured HBM copy rate of MI355X_MICROARCH.md (6.29 TB/s).  Next to it torch's cross_entropy forward + autograd backward on the
same logits (fp32 gradient, no rank).  Probe: `steps` LinearProbe.step calls (gather, cast, logits GEMM, loss, weight-gradient GEMM,
SGD) between two events, steps per second, at `classes` and at 10 000 classes."""
import argparse
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from lafs_cvpr2024_amd import ops  # noqa: E402
from lafs_cvpr2024_amd.linear_probe import LinearProbe  # noqa: E402

HBM_COPY = 6.29e12


def timed(fn, n, reps):
    fn()                                                   # warm-up: code objects, allocator
    torch.cuda.synchronize()
    best = float("inf")
    for _ in range(reps):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        for _ in range(n):
            fn()
        b.record()
        torch.cuda.synchronize()
        best = min(best, a.elapsed_time(b) / 1e3 / n)
    return best


def main():
    p = argparse.ArgumentParser()
    p.add_argument("--rows", default=1024, type=int)
    p.add_argument("--classes", default=205990, type=int)
    p.add_argument("--features", default=1536, type=int)
    p.add_argument("--calls", default=200, type=int)
    p.add_argument("--steps", default=50, type=int)
    p.add_argument("--reps", default=3, type=int)
    p.add_argument("--out", default="", type=str)
    a = p.parse_args()
    dev = torch.device("cuda", 0)
    g = torch.Generator(device=dev).manual_seed(0)
    B, C = a.rows, a.classes
    ld = (C + 7) // 8 * 8
    lines = [f"lafs_softmax_ce_rank: B = {B}, C = {C}, ld = lddl = {ld}, {torch.cuda.get_device_name(0)}",
             f"times: {a.calls} calls between two device events, best of {a.reps} after one warm-up"]
    logits = torch.randn(B, ld, device=dev, generator=g) * 3
    y = torch.randint(0, C, (B,), device=dev, generator=g, dtype=torch.int32)
    dl = torch.empty(B, ld, device=dev, dtype=torch.bfloat16)
    loss, rank = torch.empty(B, device=dev), torch.empty(B, device=dev, dtype=torch.int32)
    ws = ops.softmax_ce_rank_workspace(B, C, dev)
    t_eval = timed(lambda: ops.softmax_ce_rank(logits, y, C, 1.0, None, loss, rank, ws), a.calls, a.reps)
    t_train = timed(lambda: ops.softmax_ce_rank(logits, y, C, 1.0 / B, dl, loss, rank, ws), a.calls, a.reps)
    b_eval, b_train = 4.0 * B * C, 8.0 * B * C + 2.0 * B * ld
    yl = y.long()

    def torch_ce():
        z = logits[:, :C].detach().requires_grad_(True)
        torch.nn.functional.cross_entropy(z, yl).backward()
        return z.grad
    t_torch = timed(torch_ce, a.calls, a.reps)
    lines += [f"  no gradient   {t_eval * 1e6:9.1f} us   {b_eval / 1e6:8.1f} MB   {b_eval / t_eval / 1e12:5.2f} TB/s = {100 * b_eval / t_eval / HBM_COPY:5.1f} % of the 6.29 TB/s copy rate",
              f"  with gradient {t_train * 1e6:9.1f} us   {b_train / 1e6:8.1f} MB   {b_train / t_train / 1e12:5.2f} TB/s = {100 * b_train / t_train / HBM_COPY:5.1f} % of the 6.29 TB/s copy rate",
              f"  gradient pass alone (difference) {(t_train - t_eval) * 1e6:9.1f} us for {(b_train - b_eval) / 1e6:8.1f} MB: {(b_train - b_eval) / (t_train - t_eval) / 1e12:5.2f} TB/s",
              f"  torch cross_entropy fwd + bwd (fp32 gradient, no rank) {t_torch * 1e6:9.1f} us: {t_torch / t_train:5.2f} x the call with gradient"]
    del logits, dl
    torch.cuda.empty_cache()
    F = a.features
    for n_class in (C, 10000):
        probe = LinearProbe(F, n_class, dev, seed=0)
        probe.set_lr(0.1)
        N = 4 * B
        cached = probe.cache(torch.randn(N, F, device=dev, generator=g), torch.randint(0, n_class, (N,), device=dev, generator=g))
        idx = torch.randperm(N, device=dev, generator=g)[:B]
        t_step = timed(lambda: probe.step(cached, idx, B), a.steps, a.reps)
        flops = 2 * 2.0 * B * probe.Cp * probe.Fp
        lines.append(f"LinearProbe.step: B = {B}, F = {F}, C = {n_class}: {t_step * 1e3:8.3f} ms = {1 / t_step:8.1f} steps/s "
                     f"({flops / t_step / 1e12:6.1f} TFLOP/s over the two GEMMs' 4 B C F; arena {probe.arena.size * 14 / 1e9:.2f} GB)")
        del probe, cached
        torch.cuda.empty_cache()
    text = "\n".join(lines) + "\n"
    print(text, end="")
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(text)


if __name__ == "__main__":
    main()
