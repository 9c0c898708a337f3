"""Cost of the KoLeo regulariser in the LAFS step: ms per step of bench.py's workload (ViT-S/8, batch 64, 2 global + 8 local crops,
out_dim 100000, hipGraph) with koleo_weight 0.1 against the same build with the weight at 0.  Three engines live side by side -- weight
0, weight 0.1 and a second one with weight 0, whose distance from the first is what two equal engines differ by (buffer placement) --
and take turns in blocks of --steps steps, --rounds times, in rotating order, so that drift of the shared machine lands on all; every
block is timed by device events around it.  Prints the per-block times, the medians and their differences, and lafs_koleo_fwd_bwd
alone at the step's shape (2 x 64 x 384) as an event-timed loop.

    python tools/lab/t_koleo_cost.py [--steps 40] [--rounds 6] [--batch 64]"""
import argparse
import os
import statistics
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__)))))

import torch  # noqa: E402

from lafs_cvpr2024_amd import ops, vision_transformer as vits  # noqa: E402
from lafs_cvpr2024_amd.dino_loss import DINOLoss  # noqa: E402
from lafs_cvpr2024_amd.engine import LafsPretrainEngine  # noqa: E402
from lafs_cvpr2024_amd.utils import MultiCropWrapper  # noqa: E402


def build(weight, B, K, nl, device):
    torch.manual_seed(0)
    student = MultiCropWrapper(vits.vit_small(patch_size=8, drop_path_rate=0.1), vits.DINOHead(384, K, use_bn=False, norm_last_layer=True))
    teacher = MultiCropWrapper(vits.vit_small(patch_size=8), vits.DINOHead(384, K, use_bn=False))
    teacher.load_state_dict(student.state_dict())
    eng = LafsPretrainEngine(student, teacher, DINOLoss(K, 2 + nl, 0.07, 0.04, 30, 41), B, n_local=nl, clip_grad=3.0, freeze_last_layer=1,
                             use_graph=True, device=device, koleo_weight=weight)
    g = torch.Generator(device=device).manual_seed(0)
    eng.in_global_all.copy_(torch.randn(eng.in_global_all.shape, device=device, generator=g).clamp_(-1, 1))
    eng.in_local_all.copy_(torch.randn(eng.in_local_all.shape, device=device, generator=g).clamp_(-1, 1))
    return eng


def block(eng, steps):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(steps):
        eng.step(lr=2.5e-4, wd=0.04, momentum=0.996, teacher_temp=0.04, epoch=1)
    b.record()
    b.synchronize()
    return a.elapsed_time(b) / steps


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=40)
    ap.add_argument("--rounds", type=int, default=6)
    ap.add_argument("--batch", type=int, default=64)
    ap.add_argument("--out-dim", type=int, default=100000)
    ap.add_argument("--local-crops", type=int, default=8)
    args = ap.parse_args()
    dev = torch.device("cuda", 0)
    names = ("0 (first)", "0.1", "0 (second)")
    engines = {n: build(w, args.batch, args.out_dim, args.local_crops, dev) for n, w in zip(names, (0.0, 0.1, 0.0))}
    for eng in engines.values():                              # capture + warm-up
        block(eng, 10)
    times = {n: [] for n in names}
    for r in range(args.rounds):
        for k in range(3):
            n = names[(r + k) % 3]
            times[n].append(block(engines[n], args.steps))
    med = {n: statistics.median(t) for n, t in times.items()}
    for n, t in times.items():
        print(f"koleo_weight {n}: ms/step per block {[round(v, 4) for v in t]}  median {med[n]:.4f}  spread {max(t) - min(t):.4f}")
    print(f"two equal engines (weight 0) differ by {1e3 * (med[names[2]] - med[names[0]]):.1f} us per step")
    print(f"weight 0.1 against the mean of the two: {1e3 * (med[names[1]] - 0.5 * (med[names[0]] + med[names[2]])):.1f} us per step; "
          f"loss {float(engines[names[1]].loss):.5f}, koleo term {float(engines[names[1]].koleo_value):.5f}")
    # the kernel pair alone, back to back on one stream (launch-bound: what it costs where nothing hides it)
    B, D = args.batch, 384
    x = torch.randn(2 * B, D, device=dev)
    dx, loss = torch.zeros_like(x), torch.zeros(2, device=dev)
    nn, ws = torch.zeros(2 * B, device=dev, dtype=torch.int32), ops.koleo_workspace(2, B, D, dev)
    call = lambda: ops.koleo(x, 2, B, grad_scale=0.1, dx=dx, accumulate=True, loss=loss, nn=nn, ws=ws)
    for _ in range(20):
        call()
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(500):
        call()
    b.record()
    b.synchronize()
    print(f"lafs_koleo_fwd_bwd alone, 2 x {B} x {D}: {1e3 * a.elapsed_time(b) / 500:.1f} us per call (two launches, eager loop)")


if __name__ == "__main__":
    main()
