#!/usr/bin/env python3
"""Timing of the DINO-face views (lafs_dino_views) on the GPU box, one process for both sides of each comparison:

  kernels  lafs_dino_views (2 global + 8 local views per image) against lafs_augment_views (the 20 views of DataAugmentation_LAFS)
           at B = 64, n_local = 8, the same images and sampled records of each loader; device events around `--reps` back-to-back
           calls, the two sides alternating for `--rounds` rounds;
  step     the --arch fvit pre-training step (default dims) fed by --data synthetic_u8 --views dino (views built on the side
           stream underneath the step) against --data synthetic (random crops made on the compute stream), alternating
           `--rounds` epochs of `--steps` steps on ONE engine; device events around each epoch.

usage: python tools/bench_dino_views.py [kernels] [step] [--reps N] [--rounds N] [--steps N] [--batch B]   (default: both)
Prints one JSON line per part: median and (min, max) over the rounds, so that the spread stands next to the difference."""
import argparse
import json
import os
import statistics
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
import torch

from lafs_cvpr2024_amd import augment as aug
from lafs_cvpr2024_amd.ops import _p, call


def timed(fn, reps):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda.synchronize(); e0.record()
    for _ in range(reps):
        fn()
    e1.record(); torch.cuda.synchronize()
    return e0.elapsed_time(e1) / reps * 1e-3


def summary(ts):
    return {"median_us": round(statistics.median(ts) * 1e6, 1), "min_us": round(min(ts) * 1e6, 1), "max_us": round(max(ts) * 1e6, 1)}


def bench_kernels(o):
    B, nl = o.batch, 8
    u8 = torch.randint(0, 256, (B, 3, 112, 112), device="cuda", dtype=torch.uint8)
    dino = aug.DeviceDinoAugmenter(B, n_local=nl, device="cuda", seed=0)
    lafs = aug.DeviceAugmenter(B, n_local=nl, device="cuda", seed=0)
    rng = np.random.RandomState(0)
    dino.params_dev.copy_(torch.from_numpy(aug.sample_dino_packed(rng, B, nl)))
    lafs.params_dev.copy_(torch.from_numpy(aug.sample_packed(rng, B, nl)))
    f_dino = lambda: call("lafs_dino_views", _p(u8), _p(dino.params_dev), _p(dino.table_g), _p(dino.table_l), dino.table_l.shape[-1],
                          B, nl, dino.mean_std, _p(dino.stage_g), _p(dino.stage_l))
    rec_g = dino.params_dev[:, :2].contiguous()
    f_dino_g = lambda: call("lafs_dino_views", _p(u8), _p(rec_g), _p(dino.table_g), None, 0, B, 0, dino.mean_std, _p(dino.stage_g), None)
    f_lafs = lambda: call("lafs_augment_views", _p(u8), _p(lafs.params_dev), _p(lafs.table), B, 2 + nl, _p(lafs.views))
    sides = {"lafs_dino_views": f_dino, "lafs_dino_views_globals_only": f_dino_g, "lafs_augment_views": f_lafs}
    for f in sides.values():                                  # warm-up: code objects, LDS attribute
        timed(f, 5)
    ts = {k: [] for k in sides}
    for _ in range(o.rounds):
        for k, f in sides.items():
            ts[k].append(timed(f, o.reps))
    out_bytes = {"lafs_dino_views": (2 * 112 * 112 + nl * 48 * 48) * 3 * 4 * B, "lafs_dino_views_globals_only": 2 * 112 * 112 * 3 * 4 * B,
                 "lafs_augment_views": 2 * (2 + nl) * 112 * 112 * 3 * 4 * B}
    res = {k: dict(summary(v), written_MB=round(out_bytes[k] / 1e6, 2)) for k, v in ts.items()}
    print(json.dumps({"part": "kernels", "B": B, "n_local": nl, "reps": o.reps, "rounds": o.rounds, **res}))


def bench_step(o):
    from lafs_cvpr2024_amd import lafs_train as L
    from lafs_cvpr2024_amd import utils
    from lafs_cvpr2024_amd.dino_loss import DINOLoss
    from lafs_cvpr2024_amd.engine import LafsPretrainEngine
    from lafs_cvpr2024_amd.vision_transformer import DINOHead
    args = L.get_args_parser().parse_args(f"--arch fvit --batch_size_per_gpu {o.batch} --views dino --data synthetic_u8".split())
    dev = torch.device("cuda", 0)
    torch.manual_seed(0)
    sb, tb, dim = L.build_backbones(args)
    student = utils.MultiCropWrapper(sb, DINOHead(dim, args.out_dim, use_bn=args.use_bn_in_head, norm_last_layer=args.norm_last_layer))
    teacher = utils.MultiCropWrapper(tb, DINOHead(dim, args.out_dim, args.use_bn_in_head))
    teacher.load_state_dict(student.state_dict())
    nl = args.local_crops_number
    engine = LafsPretrainEngine(student, teacher, DINOLoss(args.out_dim, nl + 2, 0.07, 0.04, 30, 41), o.batch, n_local=nl, device=dev)
    views = L.build_dino_views(args, dev)
    hp = dict(lr=1e-5, wd=0.04, momentum=0.996, teacher_temp=0.04, epoch=1)

    def epoch(kind, steps):
        if kind == "dino":
            src = L._Pipelined(L.SyntheticU8Views(steps, o.batch, nl, dev, 0, augment=False), views, engine)
        else:
            src = L.SyntheticCrops(steps, o.batch, nl, dev, 0)
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        torch.cuda.synchronize(); e0.record()
        for images, after in src:
            engine.step(images, **hp)
            if callable(after):
                after()
        e1.record(); torch.cuda.synchronize()
        return e0.elapsed_time(e1) / steps * 1e-3

    for kind in ("synthetic", "dino"):                        # warm-up: graph capture, allocator, both sources
        epoch(kind, 6)
    ts = {"synthetic": [], "dino": []}
    for _ in range(o.rounds):
        for kind in ts:
            ts[kind].append(epoch(kind, o.steps))
    res = {"step_" + k: summary(v) for k, v in ts.items()}
    print(json.dumps({"part": "step", "arch": "fvit", "dims": args.fvit_dims, "B": o.batch, "n_local": nl, "steps": o.steps,
                      "rounds": o.rounds, **res}))


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("parts", nargs="*", default=["kernels", "step"])
    ap.add_argument("--reps", type=int, default=200)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--batch", type=int, default=64)
    o = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("bench_dino_views.py measures on the GPU: no device found")
    if "kernels" in o.parts:
        bench_kernels(o)
    if "step" in o.parts:
        bench_step(o)
