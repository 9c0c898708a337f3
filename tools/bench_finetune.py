#!/usr/bin/env python3
"""Fine-tune step benchmark (BASELINE.json configs C4/C5 on ONE GPU): Part-fViT ViT-B (dim 768, depth 12, heads 11, mlp 2048)
+ margin head, batch 128, uint8 112x112 synthetic faces resident in HBM.  GPU box only.
usage: python tools/bench_finetune.py [--head CosFace|ArcFace|PartialFC] [--with-land 0|1] [--dropout 0.1] [--classes N] [--batch B]
                                      [--mixup A] [--mixup-prob P] [--cutmix A] [--mixup-mode batch|pair|elem] [--smoothing E]
                                      [--pre-land 0|1] [--keep-land 0|1] [--land-weight W]"""
import argparse
import json
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch

from lafs_cvpr2024_amd.face_pre_pro.ViT_face import ViT_face_landmark_patch8
from lafs_cvpr2024_amd.finetune_engine import FinetuneEngine

ap = argparse.ArgumentParser()
ap.add_argument("--head", default="CosFace")
ap.add_argument("--with-land", type=int, default=1)
ap.add_argument("--dropout", type=float, default=0.1)
ap.add_argument("--classes", type=int, default=205990)
ap.add_argument("--batch", type=int, default=128)
ap.add_argument("--sample-rate", type=float, default=0.1)
ap.add_argument("--steps", type=int, default=12)
ap.add_argument("--warmup", type=int, default=3)
ap.add_argument("--miopen-find", type=int, default=0, help="torch.backends.cudnn.benchmark (MIOpen exhaustive find) for the CNN branch")
ap.add_argument("--channels-last", type=int, default=0)
ap.add_argument("--mixup", type=float, default=0.2)
ap.add_argument("--mixup-prob", type=float, default=0.1)
ap.add_argument("--cutmix", type=float, default=0.0)
ap.add_argument("--mixup-mode", default="batch")
ap.add_argument("--smoothing", type=float, default=0.0)
ap.add_argument("--pre-land", type=int, default=0, help="frozen stage-1 landmark CNN (train_largescale.py --pre_land); alone it needs --with-land 0")
ap.add_argument("--keep-land", type=int, default=0, help="landmark supervision of the backbone's own branch (--keep_land)")
ap.add_argument("--land-weight", type=float, default=1000.0)
a = ap.parse_args()
torch.backends.cudnn.benchmark = bool(a.miopen_find)
dev = torch.device("cuda", 0)
torch.manual_seed(0)
sharded = a.head == "PartialFC"
m = ViT_face_landmark_patch8(loss_type="None" if sharded else "CosFace", GPU_ID=None, num_class=a.classes, image_size=112, patch_size=8,
                             dim=768, depth=12, heads=11, mlp_dim=2048, dropout=a.dropout, emb_dropout=a.dropout,
                             with_land=bool(a.with_land), drop_path_rate=0.1)
head = None
if sharded:
    from lafs_cvpr2024_amd.partial_fc import PartialFC
    head = PartialFC(768, a.classes, a.batch, sample_rate=a.sample_rate, device=dev)
teacher = None
if a.pre_land:
    from lafs_cvpr2024_amd.face_pre_pro.ViT_face import face_landmark_4simmin_glo_loc
    teacher = face_landmark_4simmin_glo_loc(loss_type="CosFace", GPU_ID=None, num_class=30000, num_patches=196, image_size=112, patch_size=8,
                                            dim=512, depth=12, heads=11, mlp_dim=2560, dropout=0.1, emb_dropout=0.1).eval()
eng = FinetuneEngine(m, a.batch, acc_step=1, margin_type=1 if a.head == "ArcFace" else 0, m=0.5 if a.head == "ArcFace" else 0.4,
                     device=dev, sharded_head=head, mixup_alpha=a.mixup, mixup_prob=a.mixup_prob, cutmix_alpha=a.cutmix, mix_mode=a.mixup_mode,
                     label_smoothing=a.smoothing, landmark_teacher=teacher, keep_land=bool(a.keep_land))
land = dict(land_weight=a.land_weight) if a.keep_land else {}
m.train()
if a.channels_last and a.with_land:
    m.stn.to(memory_format=torch.channels_last)
x = torch.randint(0, 256, (a.batch, 3, 112, 112), dtype=torch.uint8, device=dev)
y = torch.randint(0, a.classes, (a.batch,), device=dev)
trace = []
for _ in range(a.warmup):
    trace.append(round(float(eng.step(x, y, lr=1e-4, **land).item()), 3))
torch.cuda.synchronize(); t0 = time.perf_counter()
for _ in range(a.steps):
    loss = eng.step(x, y, lr=1e-4, **land)
torch.cuda.synchronize(); dt = (time.perf_counter() - t0) / a.steps
print(json.dumps({"workload": f"Part-fViT ViT-B + {a.head} fine-tune step, batch {a.batch}, {a.classes} classes, with_land={a.with_land}, "
                              f"dropout={a.dropout}" + (f", pre_land={a.pre_land} keep_land={a.keep_land}" if a.pre_land else "") + (f", sample_rate={a.sample_rate}" if sharded else "") +
                              (f", cutmix={a.cutmix} mode={a.mixup_mode} smoothing={a.smoothing} mixup_prob={a.mixup_prob}" if eng.mix_rows else ""),
                  "ms_per_step": round(dt * 1e3, 2), "images_per_s": round(a.batch / dt, 1), "loss": round(float(loss.item()), 4), "warmup_losses": trace}))
