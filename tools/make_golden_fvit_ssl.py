#!/usr/bin/env python
"""Golden vectors of LAFS pre-training on an fViT pair -> tests/golden/f27_lafs_step_fvit.npz (+ f27_lafs_step_fvit_<i>.npz).

Runs where the read-only reference checkout is mounted (LAFS_REFERENCE, as for tools/make_golden.py) and imports the reference's own
modules on the CPU in fp32 through tools/make_golden.py's import recipe; only numeric arrays are stored, none of the reference's text.

  model      MultiCropWrapper(ViTs_face_overlap(12 / 8 / 4 on 112 px, dim 64, depth 2, heads 2, mlp 128, no dropout), DINOHead(64, 256,
             hidden 64, bottleneck 32)) for student and teacher (head and K as F16), DropPath 0, pos_embedding and cls_token x 0.05,
             BatchNorm weight 1 + 0.1 n, bias 0.1 n (as F26).  NEITHER network is put in eval mode (reference lafs_train.py: no .eval()
             but :269): both BatchNorm heads normalise with batch statistics and update their running buffers.
  steps      two full steps of lafs_train.py:577-613: teacher on the 2 global crops, student on 2 global + 2 local crops, DINOLoss,
             backward, per-tensor clip at 3.0, last layer cancelled in step 0, AdamW, EMA of the parameters (buffers are not EMA'd,
             :610-613), center.  B = 4: every BatchNorm group has 8 rows (with very few rows rstd amplifies the trunk's bf16 noise).
  crops      crop0 .. crop3, rounded to fp16 BEFORE the reference sees them (the stored values are the exact inputs), shared by both steps
  s<k>.*     loss, s_out / t_out (all 256 logit columns), center, norms (pre-clip, in norm_names order), grad_post.* (post-clip),
             student.* / teacher.* (state dicts behind the step, BatchNorm buffers included)

    python tools/make_golden_fvit_ssl.py
"""
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from make_golden import _import_reference, save  # noqa: E402

CFG = dict(loss_type="None", GPU_ID=None, num_class=10, image_size=112, patch_size=8, ac_patch_size=12, pad=4, dim=64, depth=2, heads=2,
           mlp_dim=128, dropout=0, emb_dropout=0)
K, B, NCROPS = 256, 4, 4
PART_BYTES = 900 * 1024


def main():
    import torch.distributed as dist
    os.environ.setdefault("MASTER_ADDR", "127.0.0.1"); os.environ.setdefault("MASTER_PORT", "29547")
    dist.init_process_group("gloo", rank=0, world_size=1)            # DINOLoss.update_center all-reduces
    ref_utils, ref_vit, ref_lafs, ref_face, _ = _import_reference()
    torch.set_num_threads(4)
    torch.manual_seed(27)

    def mk():
        m = ref_face.ViTs_face_overlap(**CFG)
        for q in m.modules():                           # Residual_droppath hard-codes rate 0.1 -> parity mode = 0
            if isinstance(q, ref_vit.DropPath):
                q.drop_prob = 0.0
        return m
    student = ref_utils.MultiCropWrapper(mk(), ref_vit.DINOHead(64, K, hidden_dim=64, bottleneck_dim=32, norm_last_layer=True))
    teacher = ref_utils.MultiCropWrapper(mk(), ref_vit.DINOHead(64, K, hidden_dim=64, bottleneck_dim=32))
    with torch.no_grad():
        sb = student.backbone
        sb.pos_embedding.mul_(0.05); sb.cls_token.mul_(0.05)
        bn = sb.mlp_head[0]
        bn.weight.copy_(1 + 0.1 * torch.randn(64)); bn.bias.copy_(0.1 * torch.randn(64))
    teacher.load_state_dict(student.state_dict())
    for p in teacher.parameters():
        p.requires_grad = False
    assert student.training and teacher.training
    crit = ref_lafs.DINOLoss(K, NCROPS, 0.07, 0.04, 3, 10)
    opt = torch.optim.AdamW(ref_utils.get_params_groups(student))
    fx = {"init." + k: v.clone() for k, v in student.state_dict().items()}
    crops = [torch.randn(B, 3, s, s).clamp(-1, 1).half().float() for s in (112, 112, 48, 48)]
    fx.update({f"crop{i}": c.half() for i, c in enumerate(crops)})
    lrs, wds, moms = [5e-4, 4e-4], [0.04, 0.05], [0.9, 0.95]
    for step in range(2):
        epoch = step
        for i, g in enumerate(opt.param_groups):
            g["lr"] = lrs[step]
            if i == 0:
                g["weight_decay"] = wds[step]
        t_out = teacher(crops[:2]); s_out = student(crops)
        loss = crit(s_out, t_out, epoch)
        opt.zero_grad()
        loss.backward()
        norms = ref_utils.clip_gradients(student, 3.0)
        post = {n: p.grad.clone() for n, p in student.named_parameters() if p.grad is not None}
        ref_utils.cancel_gradients_last_layer(epoch, student, 1)
        opt.step()
        with torch.no_grad():
            for pq, pk in zip(student.parameters(), teacher.parameters()):
                pk.data.mul_(moms[step]).add_((1 - moms[step]) * pq.detach().data)
        fx.update({f"s{step}.loss": loss, f"s{step}.center": crit.center, f"s{step}.t_out": t_out[:, :256], f"s{step}.s_out": s_out[:, :256],
                   f"s{step}.norms": np.array(norms)})
        fx.update({f"s{step}.grad_post.{n}": g for n, g in post.items()})
        fx.update({f"s{step}.student.{k}": v.clone() for k, v in student.state_dict().items()})
        fx.update({f"s{step}.teacher.{k}": v.clone() for k, v in teacher.state_dict().items()})
        assert int(student.backbone.mlp_head[0].num_batches_tracked) == 2 * (step + 1)
        assert int(teacher.backbone.mlp_head[0].num_batches_tracked) == step + 1
    fx["hyper"] = np.array([lrs, wds, moms])
    fx["norm_names"] = np.array([n for n, p in student.named_parameters() if p.requires_grad])
    fx["teacher_backbone_keys"] = np.array([k[len("backbone."):] for k in teacher.state_dict() if k.startswith("backbone.")])
    # no committed file may exceed 1 MiB and random floats do not compress: the arrays go, in key order, into as many parts as it takes
    parts, room = [{}], PART_BYTES
    for k in sorted(fx):
        a = fx[k].detach().numpy() if isinstance(fx[k], torch.Tensor) else np.asarray(fx[k])
        if a.nbytes > room and parts[-1]:
            parts.append({}); room = PART_BYTES
        parts[-1][k] = fx[k]; room -= a.nbytes
    for i, part in enumerate(parts):
        save("f27_lafs_step_fvit" + (f"_{i}" if i else ""), **part)
    dist.destroy_process_group()


if __name__ == "__main__":
    main()
