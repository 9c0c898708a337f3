#!/usr/bin/env python
"""Golden vectors of fViT (reference face_pre_pro/ViT_face.py:1506-1613, ``ViTs_face_overlap``) -> tests/golden/f26_fvit.npz (+ f26_fvit_<i>.npz).

Runs where the read-only reference checkout is mounted (LAFS_REFERENCE, as for tools/make_golden.py) and imports the reference's own
modules on the CPU in fp32 through tools/make_golden.py's import recipe; only numeric arrays are stored, none of the reference's text.

  model      ViTs_face_overlap(12 / 8 / 4 on 112 px, dim 128, depth 2, heads 3, mlp 256, no dropout), DropPath 0 (as F7),
             pos_embedding and cls_token x 0.05 (as F20: the output then depends on the patches), BatchNorm weight 1 + 0.1 n, bias 0.1 n
  p.*        the state dict before any forward
  train      the list forward [x112_a, x112_b, x48_a, x48_b, x48_c] (2 images each: BatchNorm groups of 4 and 6 rows), x112_a with
             requires_grad; z, the gradients g.* and gx112_a of (z * w).sum(), the BatchNorm buffers behind it (bn.*)
  eval       for_fea=True on a fresh [3, 3, 112, 112] batch with those buffers (xe -> ze)
  pad 2      a second model (12 / 8 / 2: the windows reach into the bottom / right padding at 112 px) with the state dict behind the
             training forward, eval only (xe2 -> ze2)

    python tools/make_golden_fvit.py
"""
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from make_golden import _import_reference, grads, save, sd  # noqa: E402

CFG = dict(loss_type="None", GPU_ID=None, num_class=10, image_size=112, patch_size=8, ac_patch_size=12, dim=128, depth=2, heads=3,
           mlp_dim=256, dropout=0, emb_dropout=0)
PART_BYTES = 900 * 1024


def main():
    _, ref_vit, _, ref_face, _ = _import_reference()

    def make(pad):
        m = ref_face.ViTs_face_overlap(pad=pad, **CFG)
        for mod in m.modules():                         # Residual_droppath hard-codes rate 0.1 -> parity mode = 0
            if isinstance(mod, ref_vit.DropPath):
                mod.drop_prob = 0.0
        return m

    torch.manual_seed(26)
    m = make(4)
    with torch.no_grad():
        m.pos_embedding.mul_(0.05); m.cls_token.mul_(0.05)
        bn = m.mlp_head[0]
        bn.weight.copy_(1 + 0.1 * torch.randn(128)); bn.bias.copy_(0.1 * torch.randn(128))
    p0 = {k: v.clone() for k, v in sd(m).items()}
    # (images are stored as fp16: they are rounded to it BEFORE the reference sees them, so the stored values are the exact inputs)
    crops = [torch.randn(2, 3, s, s).clamp(-1, 1).half().float() for s in (112, 112, 48, 48, 48)]
    crops[0].requires_grad_(True)
    w = torch.randn(10, 128)
    m.train()
    z = m(crops)
    (z * w).sum().backward()
    bnb = {"bn." + k: v.clone() for k, v in bn.state_dict().items() if k.startswith(("running", "num"))}
    assert int(bnb["bn.num_batches_tracked"]) == 2
    m.eval()
    xe = torch.randn(3, 3, 112, 112).clamp(-1, 1).half().float()
    with torch.no_grad():
        ze = m(xe, for_fea=True)
    m2 = make(2)
    m2.load_state_dict(m.state_dict())
    m2.eval()
    xe2 = torch.randn(3, 3, 112, 112).clamp(-1, 1).half().float()
    with torch.no_grad():
        ze2 = m2(xe2, for_fea=True)
    arrays = dict(**p0, **grads(m), **bnb, w=w, z=z, gx112_a=crops[0].grad, xe=xe.half(), ze=ze, xe2=xe2.half(), ze2=ze2,
                  **{f"x{i}": c.detach().half() for i, c in enumerate(crops)})
    # no committed file may exceed 1 MiB and random floats do not compress: the arrays go, in key order, into as many parts as it takes
    # (f26_fvit.npz, f26_fvit_1.npz, ...; tests/test_fvit_host.py load_fvit() merges them)
    parts, room = [{}], PART_BYTES
    for k in sorted(arrays):
        nbytes = arrays[k].numel() * arrays[k].element_size()
        if nbytes > room and parts[-1]:
            parts.append({}); room = PART_BYTES
        parts[-1][k] = arrays[k]; room -= nbytes
    for i, part in enumerate(parts):
        save("f26_fvit" + (f"_{i}" if i else ""), **part)


if __name__ == "__main__":
    main()
