#!/usr/bin/env python3
"""Generate the attention read-out fixtures (F23, F24) under tests/golden/ by running the REFERENCE itself.

Same recipe as tools/make_golden.py (whose import shims are reused): the reference's own modules on CPU in fp32, small seeded
inputs, data only in the .npz files.

  f23_vit_selfattention.npz      VisionTransformer (patch 8, embed 128, depth 3, 2 heads, qkv_bias, LN eps 1e-6, eval):
                                 get_last_selfattention and get_intermediate_layers(x, 2) for a 112x112 batch (197 tokens) and a
                                 48x48 batch (37 tokens)
  f24_partfvit_selfattention.npz the model and the first image of f13_partfvit_land.npz, eval: the last and the first block's
                                 `attention_score` behind one forward, theta and the embedding

F23's 0.64 M parameters are more than a fixture may weigh, so they are not stored: both sides fill the (identical) state_dict with
tests/conftest.det_fill_random, as F9 / F13 / F18 do for the landmark CNN; the fixture keeps the key list and one fp64 sum per
tensor so that a drift of that fill is noticed.  F24's trunk weights and input are the ones stored in f13_partfvit_land.npz.

Usage:  python tools/make_golden_attention.py [--out DIR]      (default: tests/golden; deterministic)
"""
import argparse
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.join(ROOT, "tests"))

from make_golden import _import_reference, npy  # noqa: E402


def save(out, name, **arrays):
    os.makedirs(out, exist_ok=True)
    path = os.path.join(out, name + ".npz")
    np.savez_compressed(path, **{k: npy(v) for k, v in arrays.items()})
    print(f"  wrote {path}  ({os.path.getsize(path) / 1024:.0f} KiB, {len(arrays)} arrays)")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "tests", "golden"))
    args = ap.parse_args()
    _, ref_vit, _, ref_face, _ = _import_reference()
    from conftest import det_fill, det_fill_random, load_golden, sub
    torch.set_num_threads(4)

    print("F23 vit self-attention / intermediate layers")
    torch.manual_seed(23)
    m = ref_vit.VisionTransformer(img_size=[112], patch_size=8, embed_dim=128, depth=3, num_heads=2, mlp_ratio=4, qkv_bias=True,
                                  norm_layer=lambda d: torch.nn.LayerNorm(d, eps=1e-6), drop_path_rate=0.0)
    det_fill_random(m)
    m.eval()
    xg = torch.randn(1, 3, 112, 112).clamp(-1, 1)
    xl = torch.randn(2, 3, 48, 48).clamp(-1, 1)
    with torch.no_grad():
        ag, al = m.get_last_selfattention(xg), m.get_last_selfattention(xl)
        ig, il = m.get_intermediate_layers(xg, 2), m.get_intermediate_layers(xl, 2)
    keys = sorted(m.state_dict().keys())
    save(args.out, "f23_vit_selfattention", xg=xg, xl=xl, attn_g=ag, attn_l=al, inter_g0=ig[0], inter_g1=ig[1], inter_l0=il[0],
         inter_l1=il[1], keys=np.array(keys), key_sums=np.array([float(m.state_dict()[k].double().sum()) for k in keys]))

    print("F24 part-fvit attention_score")
    f13 = load_golden("f13_partfvit_land")
    pl = ref_face.ViT_face_landmark_patch8(loss_type="None", GPU_ID=None, num_class=10, image_size=112, patch_size=8, dim=128, depth=2,
                                           heads=3, mlp_dim=256, dropout=0.0, emb_dropout=0.0, with_land=True)
    det_fill(pl.stn); det_fill(pl.output_layer)
    missing, unexpected = pl.load_state_dict(sub(f13, "p."), strict=False)
    assert not unexpected and all(k.startswith(("stn.", "output_layer.")) for k in missing)
    pl.eval()
    with torch.no_grad():
        e = pl(f13["x"][:1])
    score = lambda l: pl.transformer.layers[l][0].fn.fn.attention_score
    save(args.out, "f24_partfvit_selfattention", attn_last=score(-1), attn_first=score(0), theta=pl.theta, e=e)


if __name__ == "__main__":
    main()
