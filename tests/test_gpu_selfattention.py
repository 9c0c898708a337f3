"""GPU parity of the inspection API -- VisionTransformer.get_last_selfattention / get_intermediate_layers (F23) and
ViT_face_landmark_patch8.get_selfattention (F24) -- against what the reference itself returned, and the attention-map tool."""
import os
import subprocess
import sys
from functools import partial

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

from conftest import ROOT, det_fill, det_fill_random, load_golden, sub  # noqa: E402
from lafs_cvpr2024_amd import vision_transformer as vits  # noqa: E402
from lafs_cvpr2024_amd.face_pre_pro.ViT_face import ViT_face_landmark_patch8  # noqa: E402

DEV = "cuda"
ROW_SUM_TOL = 5e-5          # as tests/test_gpu_attention_probs.py
GATE_F23_ATTN = 6.0e-3      # observed 2.87e-3 (112 x 112) / 3.00e-3 (48 x 48) on MI355X; gate = 2x the worse
GATE_F24_ATTN = 2.0e-3      # observed 1.00e-3 (last block) / 0.99e-3 (first block) on MI355X; gate = 2x the worse


def rel_l2(a, b):
    a, b = a.detach().double().cpu(), b.detach().double().cpu()
    return ((a - b).norm() / (b.norm() + 1e-30)).item()


def _f23_model():
    m = vits.VisionTransformer(img_size=[112], patch_size=8, embed_dim=128, depth=3, num_heads=2, qkv_bias=True,
                               norm_layer=partial(torch.nn.LayerNorm, eps=1e-6))
    det_fill_random(m)                      # the fixture's weights (tools/make_golden_attention.py; pinned by its key sums on the CPU)
    vits.attach_arena(m, DEV)
    return m.eval()


@pytest.mark.parametrize("tag,N", [("g", 197), ("l", 37)])
def test_f23_vit_selfattention_and_intermediate_layers(tag, N):
    fx = load_golden("f23_vit_selfattention")
    m = _f23_model()
    x = fx["x" + tag].to(DEV)
    B = x.shape[0]
    inter = m.get_intermediate_layers(x, 2)
    assert len(inter) == 2
    for i, t in enumerate(inter):
        assert t.shape == (B, N, 128) and t.dtype == torch.float32
        e = rel_l2(t, fx[f"inter_{tag}{i}"])
        print(f"[F23 {tag}] intermediate layer {i}: rel-L2 {e:.3e}")
        assert e < 2e-2
    last = m.get_intermediate_layers(x, 1)
    assert len(last) == 1 and torch.equal(last[0], inter[1])
    assert torch.equal(last[0][:, 0], m(x))
    assert torch.equal(m.get_intermediate_layers(x, 3)[1], inter[0])
    attn = m.get_last_selfattention(x)
    assert attn.shape == (B, 2, N, N) and attn.dtype == torch.float32
    off = (attn.double().sum(-1) - 1).abs().max().item()
    e = rel_l2(attn, fx["attn_" + tag])
    print(f"[F23 {tag}] last self-attention: rel-L2 {e:.3e} (gate {GATE_F23_ATTN:.1e}), row sums off by {off:.3e}")
    assert off < ROW_SUM_TOL
    assert e < GATE_F23_ATTN


def test_f24_partfvit_selfattention():
    f13, fx = load_golden("f13_partfvit_land"), load_golden("f24_partfvit_selfattention")
    m = ViT_face_landmark_patch8(loss_type="None", GPU_ID=None, num_class=10, image_size=112, patch_size=8, dim=128, depth=2,
                                 heads=3, mlp_dim=256, dropout=0.0, emb_dropout=0.0, with_land=True)
    det_fill(m.stn); det_fill(m.output_layer)
    missing, unexpected = m.load_state_dict(sub(f13, "p."), strict=False)
    assert not unexpected and all(k.startswith(("stn.", "output_layer.")) for k in missing)
    vits.attach_arena(m, DEV)
    m.eval()
    x = f13["x"][:1].to(DEV)
    errs = {}
    for key, layer in (("attn_last", -1), ("attn_first", 0)):
        attn, theta = m.get_selfattention(x, layer=layer)
        assert attn.shape == (1, 3, 197, 197) and attn.dtype == torch.float32 and theta.shape == (1, 196, 2)
        assert (attn.double().sum(-1) - 1).abs().max().item() < ROW_SUM_TOL
        torch.testing.assert_close(theta.detach().cpu(), fx["theta"], rtol=1e-3, atol=2e-2)          # the F13 gates of test_gpu_finetune.py
        cls, theta2 = m.get_selfattention(x, layer=layer, cls_only=True)
        assert cls.shape == (1, 3, 1, 197) and torch.equal(cls, attn[:, :, :1]) and torch.equal(theta2, theta)
        errs[key] = rel_l2(attn, fx[key])
        print(f"[F24] {key}: rel-L2 {errs[key]:.3e} (gate {GATE_F24_ATTN:.1e})")
    assert torch.equal(m.get_selfattention(x, layer=1)[0], m.get_selfattention(x)[0])
    with torch.no_grad():
        e, theta_fwd = m(x, visualize=True)
    assert torch.equal(theta_fwd, theta)
    assert rel_l2(e, fx["e"]) < 2e-2
    assert max(errs.values()) < GATE_F24_ATTN, errs


@pytest.mark.parametrize("arch,dims,heads", [("partfvit", "128,2,3,256", 3), ("vit_small", "128,2,2,512", 2)])
def test_attention_map_tool_smoke(tmp_path, arch, dims, heads):
    cmd = [sys.executable, os.path.join(ROOT, "tools", "attention_maps.py"), "--arch", arch, "--dims", dims, "--random-init", "--num", "2",
           "--out", str(tmp_path)]
    p = subprocess.run(cmd, capture_output=True, text=True, timeout=600, env=dict(os.environ, PYTHONPATH=ROOT))
    assert p.returncode == 0, p.stdout[-3000:] + p.stderr[-3000:]
    from PIL import Image
    for b in range(2):
        for h in range(heads):
            w = np.load(tmp_path / f"img{b}_head{h}.npy")
            assert w.dtype == np.float32 and w.shape == ((196,) if arch == "partfvit" else (14, 14))
            assert (w >= 0).all() and 0 < w.sum() <= 1 + 1e-6             # the cls -> cls weight is the rest of the row
            with Image.open(tmp_path / f"img{b}_head{h}.png") as im:
                assert im.size == (112, 112) and im.mode == "RGB"
        if arch == "partfvit":
            assert np.load(tmp_path / f"img{b}_theta.npy").shape == (196, 2)
