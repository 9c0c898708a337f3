"""CPU checks of the attention read-out (lafs_attention_probs, VisionTransformer.get_last_selfattention / get_intermediate_layers,
ViT_face_landmark_patch8.get_selfattention): the surface exists, the reference-made fixtures F23 / F24 are what they claim to be, and
the argument checks that need no device raise."""
import os
import subprocess
import sys
from functools import partial

import numpy as np
import pytest
import torch

from conftest import GOLDEN, ROOT, det_fill_random, load_golden

# The reference's softmax rows, summed in fp64, miss 1 by at most 1.5e-7 on both fixtures (2.4e-7 summed in fp32) -- measured on the
# CPU from the fixtures alone; 1e-6 = 8 ulp of fp32 at 1.0 leaves that room and would not hide a lost entry (the smallest row
# maximum is 5e-3).
ROW_SUM_TOL = 1e-6


def _vit():
    from lafs_cvpr2024_amd import vision_transformer as vits
    return vits.VisionTransformer(img_size=[112], patch_size=8, embed_dim=128, depth=3, num_heads=2, qkv_bias=True,
                                  norm_layer=partial(torch.nn.LayerNorm, eps=1e-6))


def _partfvit(**kw):
    from lafs_cvpr2024_amd.face_pre_pro.ViT_face import ViT_face_landmark_patch8
    return ViT_face_landmark_patch8(loss_type="None", GPU_ID=None, num_class=10, image_size=112, patch_size=8, dim=128, depth=2, heads=3,
                                    mlp_dim=256, dropout=0.0, emb_dropout=0.0, **kw)


def test_entry_point_is_bound():
    from lafs_cvpr2024_amd import _lib, ops
    assert "lafs_attention_probs" in _lib.EXPORTED
    assert callable(ops.attention_probs)


def test_modules_have_the_inspection_methods():
    from lafs_cvpr2024_amd import vision_transformer as vits
    from lafs_cvpr2024_amd.face_pre_pro.ViT_face import ViT_face_landmark_patch8
    assert callable(vits.VisionTransformer.get_last_selfattention) and callable(vits.VisionTransformer.get_intermediate_layers)
    assert callable(ViT_face_landmark_patch8.get_selfattention)


def test_f23_fixture_rows_sum_to_one_and_shapes():
    fx = load_golden("f23_vit_selfattention")
    for tag, B, N in (("g", 1, 197), ("l", 2, 37)):
        a = fx["attn_" + tag]
        assert a.shape == (B, 2, N, N) and a.dtype == torch.float32 and bool((a >= 0).all())
        assert (a.double().sum(-1) - 1).abs().max().item() < ROW_SUM_TOL
        for i in range(2):
            assert fx[f"inter_{tag}{i}"].shape == (B, N, 128)
    # the weights are not stored: the fill both sides use must still produce what the generator saw
    m = _vit()
    det_fill_random(m)
    sd = m.state_dict()
    assert [str(k) for k in fx["keys"]] == sorted(sd)
    np.testing.assert_allclose([float(sd[str(k)].double().sum()) for k in fx["keys"]], fx["key_sums"].numpy(), rtol=0, atol=1e-9)


def test_f24_fixture_rows_sum_to_one_and_shapes():
    fx = load_golden("f24_partfvit_selfattention")
    for k in ("attn_last", "attn_first"):
        a = fx[k]
        assert a.shape == (1, 3, 197, 197) and a.dtype == torch.float32 and bool((a >= 0).all())
        assert (a.double().sum(-1) - 1).abs().max().item() < ROW_SUM_TOL
    assert fx["theta"].shape == (1, 196, 2) and fx["e"].shape == (1, 128)
    assert not torch.equal(fx["attn_last"], fx["attn_first"])


def test_generator_reproduces_the_fixtures(tmp_path):
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    from make_golden import REF
    if not os.path.isdir(REF):
        pytest.skip("the reference checkout is not mounted")
    p = subprocess.run([sys.executable, os.path.join(ROOT, "tools", "make_golden_attention.py"), "--out", str(tmp_path)],
                       capture_output=True, text=True, timeout=900)
    assert p.returncode == 0, p.stdout[-2000:] + p.stderr[-2000:]
    for name in ("f23_vit_selfattention.npz", "f24_partfvit_selfattention.npz"):
        new, old = np.load(tmp_path / name), np.load(os.path.join(GOLDEN, name))
        assert sorted(new.files) == sorted(old.files)
        for k in old.files:
            assert new[k].dtype == old[k].dtype and new[k].shape == old[k].shape and new[k].tobytes() == old[k].tobytes(), (name, k)


@pytest.mark.parametrize("n", [0, 4, -1])
def test_intermediate_layers_range_is_checked_before_any_device_work(n):
    with pytest.raises(ValueError):
        _vit().get_intermediate_layers(torch.zeros(1, 3, 112, 112), n)


def test_selfattention_refuses_training_mode_and_bad_layers():
    m = _partfvit()
    m.train()
    with pytest.raises(RuntimeError, match="eval"):
        m.get_selfattention(torch.zeros(1, 3, 112, 112))
    m.eval()
    for layer in (2, -3):
        with pytest.raises(ValueError):
            m.get_selfattention(torch.zeros(1, 3, 112, 112), layer=layer)
