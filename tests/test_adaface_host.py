"""CPU: the AdaFace plumbing that needs no GPU -- the entry points' parsers, the class and buffer names build_backbone produces, a strict
load of an AdaFace checkpoint through the verification entry's parser and builder, and a CosFace checkpoint that must not load into an
AdaFace model silently."""
import argparse
import re

import pytest
import torch

from lafs_cvpr2024_amd import _lib, train_largescale as tl
from lafs_cvpr2024_amd.face_pre_pro.ViT_face import AdaFace, CosFace, ViT_face_landmark_patch8, ViTs_face_overlap


def _small(loss_type, num_class=40):
    return ViT_face_landmark_patch8(loss_type=loss_type, GPU_ID=None, num_class=num_class, image_size=112, patch_size=8, dim=64, depth=1,
                                    heads=1, mlp_dim=64, with_land=False)


def test_parser_offers_the_adaface_head_and_its_two_flags():
    p = tl.get_args_parser()
    a = p.parse_args("--head AdaFace".split())
    assert a.head == "AdaFace" and a.adaface_h == 0.333 and a.adaface_t_alpha == 0.01
    a = p.parse_args("--head AdaFace --adaface_h 0.5 --adaface_t_alpha 0.02".split())
    assert (a.adaface_h, a.adaface_t_alpha) == (0.5, 0.02)
    with pytest.raises(SystemExit):
        p.parse_args("--head SphereFace".split())
    with pytest.raises(SystemExit):                      # the class-sharded form is out of scope: --partial_margin keeps its two choices
        p.parse_args("--head PartialFC --partial_margin AdaFace".split())


def test_the_evaluation_entries_inherit_the_head_choice():
    from lafs_cvpr2024_amd import ijb_evaluation, verification  # noqa: F401
    p = argparse.ArgumentParser("v", parents=[tl.get_args_parser()])
    p.add_argument("--checkpoint", required=True, type=str)
    assert p.parse_args("--head AdaFace --checkpoint x.pth".split()).head == "AdaFace"
    src = open(ijb_evaluation.__file__).read() + open(verification.__file__).read()
    assert len(re.findall(r"parents=\[tl\.get_args_parser\(\)\]", src)) == 2 and len(re.findall(r"tl\.build_backbone\(args\)", src)) == 2


def test_both_backbones_build_the_adaface_head_under_the_cosface_names():
    for model in (_small("AdaFace"),
                  ViTs_face_overlap(loss_type="AdaFace", GPU_ID=None, num_class=40, image_size=112, patch_size=8, ac_patch_size=12, pad=4, dim=64,
                                    depth=1, heads=1, mlp_dim=64)):
        assert isinstance(model.loss, AdaFace) and not isinstance(model.loss, CosFace)
        sd = model.state_dict()
        assert tuple(sd["loss.weight"].shape) == (40, 64)
        assert sd["loss.batch_mean"].tolist() == [20.0] and sd["loss.batch_std"].tolist() == [100.0]
        assert sd["loss.batch_mean"].dtype == torch.float32
        assert {"batch_mean", "batch_std"} == {n for n, _ in model.loss.named_buffers()}
        assert (model.loss.s, model.loss.m, model.loss.h, model.loss.t_alpha, model.loss.eps) == (64.0, 0.4, 0.333, 0.01, 1e-3)
    torch.manual_seed(0)
    a = AdaFace(64, 40, None)
    torch.manual_seed(0)
    c = CosFace(64, 40, None)
    assert torch.equal(a.weight, c.weight)               # the same initialisation
    with pytest.raises(NotImplementedError, match="only 'CosFace' and 'None'"):
        _small("SphereFace")


def test_state_storage_keeps_the_buffers_live_views_of_one_state():
    a = AdaFace(64, 40, None)
    st = a.state_storage()
    assert st.tolist() == [20.0, 100.0] and a.state_storage() is st
    st[0], st[1] = 21.5, 3.25                            # what the kernel does
    assert a.state_dict()["batch_mean"].tolist() == [21.5] and a.state_dict()["batch_std"].tolist() == [3.25]
    a.load_state_dict({"weight": torch.zeros(40, 64), "batch_mean": torch.tensor([7.0]), "batch_std": torch.tensor([8.0])})
    assert st.tolist() == [7.0, 8.0]
    assert sorted(a.state_dict()) == ["batch_mean", "batch_std", "weight"]


def test_build_backbone_and_strict_checkpoint_load(tmp_path, monkeypatch):
    """--head AdaFace --checkpoint ...: what train_largescale.py saves (`module.`-prefixed) loads strictly into what the verification
    entry builds from the same flags; a CosFace checkpoint is refused by its missing keys, and the other way round by unexpected ones."""
    built = {}

    def small(**kw):
        built.update(kw)
        return _small(kw["loss_type"], kw["num_class"])
    monkeypatch.setattr(tl, "ViT_face_landmark_patch8", small)
    p = argparse.ArgumentParser("v", parents=[tl.get_args_parser()])
    p.add_argument("--checkpoint", required=True, type=str)
    path = str(tmp_path / "Backbone_VIT_Epoch_1.pth")
    args = p.parse_args(f"--head AdaFace --num_class 40 --with_land false --checkpoint {path}".split())
    trained = tl.build_backbone(args)
    assert built["loss_type"] == "AdaFace" and isinstance(trained.loss, AdaFace)
    trained.loss.state_storage()[:] = torch.tensor([19.25, 2.5])
    torch.save({"module." + k: v for k, v in trained.state_dict().items()}, path)
    sd = {k[len("module."):]: v for k, v in torch.load(path, map_location="cpu").items()}
    fresh = tl.build_backbone(args)
    assert fresh.load_state_dict(sd, strict=True).missing_keys == []
    assert fresh.loss.batch_mean.tolist() == [19.25] and fresh.loss.batch_std.tolist() == [2.5]
    cos = tl.build_backbone(p.parse_args(f"--head CosFace --num_class 40 --with_land false --checkpoint {path}".split()))
    assert built["loss_type"] == "CosFace"
    with pytest.raises(RuntimeError, match="Missing key.*loss.batch_mean"):
        fresh.load_state_dict(cos.state_dict())
    with pytest.raises(RuntimeError, match="Unexpected key.*loss.batch_mean"):
        cos.load_state_dict(sd)
    sharded = tl.build_backbone(p.parse_args(f"--head PartialFC --num_class 40 --with_land false --checkpoint {path}".split()))
    assert built["loss_type"] == "None" and not hasattr(sharded, "loss")


def test_abi_declares_the_two_new_entries():
    for name in ("lafs_adaface_margins", "lafs_margin_softmax_ce_ada_bf16"):
        assert name in _lib.EXPORTED
