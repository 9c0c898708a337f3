"""CPU checks of the landmark-teacher modes (`pre_land` / `keep_land`, reference train_largescale.py:435-437, 565-582, 807-843): the
weight schedule against the table the reference's own lines produced, the argument errors of the entry point and of FinetuneEngine,
and the fp64 oracle the GPU test of lafs_landmark_mse relies on (tests/land_mse_cases.py): it is torch's MSELoss, an fp32 emulation of
the kernel passes its bounds, and seeded faults fail them."""
import numpy as np
import pytest
import torch

import land_mse_cases as LM
from conftest import load_golden
from fvit_cases import FVIT_CFG


def _args(*argv):
    from lafs_cvpr2024_amd import train_largescale as T
    return T.get_args_parser().parse_args(list(argv))


def test_land_loss_control_equals_the_reference_table():
    from lafs_cvpr2024_amd import train_largescale as T
    table = load_golden("f28_pre_land")["schedule"].tolist()
    assert len(table) == 41
    assert [float(T.land_loss_control(e)) for e in range(41)] == table
    assert [T.land_loss_control(e) for e in (0, 7, 8, 13, 14, 20, 21, 27, 28)] == [1000, 1000, 100, 100, 1, 1, 0.11, 0.11, 0]


@pytest.mark.parametrize("argv,match", [
    (("--keep_land", "true"), "needs --pre_land"),
    (("--pre_land", "true", "--with_land", "true"), "needs --with_land false"),
    (("--pre_land", "true", "--keep_land", "true", "--with_land", "false"), "needs --with_land true"),
    (("--pre_land", "true", "--with_land", "false", "--net", "VITs"), "VITs"),
    (("--pre_land", "true", "--keep_land", "true", "--net", "VITs"), "VITs"),
])
def test_entry_point_argument_errors(argv, match):
    from lafs_cvpr2024_amd import train_largescale as T
    args = _args(*argv)
    with pytest.raises(SystemExit, match=match):
        T.check_net_args(args)
    with pytest.raises(SystemExit, match=match):
        T.main(args)                                                         # (refused before anything is initialised)


def test_entry_point_accepts_the_two_modes_and_defaults_to_neither():
    from lafs_cvpr2024_amd import train_largescale as T
    d = _args()
    assert (d.pre_land, d.keep_land, d.land_loss_weight) == (False, False, None)
    assert T.build_landmark_teacher(d) is None
    T.check_net_args(_args("--pre_land", "true", "--with_land", "false"))
    T.check_net_args(_args("--pre_land", "true", "--keep_land", "true"))
    assert _args("--land_loss_weight", "0.5").land_loss_weight == 0.5
    # the verification and IJB entry points read the same flags from the shared parser
    import argparse
    p = argparse.ArgumentParser(parents=[T.get_args_parser()], conflict_handler="resolve")
    p.add_argument("--checkpoint", default="")
    a = p.parse_args(["--pre_land", "true", "--with_land", "false", "--pretrain_path", "stage1.pth", "--checkpoint", "x.pth"])
    assert a.pre_land and not a.keep_land and a.pretrain_path == "stage1.pth"


def test_teacher_is_built_with_the_reference_arguments(capsys):
    from lafs_cvpr2024_amd import train_largescale as T
    from lafs_cvpr2024_amd.face_pre_pro.ViT_face import face_landmark_4simmin_glo_loc
    t = T.build_landmark_teacher(_args("--pre_land", "true", "--with_land", "false"))
    assert "seeded initialisation" in capsys.readouterr().out                # no --pretrain_path: a warning, as lafs_train.py
    assert isinstance(t, face_landmark_4simmin_glo_loc) and not t.training
    assert (t.num_patches, t.patch_size, t.dim, t.row_num) == (196, 8, 512, 14)
    assert t.output_layer[1].out_features == 392 and tuple(t.pos_embedding.shape) == (1, 197, 512)


def test_engine_refusals_come_before_any_device_work():
    from lafs_cvpr2024_amd import _lib
    from lafs_cvpr2024_amd.face_pre_pro.ViT_face import ViT_face_landmark_patch8, ViTs_face_overlap
    from lafs_cvpr2024_amd.finetune_engine import FinetuneEngine
    teacher = torch.nn.Module()
    teacher.stn, teacher.output_layer = torch.nn.Identity(), torch.nn.Identity()
    with pytest.raises(_lib.LafsHipError, match="needs a landmark_teacher"):
        FinetuneEngine(None, 8, keep_land=True)
    with pytest.raises(_lib.LafsHipError, match="with_land=True"):           # mode B on a backbone without a branch
        FinetuneEngine(None, 8, landmark_teacher=teacher, keep_land=True)
    with pytest.raises(_lib.LafsHipError, match="ViTs_face_overlap"):        # mode A passes its own checks: the backbone check fires
        FinetuneEngine(None, 8, landmark_teacher=teacher)
    with pytest.raises(_lib.LafsHipError, match="mix_mode"):                 # the mixing checks still come first
        FinetuneEngine(None, 8, mix_mode="half", keep_land=True)
    cfg = dict(loss_type="CosFace", GPU_ID=None, num_class=16, image_size=112, patch_size=8, dim=64, depth=1, heads=1, mlp_dim=64)
    with pytest.raises(_lib.LafsHipError, match="with_land=False"):          # mode A on a backbone with its own branch
        FinetuneEngine(ViT_face_landmark_patch8(with_land=True, **cfg), 8, landmark_teacher=teacher)
    with pytest.raises(_lib.LafsHipError, match="with_land=True"):
        FinetuneEngine(ViT_face_landmark_patch8(with_land=False, **cfg), 8, landmark_teacher=teacher, keep_land=True)
    fvit = ViTs_face_overlap(pad=4, **{**FVIT_CFG, "loss_type": "CosFace", "num_class": 16})
    for keep in (False, True):
        with pytest.raises(_lib.LafsHipError, match="fViT"):
            FinetuneEngine(fvit, 8, landmark_teacher=teacher, keep_land=keep)
    with pytest.raises(_lib.LafsHipError, match="stn"):
        FinetuneEngine(ViT_face_landmark_patch8(with_land=False, **cfg), 8, landmark_teacher=torch.nn.Linear(2, 2))


def test_binding_and_hyper_slot():
    from lafs_cvpr2024_amd import _lib
    assert "lafs_landmark_mse" in _lib.EXPORTED and len(_lib._PROTOS["lafs_landmark_mse"]) == 9
    assert _lib.HP_LAND_W == _lib.HP_MIX_LAM + 1 < _lib.HP_COUNT


# ------------------------------------------------------------------------------------------------ the oracle of the kernel test
@pytest.mark.parametrize("B,n", [(1, 36), (5, 196)])
def test_oracle_is_torch_mse_and_its_autograd_in_float64(B, n):
    pred, label = LM.make_inputs("uniform", B, n)
    w, gs = LM.f32c(0.11), LM.f32c(1.0 / 3.0)
    g = np.random.RandomState(3)
    d_old, l_old = g.randn(B, n, 2), 7.25
    p = torch.tensor(pred, dtype=torch.float64, requires_grad=True)
    l = torch.tensor(label, dtype=torch.float64)
    loss_land = torch.nn.MSELoss()(l / 111.0, p / 111.0)
    (w * gs * loss_land).backward()
    loss_land = loss_land.detach()
    ref = LM.oracle(pred, label, w, gs, d_old, l_old)
    assert abs(ref["loss_land"] - float(loss_land)) <= 1e-12 * float(loss_land)
    assert abs(ref["loss"] - (l_old + w * gs * float(loss_land))) <= 1e-12 * abs(ref["loss"])
    want = d_old + p.grad.numpy()
    assert np.all(np.abs(ref["dtheta"] - want) <= 1e-12 * np.abs(want).max())


@pytest.mark.parametrize("kind", LM.INPUTS)
@pytest.mark.parametrize("B,n", LM.SHAPES)
def test_float32_emulation_of_the_kernel_passes_the_bounds(B, n, kind):
    pred, label = LM.make_inputs(kind, B, n)
    g = np.random.RandomState(5)
    d_old, l_old = g.randn(B, n, 2).astype(np.float32), np.float32(6.5)
    worst = {}
    for w in LM.WEIGHTS:
        for gs in LM.GRAD_SCALES:
            ll, lo, dt = LM.emulate_f32(pred, label, w, gs, d_old, l_old)
            ok, ratios = LM.check_case(ll, lo, dt, pred, label, w, gs, d_old, l_old)
            assert ok, (w, gs, ratios)
            for k, v in ratios.items():
                worst[k] = max(worst.get(k, 0.0), v)
            if w == 0.0:
                assert np.array_equal(dt, d_old) and lo == l_old            # exact zeros added
            if kind == "equal":
                assert ll == 0.0 and np.array_equal(dt, d_old) and lo == l_old
    print(f"[landmark mse emulation] B={B} n={n} {kind}: worst |err| / bound {worst}")
    if kind == "uniform":
        assert worst["dtheta"] > 0.05, "the gradient bound is within a factor 20 of what fp32 really does"


FAULTS = {
    "missing factor 2": lambda r, c: dict(dtheta=c["d_old"] + 0.5 * r["inc"]),
    "missing 1 / 111^2": lambda r, c: dict(dtheta=c["d_old"] + r["inc"] * 111.0 ** 2, loss_land=r["loss_land"] * 111.0 ** 2,
                                           loss=c["l_old"] + r["term"] * 111.0 ** 2),
    "mean over B n": lambda r, c: dict(dtheta=c["d_old"] + 2.0 * r["inc"], loss_land=2.0 * r["loss_land"], loss=c["l_old"] + 2.0 * r["term"]),
    "flipped sign": lambda r, c: dict(dtheta=c["d_old"] - r["inc"]),
    "weight ignored": lambda r, c: dict(dtheta=c["d_old"] + r["inc"] / c["w"], loss=c["l_old"] + r["term"] / c["w"]),
    "grad_scale ignored": lambda r, c: dict(dtheta=c["d_old"] + r["inc"] / c["gs"], loss=c["l_old"] + r["term"] / c["gs"]),
    "overwrite instead of accumulate": lambda r, c: dict(dtheta=r["inc"], loss=r["term"]),
}


@pytest.mark.parametrize("fault", sorted(FAULTS))
def test_seeded_faults_fail_the_bounds(fault):
    B, n = 2, 196
    pred, label = LM.make_inputs("uniform", B, n)
    w, gs = LM.f32c(0.11), LM.f32c(1.0 / 3.0)
    g = np.random.RandomState(9)
    # (old values of the size the engine holds: gradients of the size of the increment, a loss of a few units)
    d_old, l_old = (1e-6 * g.randn(B, n, 2)).astype(np.float32), np.float32(6.5)
    ref = LM.oracle(pred, label, w, gs, d_old, l_old)
    good = dict(loss_land=np.float32(ref["loss_land"]), loss=np.float32(ref["loss"]), dtheta=ref["dtheta"].astype(np.float32))
    ok, _ = LM.check_case(good["loss_land"], good["loss"], good["dtheta"], pred, label, w, gs, d_old, l_old)
    assert ok, "the correctly rounded result passes"
    bad = dict(good)
    bad.update({k: np.asarray(v).astype(np.float32) for k, v in FAULTS[fault](ref, dict(d_old=d_old.astype(np.float64), l_old=float(l_old), w=w, gs=gs)).items()})
    ok, ratios = LM.check_case(bad["loss_land"], bad["loss"], bad["dtheta"], pred, label, w, gs, d_old, l_old)
    assert not ok, (fault, ratios)
    assert ratios["dtheta"] > 1.0, (fault, ratios)          # every one of these faults shows in the gradient
