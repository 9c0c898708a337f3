"""CPU tests of the mixing recipe beyond batch-mode mixup (CutMix, pair / elem modes, label smoothing): the host Mixup class and the
dense oracle against the reference's own results (tests/golden/f25_mixup_modes.npz, tools/make_golden_mixup.py), the RNG contract of the
engine's parameter draw, the command line and the ABI table."""
import os
import re
import types

import numpy as np
import pytest
import torch

from conftest import load_golden, sub
from test_oracle_golden import close
import mixup_oracle as mo

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
C = 50
FX = load_golden("f25_mixup_modes")
NAMES = [str(n) for n in FX["names"]]


def case(name):
    c = sub(FX, "c." + name + ".")
    ma, ca, mn, mx, prob, sw, eps, seed = (float(v) for v in c["cfg"])
    c["kw"] = dict(mixup_alpha=ma, cutmix_alpha=ca, cutmix_minmax=None if mn < 0 else (mn, mx), prob=prob, switch_prob=sw,
                   mode=name.split("_")[0], label_smoothing=eps, num_classes=C)
    c["seed"], c["eps"] = int(seed), eps
    return c


def test_fixture_covers_the_recipe():
    modes = {n.split("_")[0] for n in NAMES}
    assert modes == {"batch", "pair", "elem"}
    for mode in modes:
        kinds = {n.split("_")[1] for n in NAMES if n.startswith(mode)}
        assert {"mixup", "cutmix", "switch", "minmax"} <= kinds, (mode, kinds)
    assert {case(n)["eps"] for n in NAMES} == {0.0, 0.1}
    p05 = case("elem_switch_p05_s1")
    assert 0 < int((p05["lam"] == 1.0).sum()) < 8                       # prob 0.5: some rows stay unmixed
    assert any(case(n)["y"][1] == case(n)["y"][6] for n in NAMES)       # a row whose partner carries its own class


@pytest.mark.parametrize("name", NAMES)
def test_host_mixup_reproduces_the_reference(name):
    """Same np.random stream, same fp32 operations: mixed images, dense targets and lambdas are the reference's, exactly."""
    from lafs_cvpr2024_amd.util.mixup_my import Mixup
    c = case(name)
    np.random.seed(c["seed"])
    x, t = Mixup(**c["kw"])(c["x_in"].clone(), c["y"], device="cpu")
    assert torch.equal(x, c["x_out"])
    assert torch.equal(t, c["target"])
    keys, pos = np.random.get_state()[1:3]
    assert np.array_equal(keys, c["rng_keys"].numpy()) and pos == int(c["rng_pos"])
    # the parameter draw alone: same lambdas, same RNG state, and (through the oracle's mixing) the same images
    mix = Mixup(**c["kw"])
    np.random.seed(c["seed"])
    lam, cut, box = mix.draw_params(8, (16, 16))
    keys, pos = np.random.get_state()[1:3]
    assert np.array_equal(keys, c["rng_keys"].numpy()) and pos == int(c["rng_pos"])
    assert lam.dtype == np.float32 and cut.dtype == bool and box.shape == (8, 4)
    if name.startswith("batch"):
        assert mix.last_lam == float(c["lam"][0]) and np.all(lam == np.float32(mix.last_lam))
    else:
        assert np.array_equal(lam.astype(np.float64), c["lam"].numpy())
    if "_cutmix_" in name:
        assert cut.all()
    if "_mixup_" in name:
        assert not cut.any()
    xo = mo.mix_images(c["x_in"], lam, cut, box)
    if name.startswith("batch") and not cut.any():
        close(xo, c["x_out"], 1e-6, 1e-7)           # x.mul_(lam) with a Python double against fp32 lambdas (F11's tolerance)
    else:
        assert torch.equal(xo, c["x_out"])
    # partner of row b is row B-1-b; pair mode: both rows of a pair share lambda, decision and box
    if name.startswith("pair"):
        assert np.array_equal(lam, lam[::-1]) and np.array_equal(cut, cut[::-1]) and np.array_equal(box, box[::-1])


@pytest.mark.parametrize("name", NAMES)
def test_dense_oracle_reproduces_the_reference_loss_and_gradients(name):
    """tests/mixup_oracle.py (fp64) against the reference's CosFace soft branch + soft-target CE: the tolerances
    tests/test_oracle_golden.py applies to F10 and F11."""
    c = case(name)
    tgt = mo.dense_target(c["y"], C, c["lam"], c["eps"])
    close(tgt, c["target"], 1e-6, 1e-7)
    assert float((tgt.sum(1) - 1).abs().max()) < 1e-12
    emb = FX["emb"].double().requires_grad_(True)
    W = FX["weight"].double().requires_grad_(True)
    logits = mo.cosface_dense_from_cos(mo.cosine(emb, W), tgt)
    close(logits.detach(), c["logits"], 1e-5, 1e-5)
    ce = mo.soft_ce(logits, tgt)
    close(ce.detach(), c["ce"], 1e-5, 1e-6)
    ce.backward()
    close(emb.grad, c["gemb"], 1e-4, 1e-6)
    close(W.grad, c["gweight"], 1e-4, 1e-6)
    loss, rows, gcos = mo.loss_and_dcos(c["cos"], c["y"], c["lam"], c["eps"])
    close(loss, c["ce"], 1e-5, 1e-6)
    close(gcos, c["gcos"], 1e-4, 1e-6)


@pytest.mark.parametrize("name", ["batch_cutmix_s1", "pair_switch_s1", "elem_switch_p05_s1", "elem_minmax_s0"])
def test_engine_parameter_draw_leaves_the_rng_where_the_reference_does(name):
    """FinetuneEngine.draw_mix (what micro_step calls when no parameters are passed) consumes np.random exactly as the reference's
    Mixup.__call__ does on the same batch shape."""
    from lafs_cvpr2024_amd.finetune_engine import FinetuneEngine
    from lafs_cvpr2024_amd.util.mixup_my import Mixup
    c = case(name)
    eng = types.SimpleNamespace(mixer=Mixup(**c["kw"]), B=8, S=16, mixup_alpha=c["kw"]["mixup_alpha"])
    np.random.seed(c["seed"])
    lam, cut, box = FinetuneEngine.draw_mix(eng)
    keys, pos = np.random.get_state()[1:3]
    assert np.array_equal(keys, c["rng_keys"].numpy()) and pos == int(c["rng_pos"])
    assert np.array_equal(lam.astype(np.float64), c["lam"].float().double().numpy())


def test_existing_batch_mode_draw_is_unchanged():
    from lafs_cvpr2024_amd.util.mixup_my import Mixup
    mix = Mixup(mixup_alpha=0.2, cutmix_alpha=0.0, prob=0.5, mode="batch", label_smoothing=0.0, num_classes=C)
    np.random.seed(3)
    a = [mix.draw_lambda() for _ in range(20)]
    rng = np.random.RandomState(3)
    b = [float(rng.beta(0.2, 0.2)) if rng.rand() < 0.5 else 1.0 for _ in range(20)]
    assert a == b and 1.0 in a and any(v != 1.0 for v in a)


def test_engine_refuses_smoothing_where_it_is_undefined():
    from lafs_cvpr2024_amd import _lib
    from lafs_cvpr2024_amd.finetune_engine import FinetuneEngine
    with pytest.raises(_lib.LafsHipError, match="class-sharded head"):
        FinetuneEngine(None, 8, label_smoothing=0.1, sharded_head=object())
    with pytest.raises(_lib.LafsHipError, match="ArcFace"):
        FinetuneEngine(None, 8, label_smoothing=0.1, margin_type=1)
    with pytest.raises(_lib.LafsHipError, match="mix_mode"):
        FinetuneEngine(None, 8, mix_mode="half")


def test_cli_parses_the_mixing_flags_with_the_reference_defaults():
    from lafs_cvpr2024_amd import train_largescale as T
    a = T.get_args_parser().parse_args([])
    assert (a.mixup, a.cutmix, a.cutmix_minmax, a.mixup_prob, a.mixup_switch_prob, a.mixup_mode, a.smoothing) == \
        (0.2, 0.0, None, 0.1, 0.5, "batch", 0.0)                       # reference train_largescale.py:383-395
    assert T.mixing_active(a)
    a = T.get_args_parser().parse_args("--mixup 0 --cutmix 1.0 --cutmix-minmax 0.2 0.8 --mixup-switch-prob 0.3 --mixup-mode elem "
                                       "--smoothing 0.1 --mixup-prob 1".split())
    assert (a.mixup, a.cutmix, a.cutmix_minmax, a.mixup_prob, a.mixup_switch_prob, a.mixup_mode, a.smoothing) == \
        (0.0, 1.0, [0.2, 0.8], 1.0, 0.3, "elem", 0.1)
    assert T.mixing_active(a)                                            # timm's rule; the reference would train unmixed (:526)
    assert T.mixing_active(T.get_args_parser().parse_args("--mixup 0 --cutmix-minmax 0.2 0.8".split()))
    assert not T.mixing_active(T.get_args_parser().parse_args("--mixup 0".split()))
    with pytest.raises(SystemExit):
        T.get_args_parser().parse_args("--mixup-mode half".split())


def test_lib_lists_the_new_entry_points_with_the_headers_argument_count():
    from lafs_cvpr2024_amd import _lib
    txt = open(os.path.join(ROOT, "include", "lafs_hip.h")).read()
    txt = re.sub(r"/\*.*?\*/", "", txt, flags=re.S)
    for name in ("lafs_mix_normalize", "lafs_margin_softmax_ce_mix_bf16"):
        m = re.search(r"\bint\s+" + name + r"\s*\((.*?)\)\s*;", txt, flags=re.S)
        assert m, name
        n_args = len(m.group(1).split(","))
        assert "hipStream_t stream" in m.group(1)
        assert name in _lib.EXPORTED and len(_lib._PROTOS[name]) == n_args - 1, (name, n_args)     # (_PROTOS leaves the stream out)
    assert _lib.MIX_WORDS == 6
    assert re.search(r"LAFS_MIX_LAM = 0, LAFS_MIX_CUT, LAFS_MIX_YL, LAFS_MIX_YH, LAFS_MIX_XL, LAFS_MIX_XH, LAFS_MIX_WORDS", txt)
