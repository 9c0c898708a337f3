"""GPU: landmark supervision from a frozen stage-1 CNN in the fine-tune step (`pre_land` / `keep_land`, reference train_largescale.py:
435-437, 565-582, 807-843): lafs_landmark_mse against fp64 element by element, its seam in FinetuneEngine, both modes against the
reference fixture tests/golden/f28_pre_land.npz (tools/make_golden_pre_land.py), captured against eager, mode A's feed and its
verification."""
import functools
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(__file__))
import land_mse_cases as LM  # noqa: E402
from conftest import det_fill, det_fill_random, gate_errors, load_golden, sub  # noqa: E402
from lafs_cvpr2024_amd import _lib, ops  # noqa: E402
from lafs_cvpr2024_amd.face_pre_pro.ViT_face import ViT_face_landmark_patch8, face_landmark_4simmin_glo_loc  # noqa: E402
from lafs_cvpr2024_amd.ops import _p, call  # noqa: E402
from lafs_cvpr2024_amd.vision_transformer import attach_arena  # noqa: E402

pytestmark = pytest.mark.gpu
DEV = "cuda"
f32 = torch.float32
GATE_F13 = 3.5e-2                                    # the gate of test_f13_partfvit_with_trainable_landmark_branch (tests/test_gpu_finetune.py)
SENT = -7.0e4                                        # guard value: no output of any case comes near it


def rel_l2(a, b):
    a, b = a.detach().double().cpu(), b.detach().double().cpu()
    return float((a - b).norm() / b.norm())


@functools.lru_cache(maxsize=None)
def _fx():
    return load_golden("f28_pre_land")


@functools.lru_cache(maxsize=None)
def _f13_trunk():
    return sub(load_golden("f13_partfvit_land"), "p.")


def _teacher(fill=det_fill):
    """A small stand-in for the stage-1 model: only `.stn` and `.output_layer` are read."""
    t = face_landmark_4simmin_glo_loc(loss_type="None", GPU_ID=None, num_class=10, num_patches=196, image_size=112, patch_size=8, dim=64,
                                      depth=1, heads=1, mlp_dim=64)
    fill(t.stn); fill(t.output_layer)
    return t.eval()


def _fixture_backbone(with_land):
    """The fixture's backbone: F13's stored trunk, the fixture's class table, det_fill in the backbone's own CNN."""
    m = ViT_face_landmark_patch8(loss_type="CosFace", GPU_ID=None, num_class=16, image_size=112, patch_size=8, dim=128, depth=2, heads=3,
                                 mlp_dim=256, dropout=0.0, emb_dropout=0.0, with_land=with_land)
    state = dict(_f13_trunk())
    state["loss.weight"] = _fx()["class_table"]
    missing, unexpected = m.load_state_dict(state, strict=False)
    assert not unexpected and all(k.startswith(("stn.", "output_layer.")) for k in missing)
    if with_land:
        det_fill(m.stn); det_fill(m.output_layer)
    return m.eval()


def _thin(t, step):
    return t.reshape(-1, t.shape[-1])[::int(step)]


def _norms_match(params, keys, norms):
    """Every tensor the reference gives a gradient gets one here, with a norm within 10 % (as the F13 test holds them)."""
    ref = dict(zip([str(k) for k in keys], norms.tolist()))
    got = {k: float(p.grad.norm()) for k, p in params.items() if p.grad is not None and float(p.grad.abs().max()) > 0}
    assert set(ref) <= set(got) | {k for k, v in ref.items() if v == 0.0}
    off = {k: (got[k], v) for k, v in ref.items() if v > 0 and abs(got[k] - v) > 0.1 * v}
    assert not off, off


# ------------------------------------------------------------------------------------------------ 4. the kernel against fp64
@pytest.mark.parametrize("B,n", LM.SHAPES)
def test_landmark_mse_kernel_against_fp64_element_by_element(B, n):
    """Every output of lafs_landmark_mse within the bound tests/land_mse_cases.py builds from the kernel's own operation count (per
    pair 2 subtractions and 4 fused multiply-adds; a term of the sum passes through 2 ceil(B n / 1024) + 6 + 16 additions) and its
    reduction order; guard rows around every output untouched, the inputs unchanged, a second launch bit-identical, weight 0 and
    pred == label add exact zeros."""
    g = torch.Generator().manual_seed(B * 1000 + n)
    worst = {}
    for kind in LM.INPUTS:
        pred, label = LM.make_inputs(kind, B, n)
        pin = torch.full((B + 2, n, 2), SENT, dtype=f32)
        lin = torch.full((B + 2, n, 2), SENT, dtype=f32)
        pin[1:-1], lin[1:-1] = torch.from_numpy(pred), torch.from_numpy(label)
        pdev, ldev = pin.to(DEV), lin.to(DEV)
        d_old = (torch.randn(B, n, 2, generator=g) * 1e-4).to(f32)
        for w in LM.WEIGHTS:
            wdev = torch.tensor([w], dtype=f32, device=DEV)
            for gs in LM.GRAD_SCALES:
                for filled in (True, False):
                    runs = []
                    for _ in range(2):
                        dbuf = torch.full((B + 2, n, 2), SENT, dtype=f32)
                        dbuf[1:-1] = d_old
                        dbuf = dbuf.to(DEV)
                        lbuf = torch.tensor([SENT, 6.5, SENT], dtype=f32, device=DEV)
                        llbuf = torch.tensor([SENT, 123.0, SENT], dtype=f32, device=DEV)
                        call("lafs_landmark_mse", _p(pdev[1:]), _p(ldev[1:]), B, n, _p(wdev), gs, _p(llbuf[1:]),
                             _p(lbuf[1:]) if filled else None, _p(dbuf[1:]) if filled else None)
                        runs.append((llbuf.cpu(), lbuf.cpu(), dbuf.cpu()))
                    (ll, lo, dt), second = runs
                    assert all(torch.equal(a, b) for a, b in zip(runs[0], second)), "two launches give the same bits"
                    assert torch.equal(pdev.cpu(), pin) and torch.equal(ldev.cpu(), lin), "the inputs are read only"
                    assert ll[0] == SENT and ll[2] == SENT and lo[0] == SENT and lo[2] == SENT
                    assert bool((dt[0] == SENT).all()) and bool((dt[-1] == SENT).all())
                    if not filled:
                        assert float(lo[1]) == 6.5 and torch.equal(dt[1:-1], d_old), "NULL outputs: nothing else is written"
                    ok, ratios = LM.check_case(ll[1].numpy(), lo[1].numpy() if filled else None, dt[1:-1].numpy() if filled else None,
                                               pred, label, w, gs, d_old.numpy() if filled else None, 6.5 if filled else None)
                    assert ok, (kind, w, gs, filled, ratios)
                    for k, v in ratios.items():
                        worst[k] = max(worst.get(k, 0.0), v)
                    if filled and (w == 0.0 or kind == "equal"):
                        assert float(lo[1]) == 6.5 and torch.equal(dt[1:-1], d_old), "exact zeros added"
                    if kind == "equal":
                        assert float(ll[1]) == 0.0
    print(f"[landmark mse] B={B} n={n}: worst |err| / bound {worst}")


def test_landmark_mse_refuses_null_and_non_positive_arguments():
    t = torch.zeros(2, 36, 2, device=DEV)
    w, out = torch.ones(1, device=DEV), torch.zeros(1, device=DEV)
    good = [_p(t), _p(t), 2, 36, _p(w), 1.0, _p(out), None, None]
    call("lafs_landmark_mse", *good)
    for i, bad in ((0, None), (1, None), (4, None), (6, None), (2, 0), (3, 0), (2, -1), (5, 0.0), (5, -1.0)):
        args = list(good)
        args[i] = bad
        with pytest.raises(_lib.LafsHipError):
            call("lafs_landmark_mse", *args)
    ll = ops.landmark_mse(t, t + 1.0, w)
    assert abs(float(ll) - 1.0 / 111.0 ** 2) < 1e-6 / 111.0 ** 2
    with pytest.raises(_lib.LafsHipError):
        ops.landmark_mse(t, t[:1], w)


# ------------------------------------------------------------------------------------------------ 5. the seam in the engine
def _seam_run(weight):
    from lafs_cvpr2024_amd.finetune_engine import FinetuneEngine
    B, C = 8, 1000
    torch.manual_seed(6)
    m = ViT_face_landmark_patch8(loss_type="CosFace", GPU_ID=None, num_class=C, image_size=112, patch_size=8, dim=128, depth=2, heads=3,
                                 mlp_dim=256, dropout=0.0, emb_dropout=0.0, with_land=True, drop_path_rate=0.0)
    det_fill_random(m.stn); det_fill_random(m.output_layer)
    m.eval()
    eng = FinetuneEngine(m, B, acc_step=3, device=DEV, landmark_teacher=_teacher(), keep_land=True)
    assert eng.cnn is not None, "the default route: the HIP training plan of the landmark CNN"
    g = torch.Generator().manual_seed(9)
    u8 = torch.randint(0, 256, (B, 3, 112, 112), dtype=torch.uint8, generator=g).to(DEV)
    y = torch.randint(0, C, (B,), generator=g).to(DEV)
    eng.micro_step(u8, y, lam=1.0, land_weight=weight)
    torch.cuda.synchronize()
    return {k: getattr(eng, k).detach().double().cpu().numpy().copy() for k in ("dth", "th", "land_label", "loss", "loss_land")}


def test_landmark_term_enters_the_engine_between_the_gather_backward_and_the_cnn_backward():
    """Two identically seeded micro-steps (eval-mode model, no dropout, no DropPath, acc_step 3), weight 0 and weight w: what the
    weight changes in `dth` and `loss` is the fp64 formula on the engine's own `th` and `land_label` buffers, within the kernel test's
    bound plus one rounding (the difference of two fp32 results) plus whatever two weight-0 runs differ by (measured here)."""
    w, gs = 100.0, LM.f32c(1.0 / 3.0)
    r0, r0b, rw = _seam_run(0.0), _seam_run(0.0), _seam_run(w)
    noise_d, noise_l = float(np.abs(r0["dth"] - r0b["dth"]).max()), float(abs(r0["loss"][0] - r0b["loss"][0]))
    assert np.array_equal(r0["th"], rw["th"]) and np.array_equal(r0["land_label"], rw["land_label"]), "the forward does not see the weight"
    assert float(np.abs(rw["th"] - rw["land_label"]).max()) > 1.0, "teacher and branch disagree: the term is not trivially zero"
    ref = LM.oracle(rw["th"], rw["land_label"], LM.f32c(w), gs, r0["dth"], float(r0["loss"][0]))
    bnd = LM.bounds(ref, rw["th"].size // 2)
    e_d = np.abs((rw["dth"] - r0["dth"]) - ref["inc"])
    b_d = bnd["dtheta"] + LM.U * np.abs(rw["dth"]) + noise_d
    e_l = abs((rw["loss"][0] - r0["loss"][0]) - ref["term"])
    b_l = bnd["loss"] + LM.U * abs(rw["loss"][0]) + noise_l
    e_ll = abs(rw["loss_land"][0] - ref["loss_land"])
    print(f"[landmark seam] weight-0 run-to-run: dth {noise_d:.3e}, loss {noise_l:.3e}; worst |err| / bound: dth {float((e_d / b_d).max()):.3f}, "
          f"loss {e_l / b_l:.3f}, loss_land {e_ll / bnd['loss_land']:.3f}; loss_land {rw['loss_land'][0]:.6f}, term {ref['term']:.6f}")
    assert np.all(e_d <= b_d) and e_l <= b_l and e_ll <= bnd["loss_land"]
    assert r0["loss_land"][0] == rw["loss_land"][0], "loss_land is the unweighted mean"
    assert float(np.abs(ref["inc"]).max()) > 100 * float(b_d.max()), "the increment is far above what the bound lets through"


# ------------------------------------------------------------------------------------------------ 6. mode B against the reference
@pytest.mark.parametrize("weight", [0.0, 1.0, 1000.0])
def test_mode_b_against_the_reference_fixture(weight, monkeypatch):
    """`pre_land and keep_land` (train_largescale.py:815-843) with the landmark CNN on torch autograd (LAFS_FT_CNN=torch) and the
    teacher's labels taken from the fixture: theta, the gradients and their norms with the tolerances of the F13 test -- the same
    arithmetic plus a term linear in theta.  The fixture's batch of 2 is fed four times over (the engine takes multiples of 8): every
    mean, and so every gradient, is that of the batch of 2."""
    from lafs_cvpr2024_amd.finetune_engine import FinetuneEngine
    monkeypatch.setenv("LAFS_FT_CNN", "torch")
    fx = _fx()
    tag = f"w{weight:g}."
    m = _fixture_backbone(True)
    eng = FinetuneEngine(m, 8, acc_step=1, mixup_prob=0.0, device=DEV, landmark_teacher=_teacher(det_fill_random), keep_land=True)
    assert eng.cnn is None
    eng.set_landmark_labels(fx["land_label"].repeat(4, 1, 1))
    loss = float(eng.micro_step(fx["u8"].repeat(4, 1, 1, 1).to(DEV), fx["labels"].repeat(4).to(DEV), lam=1.0, land_weight=weight).item())
    th = eng.th.cpu()
    assert all(torch.equal(th[:2], th[2 * k:2 * k + 2]) for k in range(1, 4))
    torch.testing.assert_close(th[:2], fx["theta"], rtol=1e-3, atol=2e-2)
    # loss_land: theta is held to delta = atol + rtol |theta| <= 2e-2 + 1e-3 * 111 per value, the labels are the fixture's own, so each
    # squared difference moves by at most 2 |pred - label| delta + delta^2, and so does their mean; / 111^2
    delta = 2e-2 + 1e-3 * 111.0
    dmax = float((fx["theta"] - fx["land_label"]).abs().max())
    b_ll = (2 * dmax * delta + delta * delta) / 111.0 ** 2
    loss_land = float(eng.loss_land.item())
    ce_ref = float(fx["w0.loss"])
    print(f"[mode B, w={weight:g}] loss {loss:.5f} (reference {float(fx[tag + 'loss']):.5f}), loss_land {loss_land:.6f} (reference "
          f"{float(fx['loss_land']):.6f}, bound {b_ll:.2e})")
    assert abs(loss_land - float(fx["loss_land"])) <= b_ll
    assert abs(loss - float(fx[tag + "loss"])) <= 5e-3 * ce_ref + weight * b_ll     # (5e-3: the engine's loss against the oracle's, F10 / F13 tests)
    params = dict(m.named_parameters())
    errs = {k: rel_l2(_thin(params[k].grad, fx["rowstep." + k]), g) for k, g in sub(fx, tag + "g.").items()}
    errs.update({k: rel_l2(_thin(params[k].grad, fx["rowstep." + k]), g) for k, g in sub(fx, "g.").items()})
    assert len(errs) == 7
    gate_errors(f"mode B w={weight:g}", errs, GATE_F13)
    _norms_match(params, fx["gnorm_keys"], fx[tag + "gnorms"])


# ------------------------------------------------------------------------------------------------ 7. captured == eager
def test_captured_mode_b_steps_equal_the_eager_ones_and_a_new_weight_is_no_new_capture():
    """Four micro-steps at acc_step 2 with the weights 1000, 1000, 0.11, 0 (train-mode model, live dropout / DropPath): the captured
    engine holds the two graphs it holds without the feature, its losses equal the eager engine's to 1e-5 before the first update and
    within the eager engine's own run-to-run noise after it (the rule of test_captured_finetune_step_equals_the_eager_single_stream_step)."""
    from lafs_cvpr2024_amd.finetune_engine import FinetuneEngine
    B, C = 16, 3000
    weights = [1000.0, 1000.0, 0.11, 0.0]
    res = {}
    for mode in ("graph", "eager", "eager2"):
        torch.manual_seed(4)
        model = ViT_face_landmark_patch8(loss_type="CosFace", GPU_ID=None, num_class=C, image_size=112, patch_size=8, dim=128, depth=3,
                                         heads=2, mlp_dim=256, dropout=0.1, emb_dropout=0.1, with_land=True, drop_path_rate=0.1)
        det_fill_random(model.stn); det_fill_random(model.output_layer)
        model.train()
        eng = FinetuneEngine(model, B, acc_step=2, device=DEV, use_graph=(mode == "graph"), landmark_teacher=_teacher(), keep_land=True)
        g = torch.Generator(device=DEV).manual_seed(9)
        losses, lands = [], []
        for it, w in enumerate(weights):
            u8 = torch.randint(0, 256, (B, 3, 112, 112), device=DEV, dtype=torch.uint8, generator=g)
            y = torch.randint(0, C, (B,), device=DEV, generator=g)
            losses.append(float(eng.micro_step(u8, y, lam=(0.3 if it % 3 == 0 else 1.0), land_weight=w).item()))
            lands.append(float(eng.loss_land.item()))
            if it % 2 == 1:
                eng.optimizer_step(lr=1e-3, weight_decay=0.1)
        torch.cuda.synchronize()
        if mode == "graph":
            assert len(eng._graphs) == 2, "two captured variants, as without the landmark term: first / later micro-step of a window"
        res[mode] = dict(losses=losses, lands=lands)
    a, b, b2 = res["graph"], res["eager"], res["eager2"]
    noise = max(abs(x - y) / abs(y) for x, y in zip(b2["losses"] + b2["lands"], b["losses"] + b["lands"]))
    print("[mode B graph vs eager] losses", a["losses"], b["losses"], "loss_land", a["lands"], b["lands"], "eager run-to-run", noise)
    for key in ("losses", "lands"):
        for x, y in zip(a[key][:2], b[key][:2]):
            assert abs(x - y) < 1e-5 * abs(y), (key, a[key], b[key])
        for x, y in zip(a[key][2:], b[key][2:]):
            assert abs(x - y) < max(2e-3, 5 * noise) * abs(y), (key, a[key], b[key])
    # weight 1000 at acc_step 2 adds 500 loss_land to a cross-entropy that stays of one size over the four steps; weight 0 adds nothing
    assert a["losses"][0] - a["losses"][3] > 0.5 * 500.0 * a["lands"][0], "the replayed graph read the new weight"


# ------------------------------------------------------------------------------------------------ 8. mode A
def test_mode_a_against_the_reference_fixture():
    """`pre_land` alone (train_largescale.py:811-812): the backbone without a branch is fed the patches gathered at the teacher's
    landmarks (here the fixture's, through the hook): embedding, loss, trunk gradients and norms against the reference."""
    from lafs_cvpr2024_amd.finetune_engine import FinetuneEngine
    fx = _fx()
    m = _fixture_backbone(False)
    eng = FinetuneEngine(m, 8, acc_step=1, mixup_prob=0.0, device=DEV, landmark_teacher=_teacher(det_fill_random))
    eng.set_landmark_labels(fx["land_label"].repeat(4, 1, 1))
    loss = float(eng.micro_step(fx["u8"].repeat(4, 1, 1, 1).to(DEV), fx["labels"].repeat(4).to(DEV), lam=1.0).item())
    emb = eng.emb.cpu()
    assert all(torch.equal(emb[:2], emb[2 * k:2 * k + 2]) for k in range(1, 4))
    print(f"[mode A] loss {loss:.5f} (reference {float(fx['a.loss']):.5f}), embedding rel-L2 {rel_l2(emb[:2], fx['a.emb']):.2e}")
    assert rel_l2(emb[:2], fx["a.emb"]) < 2e-2
    assert abs(loss - float(fx["a.loss"])) <= 5e-3 * float(fx["a.loss"])
    params = dict(m.named_parameters())
    errs = {k: rel_l2(_thin(params[k].grad, fx["rowstep." + k]), g) for k, g in sub(fx, "a.g.").items()}
    assert len(errs) == 4
    gate_errors("mode A", errs, GATE_F13)
    _norms_match(params, fx["a.gnorm_keys"], fx["a.gnorms"])
    with pytest.raises(_lib.LafsHipError, match="before the micro-step is captured"):
        eng.set_landmark_labels(None)


def test_mode_a_feeds_the_patches_at_the_plan_s_landmarks_and_matches_the_module_path():
    """Without the hook: `img_in` is lafs_patch_gather_fwd at the frozen plan's theta, bit for bit; loss and the patch_to_embedding /
    loss.weight gradients equal the autograd module path fed the same patches (tolerances of
    test_finetune_engine_with_landmark_branch_matches_module_path)."""
    import torch.nn.functional as F
    from lafs_cvpr2024_amd.finetune_engine import FinetuneEngine
    from lafs_cvpr2024_amd.landmark_cnn import HipLandmarkCNN
    B, C = 8, 1000
    mk = lambda: ViT_face_landmark_patch8(loss_type="CosFace", GPU_ID=None, num_class=C, image_size=112, patch_size=8, dim=128, depth=2,
                                          heads=3, mlp_dim=256, dropout=0.0, emb_dropout=0.0, with_land=False, drop_path_rate=0.0)
    torch.manual_seed(6)
    u8 = torch.randint(0, 256, (B, 3, 112, 112), dtype=torch.uint8, device=DEV)
    labels = torch.tensor([3, 999, 17, 3, 500, 0, 42, 999], device=DEV)
    teacher = _teacher()
    m1 = mk(); m1.eval()
    eng = FinetuneEngine(m1, B, acc_step=1, device=DEV, landmark_teacher=teacher)
    loss1 = float(eng.micro_step(u8, labels, lam=1.0).item())
    t = HipLandmarkCNN(teacher, DEV)(eng.x)
    theta = torch.empty(B, 196, 2, device=DEV)
    call("lafs_landmark_theta", _p(t), B, 196, None, 0.0, None, 196, _p(theta))
    mosaic = torch.empty_like(eng.x)
    call("lafs_patch_gather_fwd", _p(eng.x), _p(theta), B, 112, 196, _p(mosaic))
    assert torch.equal(theta, eng.land_label) and torch.equal(mosaic, eng.img_in)
    assert not torch.equal(mosaic, eng.x) and float(theta.min()) == 0.0 and float(theta.max()) == 111.0
    keys = ("patch_to_embedding.weight", "loss.weight")
    g1 = {k: dict(m1.named_parameters())[k].grad.clone() for k in keys}
    m2 = mk(); m2.load_state_dict(m1.state_dict()); attach_arena(m2, DEV); m2.eval()
    logits, _ = m2(mosaic, labels)
    loss2 = F.cross_entropy(logits, labels)
    loss2.backward()
    bad = {k: rel_l2(g1[k], dict(m2.named_parameters())[k].grad) for k in keys}
    loss2 = loss2.detach()
    print("[mode A vs module path] loss", loss1, float(loss2), "gradient rel-L2", {k: f"{v:.2e}" for k, v in bad.items()})
    assert abs(loss1 - float(loss2)) < 5e-3 * abs(float(loss2)), (loss1, float(loss2))
    assert all(v < 5e-2 for v in bad.values()), bad


# ------------------------------------------------------------------------------------------------ 9. mode-A verification
def test_mode_a_verification_uses_the_teacher_s_plan():
    """A backbone without a branch, evaluated with the teacher, gives bit for bit the features of a with_land=True model that carries
    the teacher's CNN weights (the same plan, the same kernels); a backbone with its own branch ignores the teacher."""
    from lafs_cvpr2024_amd import verification as V
    cfg = dict(loss_type="None", GPU_ID=None, num_class=10, image_size=112, patch_size=8, dim=128, depth=2, heads=3, mlp_dim=256)
    teacher = _teacher()
    torch.manual_seed(4)
    m_a = ViT_face_landmark_patch8(with_land=False, **cfg)
    m_b = ViT_face_landmark_patch8(with_land=True, **cfg)
    m_b.load_state_dict(m_a.state_dict(), strict=False)
    m_b.stn.load_state_dict(teacher.stn.state_dict()); m_b.output_layer.load_state_dict(teacher.output_layer.state_dict())
    x = torch.randint(0, 256, (20, 3, 112, 112), dtype=torch.uint8, generator=torch.Generator().manual_seed(5))
    issame = np.arange(10) % 2 == 0
    feats = {}
    for name, model, t in (("a", m_a, teacher), ("b", m_b, None), ("b+t", m_b, _teacher(det_fill_random)), ("plain", m_a, None)):
        ev = V.VerificationEvaluator(model, 10, DEV, landmark_teacher=t)
        ev.keep_features = True
        ev(x, issame)
        feats[name] = ev.features.clone()
    assert torch.equal(feats["a"], feats["b"])
    assert torch.equal(feats["b+t"], feats["b"]), "mode B: nothing changes"
    assert not torch.equal(feats["plain"], feats["a"]), "without the teacher the backbone sees the plain 8 x 8 grid"
    # the IJB evaluator builds its plan through the same function
    sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "tools"))
    import make_synthetic_ijb as syn
    from lafs_cvpr2024_amd import ijb_evaluation as J
    imgs, lmk = syn.images(10), syn.dataset(10)["lmk"].astype(np.float32)
    ijb = {name: J.IJBEvaluator(model, 4, DEV, landmark_teacher=t).features(imgs, lmk).cpu()
           for name, model, t in (("a", m_a, teacher), ("b", m_b, None), ("plain", m_a, None))}
    assert torch.equal(ijb["a"], ijb["b"]) and not torch.equal(ijb["plain"], ijb["a"])
