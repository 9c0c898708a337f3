"""CPU: the AdaFace oracle of tests/adaface_cases.py judged on its own -- it equals an independent float64 autograd restatement, an
fp32 emulation of the kernels passes its bounds, eight seeded faults in that emulation fail them, and the conditions and caps the GPU
gates are stated under hold for the reference alone."""
import os
import sys

import pytest
import torch

sys.path.insert(0, os.path.dirname(__file__))
import adaface_cases as ac  # noqa: E402

_REF = {}


def _case(B, C, lam, explicit=False):
    key = (B, C, lam, explicit)
    if key not in _REF:
        case = ac.loss_case(B, C, lam, explicit)
        ref = ac.loss_ref(case["cos"][:, :C], case["y1"], case["y2"], case["lam"], case["rm"])
        _REF[key] = (case, ref)
    return _REF[key]


@pytest.mark.parametrize("lam", [1.0, 0.3])
@pytest.mark.parametrize("B,C", ac.MCE_SHAPES)
def test_sparse_oracle_equals_the_dense_autograd_restatement(B, C, lam):
    """Rows, mean and gradient of the sparse (y1, y2, lambda) oracle against float64 autograd through the dense one-hot, scatter
    formulation of the published forward: 1e-12 relative (gradient: of the row's largest element).  The oracle's flush of
    probabilities below 2^-126 -- the kernel's v_exp_f32 -- is the one intended difference: such elements are below 1e-36 in both."""
    for explicit in (False, True):
        case, ref = _case(B, C, lam, explicit)
        rows, mean, grad = ac.dense_restatement(case["cos"][:, :C], case["y1"], case["y2"], case["lam"], case["rm"])
        assert float(((ref["rows"][0] - rows).abs() / rows.abs()).max()) < 1e-12
        assert abs(float(ref["loss"][0]) - float(mean)) / abs(float(mean)) < 1e-12
        g = ref["grad"][0]
        flushed = (g == 0) & (grad != 0) & ~ref["zero"]
        assert float(grad[flushed].abs().max() if bool(flushed.any()) else 0.0) < 1e-36
        err = torch.where(flushed, torch.zeros_like(g), (g - grad).abs())
        assert float((err / grad.abs().max(1, keepdim=True).values).max()) < 1e-12
        assert bool((grad[ref["zero"]] == 0).all())


@pytest.mark.parametrize("lam", [1.0, 0.3])
@pytest.mark.parametrize("B,C", ac.MCE_SHAPES)
def test_conditions_and_caps_hold_for_the_reference_alone(B, C, lam):
    """What the GPU gates assume, shown without a kernel: no target within 1e-4 rad of a clip bound (the two planted ones lie far beyond
    theirs), no cosine within 1e-6 of a clamp threshold, every planted branch present, and the gradient's bound is 0 -- an exact bf16
    match is demanded -- at no fewer than 95 % of the elements."""
    for explicit in (False, True):
        case, ref = _case(B, C, lam, explicit)
        ac.check_conditions(case, ref, C)
        c = case["cos"][:, :C]
        assert int(((c > ac.HI) | (c < ac.LO)).sum()) >= 8                        # the planted +-0.9995 and +-1.0
        assert bool((ref["grad"][0][(c > ac.HI) | (c < ac.LO)] == 0).all())
        assert int(case["y1"][2]) == int(case["y2"][2])
        exact = float((ref["grad16"][1] == 0).double().mean())
        print(f"B={B} C={C} lam={lam} explicit={explicit}: bound 0 at {100 * exact:.2f} % of the elements")
        assert exact >= 0.95


@pytest.mark.parametrize("lam", [1.0, 0.3])
@pytest.mark.parametrize("B,C", ac.MCE_SHAPES[:2])
def test_fp32_emulation_passes_and_seeded_loss_faults_fail(B, C, lam):
    """The loss kernel emulated in fp32 torch arithmetic passes every gate; each of its seeded faults fails one: the clamp missing, a
    non-zero gradient at a clamped element, the margin weighted by y_k (shows on mixed rows), the theta clip dropped."""
    case, ref = _case(B, C, lam)
    args = (case["cos"][:, :C], case["y1"], case["y2"], case["lam"], case["rm"])
    loss, rows, grad = ac.emulate_loss(*args)
    ac.judge_loss("emulation", loss, rows, grad, ref, C)
    faults = ["no_clamp", "grad_at_clamp", "no_theta_clip"] + (["margin_times_y"] if lam < 1.0 else [])
    for fault in faults:
        loss, rows, grad = ac.emulate_loss(*args, fault=fault)
        with pytest.raises(AssertionError):
            ac.judge_loss(fault, loss, rows, grad, ref, C)


def test_fp32_emulation_passes_and_seeded_statistics_faults_fail():
    """lafs_adaface_margins emulated in fp32 passes its bounds on every case; g_ang with the wrong sign, the biased standard deviation
    and the state used before its update fail them (the last two on the cases that move the state)."""
    failed = {"g_ang_sign": 0, "biased_std": 0, "stale_state": 0}
    for name, inv, state, t, update in ac.stats_cases():
        ref = ac.margins_ref(inv, state, t, update=update)
        st, rm = ac.emulate_margins(inv, state, t, ac.H, ac.M, update)
        ac.judge_margins(name, st, rm, ref)
        assert bool(torch.isfinite(rm).all())
        if not update:
            assert torch.equal(st, torch.tensor(state, dtype=torch.float32))
        if name.startswith("spread") and "state=23.7" in name:
            k = ref["k"]
            assert float(k.min()) == -1.0 and float(k.max()) == 1.0
        for fault in failed:
            st, rm = ac.emulate_margins(inv, state, t, ac.H, ac.M, update, fault=fault)
            try:
                ac.judge_margins(f"{name} {fault}", st, rm, ref)
            except AssertionError:
                failed[fault] += 1
    print(failed)
    assert all(v > 0 for v in failed.values()), failed
    # every fault must fail the case made for it
    inv = ac.stats_cases()[0][1]
    for fault in failed:
        ref = ac.margins_ref(inv, ac.STATE0, 1.0, update=True)
        st, rm = ac.emulate_margins(inv, ac.STATE0, 1.0, ac.H, ac.M, True, fault=fault)
        with pytest.raises(AssertionError):
            ac.judge_margins(fault, st, rm, ref)


def test_gradient_through_the_margin_fails_the_head_gate():
    """No gradient flows through n_b, the statistics or k_b.  With k attached to the graph the embedding gradient moves by more than
    GATE_FT = 1.5e-2 relative L2, the gate the module and engine tests hold the gradients to.  (Targets at about 0.5 rad from their
    centres and norms inside the unclipped range of k: d z / d k = s m (sin theta_m - 1) vanishes at the pi / 2 of random centres.)"""
    g = torch.Generator().manual_seed(5)
    B, C, D = 8, 1000, 128
    xh = torch.nn.functional.normalize(torch.randn(B, D, generator=g, dtype=torch.float64), dim=1)
    x = xh * torch.linspace(19.0, 21.0, B, dtype=torch.float64)[:, None]
    w = torch.randn(C, D, generator=g, dtype=torch.float64)
    y = torch.randperm(C, generator=g)[:B]
    w[y] = 0.88 * xh + 0.47 * torch.nn.functional.normalize(torch.randn(B, D, generator=g, dtype=torch.float64), dim=1)
    lam = torch.ones(B, dtype=torch.float64)
    grads = []
    for attach in (False, True):
        xi = x.clone().requires_grad_(True)
        _, loss, _ = ac.head_ref(xi, w, y, y.flip(0), lam, (20.0, 1.0), 0.01, update=True, attach_k=attach)
        loss.backward()
        grads.append(xi.grad)
    rel = float((grads[1] - grads[0]).norm() / grads[0].norm())
    print(f"gradient through k_b moves d loss / d x by {rel:.3f} relative L2")
    assert rel > 1.5e-2
