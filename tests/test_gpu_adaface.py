"""GPU: the AdaFace head against the fp64 oracle of tests/adaface_cases.py -- lafs_adaface_margins and lafs_margin_softmax_ce_ada_bf16
element by element inside guards, the AdaFace module, and margin_type 2 of FinetuneEngine (oracle step, state under hipGraph replay,
checkpoint round trip, refusals).  Worst error / bound per case: pytest -s."""
import os
import sys

import pytest
import torch

sys.path.insert(0, os.path.dirname(__file__))
pytestmark = pytest.mark.gpu

import adaface_cases as ac  # noqa: E402
from conftest import gate_errors  # noqa: E402
from lafs_cvpr2024_amd import _lib  # noqa: E402
from lafs_cvpr2024_amd.face_pre_pro.ViT_face import AdaFace, ViT_face_landmark_patch8  # noqa: E402
from lafs_cvpr2024_amd.ops import _p, call  # noqa: E402

DEV = "cuda"
GATE_FT = 1.5e-2                                     # the project's gradient gate of this test family (tests/test_gpu_finetune.py)
f32 = torch.float32
_REF = {}


def rel_l2(a, b):
    a, b = a.detach().double().cpu(), b.detach().double().cpu()
    return ((a - b).norm() / (b.norm() + 1e-30)).item()


# ------------------------------------------------------------------------------------------------ lafs_adaface_margins
@pytest.mark.parametrize("B", [2, 8, 64, 200, 1024])
def test_margins_kernel_against_fp64(B):
    """Statistics, state and margins per element inside the bounds propagated from the fp32 two-pass arithmetic, for norms N(20, 5), all
    equal (std 0 with t_alpha 1: k stays finite), outside both clips and a spread that saturates k, from the initial and an arbitrary
    state, update 1 and 0 (0: the state's bytes unchanged); guard words round both outputs; the same bits on a second run."""
    worst = 0.0
    for name, inv, state, t, update in [c for c in ac.stats_cases() if f" B={B} " in c[0]]:
        ref = ac.margins_ref(inv, state, t, update=update)
        inv_d = inv.to(DEV)
        outs = []
        for _ in range(2):
            st, rm = ac.Guarded(2, f32, DEV), ac.Guarded(2 * B, f32, DEV, fill=float("nan"))
            st.v.copy_(torch.tensor(state, dtype=f32))
            before = st.v.clone()
            call("lafs_adaface_margins", _p(inv_d), B, _p(st.v), t, ac.H, ac.M, int(update), _p(rm.v))
            torch.cuda.synchronize()
            st.intact(name + " state"); rm.intact(name + " row_margin")
            if not update:
                assert torch.equal(st.v.view(torch.int32), before.view(torch.int32)), "update = 0 must not write the state"
            outs.append((st.v.clone(), rm.v.clone().view(B, 2)))
        assert torch.equal(outs[0][0], outs[1][0]) and torch.equal(outs[0][1], outs[1][1]), "not the same bits run to run"
        worst = max(worst, ac.judge_margins(name, outs[0][0], outs[0][1], ref))
    print(f"[adaface margins] B={B}: worst error / bound {worst:.3f}")


def test_margins_kernel_refuses_a_single_row():
    inv, st, rm = torch.ones(1, device=DEV), torch.tensor([20.0, 100.0], device=DEV), torch.zeros(1, 2, device=DEV)
    with pytest.raises(_lib.LafsHipError, match="at least two rows"):
        call("lafs_adaface_margins", _p(inv), 1, _p(st), 0.01, ac.H, ac.M, 1, _p(rm))
    assert st.tolist() == [20.0, 100.0]


# ------------------------------------------------------------------------------------------------ lafs_margin_softmax_ce_ada_bf16
def _loss_case(B, C, lam, explicit):
    key = (B, C, lam, explicit)
    if key not in _REF:
        case = ac.loss_case(B, C, lam, explicit)
        ref = ac.loss_ref(case["cos"][:, :C], case["y1"], case["y2"], case["lam"], case["rm"])
        ac.check_conditions(case, ref, C)
        _REF[key] = (case, ref)
    return _REF[key]


def _run_ada(case, B, C, y2, lam_ptr, stride):
    Cpad = case["Cpad"]
    cos, y1, rm = case["cos"].to(DEV), case["y1"].to(DEV, torch.int32), case["rm"].to(DEV)
    cos0 = cos.clone()
    dcos = torch.full((B, Cpad), 7.0, device=DEV, dtype=torch.bfloat16)
    loss, rows, part = ac.Guarded(1, f32, DEV), ac.Guarded(B, f32, DEV), ac.Guarded(B * 32, f32, DEV)
    call("lafs_margin_softmax_ce_ada_bf16", _p(cos), Cpad, B, C, _p(y1), _p(y2), _p(lam_ptr), stride, _p(rm), ac.S, 1.0, _p(dcos), Cpad,
         _p(loss.v), _p(rows.v), _p(part.v))
    torch.cuda.synchronize()
    for name, gd in (("loss", loss), ("row losses", rows), ("partials", part)):
        gd.intact(name)
    assert torch.equal(cos, cos0), "cos is read-only"
    return loss.v, rows.v, dcos


@pytest.mark.parametrize("lam", [1.0, 0.3])
@pytest.mark.parametrize("B,C", ac.MCE_SHAPES)
def test_ada_loss_kernel_against_fp64(B, C, lam):
    """Mean loss and every row loss within 1e-5 relative; the bf16 gradient element by element inside fp64_bounds.flip of the derived fp32
    error; exactly 0 at every clamped or clipped element and in the pad columns; the bound is 0 at >= 95 % of the elements.  The lambda
    arrives at stride 0 (one device word) and at stride 1, the partner implied (y2 NULL) and explicit; one row has y1 == y2, rows 0, 1, 3, 4
    carry k = +1, -1, 0, +1, and the clamp / clip branches are planted (adaface_cases.loss_case)."""
    for explicit in (False, True):
        case, ref = _loss_case(B, C, lam, explicit)
        y2 = case["y2"].to(DEV, torch.int32) if explicit else None
        for stride in (0, 1):
            lam_ptr = case["lam"][:1].to(DEV) if stride == 0 else case["lam"].to(DEV)
            loss, rows, dcos = _run_ada(case, B, C, y2, lam_ptr, stride)
            ratio, exact = ac.judge_loss(f"[ada loss] B={B} C={C} lam={lam} y2={'explicit' if explicit else 'NULL'} stride={stride}",
                                         loss, rows, dcos, ref, C)
    # the parameter table's stride reads the same words
    tab = torch.zeros(B, _lib.MIX_WORDS, device=DEV, dtype=f32)
    tab[:, _lib.MIX_LAM] = case["lam"].to(DEV)
    loss_t, rows_t, dcos_t = _run_ada(case, B, C, y2, tab, _lib.MIX_WORDS)
    assert torch.equal(loss_t, loss) and torch.equal(rows_t, rows) and torch.equal(dcos_t, dcos)


@pytest.mark.parametrize("B,C", ac.MCE_SHAPES)
def test_ada_loss_with_a_constant_margin_equals_cosface(B, C):
    """Margins (0, m) on every row, lambda 1, no clamped element: z = s (cos(acos c) - m), CosFace's logits up to the round trip through
    acosf / cosf -- the loss equals lafs_margin_softmax_ce_bf16 type 0 on the same inputs to 1e-5."""
    g = torch.Generator().manual_seed(77 + C)
    Cpad = (C + 127) // 128 * 128
    cos = ((torch.rand(B, Cpad, generator=g) * 2 - 1) * 0.99).to(DEV)
    cos[:, C:] = 0
    y1 = torch.randint(0, C, (B,), generator=g).to(DEV, torch.int32)
    rm = torch.tensor([0.0, ac.M], dtype=f32).repeat(B, 1).to(DEV)
    lam = torch.ones(1, device=DEV)
    out = {}
    for name in ("ada", "cos"):
        dcos = torch.full((B, Cpad), 7.0, device=DEV, dtype=torch.bfloat16)
        loss, rows, part = torch.zeros(1, device=DEV), torch.empty(B, device=DEV), torch.empty(B * 32, device=DEV)
        if name == "ada":
            call("lafs_margin_softmax_ce_ada_bf16", _p(cos), Cpad, B, C, _p(y1), None, _p(lam), 0, _p(rm), ac.S, 1.0, _p(dcos), Cpad, _p(loss),
                 _p(rows), _p(part))
        else:
            call("lafs_margin_softmax_ce_bf16", _p(cos), Cpad, B, C, _p(y1), None, 1.0, _p(lam), ac.S, ac.M, 0, 1.0, _p(dcos), Cpad, _p(loss),
                 _p(rows), _p(part))
        out[name] = (float(loss), rows.clone(), dcos.clone())
    print(f"[ada vs cosface] B={B} C={C}: loss {out['ada'][0]:.6f} vs {out['cos'][0]:.6f}")
    assert abs(out["ada"][0] - out["cos"][0]) < 1e-5 * abs(out["cos"][0])
    assert float(((out["ada"][1] - out["cos"][1]).abs() / out["cos"][1].abs()).max()) < 1e-5


def test_ada_loss_refusals():
    B, C, Cpad = 8, 50, 128
    cos, dcos = torch.zeros(B, Cpad, device=DEV), torch.zeros(B, Cpad, device=DEV, dtype=torch.bfloat16)
    y1, lam, rm = torch.zeros(B, device=DEV, dtype=torch.int32), torch.ones(B, device=DEV), torch.zeros(B, 2, device=DEV)
    loss, rows, part = torch.zeros(1, device=DEV), torch.empty(B, device=DEV), torch.empty(B * 32, device=DEV)
    for bad in (dict(rm=None), dict(lam=None), dict(stride=-1)):
        with pytest.raises(_lib.LafsHipError):
            call("lafs_margin_softmax_ce_ada_bf16", _p(cos), Cpad, B, C, _p(y1), None, _p(bad.get("lam", lam)), bad.get("stride", 1),
                 _p(bad.get("rm", rm)), ac.S, 1.0, _p(dcos), Cpad, _p(loss), _p(rows), _p(part))
    # the fixed-margin entries keep refusing the new type
    for entry in ("lafs_margin_softmax_ce_bf16",):
        with pytest.raises(_lib.LafsHipError, match="margin_type"):
            call(entry, _p(cos), Cpad, B, C, _p(y1), None, 1.0, None, ac.S, ac.M, 2, 1.0, _p(dcos), Cpad, _p(loss), _p(rows), _p(part))
    with pytest.raises(_lib.LafsHipError, match="margin_type"):
        call("lafs_margin_softmax_ce_mix_bf16", _p(cos), Cpad, B, C, _p(y1), None, _p(lam), 1, 0.0, ac.S, ac.M, 2, 1.0, _p(dcos), Cpad, _p(loss),
             _p(rows), _p(part))
    with pytest.raises(_lib.LafsHipError, match="margin_type"):
        call("lafs_margin_softmax_ce", _p(cos), Cpad, B, C, _p(y1), _p(y1), 1.0, ac.S, ac.M, 2, 1.0, _p(loss), _p(rows))
    with pytest.raises(_lib.LafsHipError, match="margin_type"):
        call("lafs_shard_margin_rowmax", _p(cos), Cpad, B, C, _p(y1), None, None, ac.S, ac.M, 2, _p(rows))


# ------------------------------------------------------------------------------------------------ the module
def test_adaface_module_against_the_oracle():
    """AdaFace.forward at B = 8, C = 1000, D = 128: logits and the input / weight gradients against the fp64 head (gates: the module
    figures of test_f10_cosface_hard_and_soft -- 1e-2 on the logits, 3e-2 on the gradients, the bf16 operands of the cosine GEMM), for an
    index vector and for a dense soft target; the buffers follow the fp64 EMA in training mode and stand still in eval mode."""
    g = torch.Generator().manual_seed(21)
    B, C, D = 8, 1000, 128
    head = AdaFace(D, C, None, t_alpha=1.0).to(DEV)
    x0 = torch.randn(B, D, generator=g) * torch.linspace(0.6, 2.5, B)[:, None]
    y = torch.randint(0, C, (B,), generator=g)
    probe = torch.randn(B, C, generator=g)
    for lam_v in (1.0, 0.3):
        lam = torch.full((B,), lam_v, dtype=torch.float64)
        head.train()
        head.batch_mean.fill_(20.0); head.batch_std.fill_(100.0)
        x = x0.clone().to(DEV).requires_grad_(True)
        head.weight.grad = None
        if lam_v == 1.0:
            label = y.to(DEV)
        else:
            label = torch.zeros(B, C).scatter_add_(1, y.view(-1, 1), lam.float().view(-1, 1))
            label = label.scatter_add_(1, y.flip(0).view(-1, 1), (1 - lam.float()).view(-1, 1)).to(DEV)
        out = head(x, label)
        (out * probe.to(DEV)).sum().backward()
        xr = x0.double().requires_grad_(True)
        wr = head.weight.detach().cpu().double().requires_grad_(True)
        z, _, state = ac.head_ref(xr, wr, y, y.flip(0), lam, ac.STATE0, 1.0, update=True)
        (z * probe.double()).sum().backward()
        errs = {"logits": rel_l2(out, z), "d input": rel_l2(x.grad, xr.grad), "d weight": rel_l2(head.weight.grad, wr.grad)}
        print(f"[adaface module] lam={lam_v}: " + ", ".join(f"{k} {v:.2e}" for k, v in errs.items()))
        assert errs["logits"] < 1e-2 and errs["d input"] < 3e-2 and errs["d weight"] < 3e-2, errs
        sd = head.state_dict()
        assert abs(float(sd["batch_mean"]) - state[0]) < 1e-4 * state[0] and abs(float(sd["batch_std"]) - state[1]) < 1e-4 * state[1]
    head.eval()
    before = (head.batch_mean.clone(), head.batch_std.clone())
    with torch.no_grad():
        head(x0.to(DEV), y.to(DEV))
    assert torch.equal(head.batch_mean, before[0]) and torch.equal(head.batch_std, before[1])


# ------------------------------------------------------------------------------------------------ the engine
def _model(C=1000, seed=9):
    torch.manual_seed(seed)
    model = ViT_face_landmark_patch8(loss_type="AdaFace", GPU_ID=None, num_class=C, image_size=112, patch_size=8, dim=128, depth=2, heads=3,
                                     mlp_dim=256, dropout=0.0, emb_dropout=0.0, with_land=False, drop_path_rate=0.0)
    with torch.no_grad():                              # a freshly initialised LayerNorm head gives every row the norm sqrt(dim): spread them
        model.mlp_head[0].weight.uniform_(0.5, 1.5)
        model.mlp_head[0].bias.normal_(0.0, 0.3)
    return model


@pytest.mark.parametrize("lam", [1.0, 0.3])
def test_finetune_engine_adaface_matches_oracle(lam):
    """margin_type 2 with ada_t_alpha = 1 (the margins vary strongly over the batch): one micro-step against autograd through
    oracle.partfvit.forward_embedding and the cases module's head.  Loss within 5e-3, gradients under GATE_FT."""
    from lafs_cvpr2024_amd.finetune_engine import FinetuneEngine
    from oracle import margin, partfvit
    B, C = 8, 1000
    model = _model(C)
    P = {k: v.clone().requires_grad_(True) for k, v in model.state_dict().items() if v.is_floating_point() and "batch_" not in k}
    u8 = torch.randint(0, 256, (B, 3, 112, 112), dtype=torch.uint8)
    labels = torch.tensor([3, 999, 17, 3, 500, 0, 42, 999])
    eng = FinetuneEngine(model, B, acc_step=1, s=64.0, m=0.4, margin_type=2, ada_t_alpha=1.0, device=DEV)
    loss = eng.micro_step(u8.to(DEV), labels.to(DEV), lam=lam)
    cfg = partfvit.PartFViTConfig(patch_size=8, dim=128, depth=2, heads=3, mlp_dim=256, num_patches=196)
    x, _ = margin.mixup_batch(u8.float() / 255 * 2 - 1, labels, C, lam)
    emb = partfvit.forward_embedding(P, x, cfg)
    _, ref, state = ac.head_ref(emb, P["loss.weight"], labels, labels.flip(0), torch.full((B,), lam), ac.STATE0, 1.0, update=True)
    ref.backward()
    ref = float(ref.detach())
    print(f"[adaface engine] lam={lam}: loss {float(loss.item()):.5f} vs {ref:.5f}; state {eng.ada_state.tolist()} vs {state}; "
          f"margins g_ang {eng.row_margin[:, 0].min().item():.3f} .. {eng.row_margin[:, 0].max().item():.3f}")
    assert abs(float(loss.item()) - ref) / ref < 5e-3, (float(loss.item()), ref)
    assert float(eng.row_margin[:, 0].max() - eng.row_margin[:, 0].min()) > 0.1, "the margins of this batch should vary strongly"
    named = dict(model.named_parameters())
    gate_errors(f"AdaFace micro step vs oracle, lam={lam}",
                {k: rel_l2(named[k].grad, P[k].grad) for k in ("loss.weight", "patch_to_embedding.weight", "transformer.layers.1.1.fn.fn.net.3.weight")},
                GATE_FT)


def test_adaface_state_counts_one_update_per_micro_step_graph_on_and_off(tmp_path):
    """ada_t_alpha = 0.01, three micro-steps + optimizer steps, captured and eager: the warm-up run and the capture leave no update behind
    -- the state is the same bits in both, equals three fp64 EMA updates of the norms of eng.emb inside the statistics bound, is what
    state_dict() holds, and a second engine built from the saved state dict continues identically."""
    from lafs_cvpr2024_amd.finetune_engine import FinetuneEngine
    B, C = 8, 1000
    g = torch.Generator().manual_seed(13)
    data = [(torch.randint(0, 256, (B, 3, 112, 112), dtype=torch.uint8, generator=g).to(DEV), torch.randint(0, C, (B,), generator=g).to(DEV))
            for _ in range(4)]
    res = {}
    for use_graph in (True, False):
        model = _model(C)
        model.train()
        eng = FinetuneEngine(model, B, acc_step=1, margin_type=2, ada_t_alpha=0.01, device=DEV, use_graph=use_graph)
        state, bound = torch.tensor(ac.STATE0, dtype=torch.float64), torch.zeros(2, dtype=torch.float64)
        for u8, y in data[:3]:
            eng.micro_step(u8, y, lam=1.0)
            inv = (1 / eng.emb.detach().float().norm(dim=1).clamp_min(1e-12)).cpu()      # (fp32 norms of the embedding the head saw)
            r = ac.margins_ref(inv, (float(state[0]), float(state[1])), ac.T_ALPHA, update=True)
            state, bound = r["state"][0], 0.99 * bound + r["state"][1] + 0.01 * 32 * ac.U * r["stats"][0]      # (+ lafs_l2norm_fwd's norm against torch's: fp64_bounds.l2norm_fwd's depth)
            eng.optimizer_step(lr=1e-3, weight_decay=0.1)
        torch.cuda.synchronize()
        if use_graph:
            assert eng._warm and len(eng._graphs) == 1
        got = eng.ada_state.double().cpu()
        print(f"[adaface state] graph={use_graph}: {got.tolist()} vs fp64 {state.tolist()} (bound {bound.tolist()})")
        assert bool(((got - state).abs() <= bound + 2 * ac.U * state.abs()).all()), (got, state, bound)
        sd = model.state_dict()
        assert float(sd["loss.batch_mean"]) == float(got[0]) and float(sd["loss.batch_std"]) == float(got[1])
        res[use_graph] = (eng.ada_state.clone(), eng, model)
    assert torch.equal(res[True][0].view(torch.int32), res[False][0].view(torch.int32)), (res[True][0], res[False][0])
    # ---- checkpoint round trip: a second engine from the saved state dict takes the same fourth micro-step
    _, eng, model = res[False]
    path = str(tmp_path / "ada.pth")
    torch.save(model.state_dict(), path)
    model2 = _model(C, seed=1)
    model2.load_state_dict(torch.load(path, map_location="cpu"))
    model2.train()
    eng2 = FinetuneEngine(model2, B, acc_step=1, margin_type=2, ada_t_alpha=0.01, device=DEV, use_graph=False)
    assert torch.equal(eng2.ada_state, eng.ada_state)
    l1 = float(eng.micro_step(*data[3], lam=1.0).item())
    l2 = float(eng2.micro_step(*data[3], lam=1.0).item())
    assert l1 == l2 and torch.equal(eng2.ada_state, eng.ada_state), (l1, l2, eng.ada_state, eng2.ada_state)
    assert float(model2.state_dict()["loss.batch_mean"]) == float(eng2.ada_state[0])
    # eval mode reads the state and does not move it
    model2.eval()
    before = eng2.ada_state.clone()
    eng2.micro_step(*data[0], lam=1.0)
    torch.cuda.synchronize()
    assert torch.equal(eng2.ada_state, before)


def test_adaface_engine_refusals():
    from lafs_cvpr2024_amd.finetune_engine import FinetuneEngine
    from lafs_cvpr2024_amd.partial_fc import PartialFC
    with pytest.raises(_lib.LafsHipError, match="margin_type 0 .CosFace. or 1 .ArcFace."):
        PartialFC(128, 1000, 8, margin_type=2, device=DEV)
    head = PartialFC(128, 1000, 8, device=DEV)
    with pytest.raises(_lib.LafsHipError, match="dense head"):
        FinetuneEngine(_model(), 8, margin_type=2, sharded_head=head, device=DEV)
    with pytest.raises(_lib.LafsHipError, match="label smoothing"):
        FinetuneEngine(_model(), 8, margin_type=2, label_smoothing=0.1, device=DEV)
    cos_model = ViT_face_landmark_patch8(loss_type="CosFace", GPU_ID=None, num_class=1000, image_size=112, patch_size=8, dim=128, depth=2,
                                         heads=3, mlp_dim=256, with_land=False)
    with pytest.raises(_lib.LafsHipError, match="loss_type='AdaFace'"):
        FinetuneEngine(cos_model, 8, margin_type=2, device=DEV)
    with pytest.raises(_lib.LafsHipError, match="loss_type='AdaFace'"):
        FinetuneEngine(_model(), 8, margin_type=0, device=DEV)
