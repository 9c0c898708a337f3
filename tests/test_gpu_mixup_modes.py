"""GPU tests of CutMix, pair / elem mixing and label smoothing on the fine-tune path: lafs_mix_normalize and
lafs_margin_softmax_ce_mix_bf16 against the batch-mode kernels (bit for bit where the new expressions reduce to the old ones), the
reference's parameter draws (tests/golden/f25_mixup_modes.npz) and the dense fp64 oracle (tests/mixup_oracle.py); FinetuneEngine with
the new options against the CPU oracle's autograd, captured against eager, and on the class-sharded head."""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

from conftest import gate_errors, load_golden, sub  # noqa: E402
import mixup_oracle as mo  # noqa: E402
from lafs_cvpr2024_amd import _lib  # noqa: E402
from lafs_cvpr2024_amd.face_pre_pro.ViT_face import ViT_face_landmark_patch8  # noqa: E402
from lafs_cvpr2024_amd.ops import _p, call  # noqa: E402

DEV = "cuda"
GATE_FT = 1.5e-2                                   # tests/test_gpu_finetune.py: the single micro-step (mixed or not) against the oracle
FX = load_golden("f25_mixup_modes")
NAMES = [str(n) for n in FX["names"]]


def rel_l2(a, b):
    a, b = a.detach().double().cpu(), b.detach().double().cpu()
    return ((a - b).norm() / (b.norm() + 1e-30)).item()


def table(lam, cut=None, box=None):
    """The device parameter table of lafs_mix_normalize / lafs_margin_softmax_ce_mix_bf16 (lafs_hip.h LAFS_MIX_*)."""
    lam = np.ascontiguousarray(lam, dtype=np.float32)
    B = lam.shape[0]
    t = np.zeros((B, _lib.MIX_WORDS), np.int32)
    t[:, _lib.MIX_LAM] = lam.view(np.int32)
    if cut is not None:
        t[:, _lib.MIX_CUT] = cut
        t[:, _lib.MIX_YL:] = box
    return torch.from_numpy(t).to(DEV)


def mix_normalize(u8, tab):
    out = torch.full(u8.shape, 7.0, device=DEV)
    call("lafs_mix_normalize", _p(u8), _p(out), u8.shape[0], u8.shape[-1], _p(tab))
    return out


def fixture_params(name):
    """The parameters the reference drew for this fixture case (the host class reproduces its RNG stream: test_mixup_modes_host.py)."""
    from lafs_cvpr2024_amd.util.mixup_my import Mixup
    ma, ca, mn, mx, prob, sw, eps, seed = (float(v) for v in sub(FX, "c." + name + ".")["cfg"])
    mix = Mixup(mixup_alpha=ma, cutmix_alpha=ca, cutmix_minmax=None if mn < 0 else (mn, mx), prob=prob, switch_prob=sw,
                mode=name.split("_")[0], label_smoothing=eps, num_classes=50)
    np.random.seed(int(seed))
    return mix.draw_params(8, (16, 16))


@pytest.mark.parametrize("name", NAMES)
def test_image_kernel_against_the_reference_draws_and_the_cpu_restatement(name):
    """lafs_mix_normalize under the parameters the reference drew for every fixture case (all three modes; mixup, CutMix, switching,
    min/max boxes; unmixed rows): pasted box pixels and passed-through rows are, bit for bit, what the kernel emits for the source row
    at lambda 1; blended rows meet the comparison of the F11 GPU test against the CPU restatement on x/255*2-1."""
    lam, cut, box = fixture_params(name)
    B, S = 8, 16
    g = torch.Generator().manual_seed(len(name))
    u8 = torch.randint(0, 256, (B, 3, S, S), dtype=torch.uint8, generator=g)
    plain = mix_normalize(u8.to(DEV), table(np.ones(B))).cpu()                 # every row at lambda 1
    torch.testing.assert_close(plain, u8.float() / 255 * 2 - 1, rtol=1e-5, atol=1e-6)     # (x * (2/255) - 1 on the device, possibly fused)
    out = mix_normalize(u8.to(DEV), table(lam, cut, box)).cpu()
    ref = mo.mix_images(plain, torch.from_numpy(lam), cut, box)
    n_exact = 0
    for b in range(B):
        if cut[b] or lam[b] == 1.0:
            assert torch.equal(out[b], ref[b]), (name, b)                           # the partner's / the row's own lambda-1 pixels, exactly
            n_exact += 1
            if cut[b]:
                yl, yh, xl, xh = box[b]
                assert torch.equal(out[b, :, yl:yh, xl:xh], plain[B - 1 - b, :, yl:yh, xl:xh])
                inside = torch.zeros(S, S, dtype=torch.bool); inside[yl:yh, xl:xh] = True
                assert torch.equal(out[b][:, ~inside], plain[b][:, ~inside])
        else:
            torch.testing.assert_close(out[b], ref[b], rtol=1e-5, atol=1e-6)
    if "_cutmix_" in name:
        assert n_exact == B


@pytest.mark.parametrize("lam", [0.3, 1.0, 0.0])
def test_image_kernel_with_a_uniform_blend_table_equals_the_batch_kernel(lam):
    B, S = 16, 112
    u8 = torch.randint(0, 256, (B, 3, S, S), dtype=torch.uint8, device=DEV)
    ref = torch.empty(B, 3, S, S, device=DEV)
    call("lafs_mixup_normalize", _p(u8), _p(ref), B, S, lam, None)
    assert torch.equal(mix_normalize(u8, table(np.full(B, lam))), ref)


def _cos_and_labels(B, C, seed):
    g = torch.Generator().manual_seed(seed)
    Cpad = (C + 127) // 128 * 128
    cos = (torch.rand(B, Cpad, generator=g) * 2 - 1)
    cos[:, C:] = 0
    y = torch.randint(0, C, (B,), generator=g)
    return cos, y, Cpad


def _mix_loss(cos, Cpad, B, C, y1, y2, lam_ptr, stride, eps, m, margin_type):
    dcos = torch.full((B, Cpad), 7.0, device=DEV, dtype=torch.bfloat16)
    loss, rows, part = torch.zeros(1, device=DEV), torch.empty(B, device=DEV), torch.empty(B * 48, device=DEV)
    call("lafs_margin_softmax_ce_mix_bf16", _p(cos), Cpad, B, C, _p(y1), _p(y2), _p(lam_ptr), stride, eps, 64.0, m, margin_type, 1.0,
         _p(dcos), Cpad, _p(loss), _p(rows), _p(part))
    return loss, rows, dcos


@pytest.mark.parametrize("margin_type,m,lam", [(0, 0.4, 0.3), (1, 0.5, 1.0), (1, 0.5, 0.3)])
@pytest.mark.parametrize("B,C", [(8, 1000), (32, 20533)])
def test_mix_loss_kernel_without_smoothing_equals_the_batch_kernel_bit_for_bit(margin_type, m, lam, B, C):
    """eps = 0 and one lambda on every row: the target expression off + (1 - eps) w reduces exactly to w, every reduction runs in the
    same order -- loss and bf16 gradient equal lafs_margin_softmax_ce_bf16's bit for bit, for both margin types; lambda read from a
    plain array and from the parameter table, partner implied and explicit.  ArcFace runs with lambda 1 (hard labels) and with 0.3, where
    both spikes are live.  Both entry points launch the same kernel pair when eps = 0, so this guards the lambda plumbing (scalar, one
    device word at stride 0, a word per row at stride 1 or LAFS_MIX_WORDS) and the dispatch on eps; the arithmetic itself is held against
    fp64 in tests/test_gpu_finetune.py (batch entries) and below (per-row entry)."""
    cos, y, Cpad = _cos_and_labels(B, C, 31 + B)
    cos = cos.to(DEV)
    y1 = y.to(DEV, torch.int32)
    y1[3] = y1[B - 4]                                                   # a row whose partner carries its own class
    y2 = y1.flip(0).contiguous()
    ref = torch.full((B, Cpad), 7.0, device=DEV, dtype=torch.bfloat16)
    loss_ref, rows_ref, part = torch.zeros(1, device=DEV), torch.empty(B, device=DEV), torch.empty(B * 32, device=DEV)
    call("lafs_margin_softmax_ce_bf16", _p(cos), Cpad, B, C, _p(y1), _p(y2), lam, None, 64.0, m, margin_type, 1.0, _p(ref), Cpad,
         _p(loss_ref), _p(rows_ref), _p(part))
    rows_ref = rows_ref.clone()
    lam_rows = torch.full((B,), lam, device=DEV)
    for y2_arg, ptr, stride in ((y2, lam_rows, 1), (None, table(np.full(B, lam)), _lib.MIX_WORDS)):
        loss, rows, dcos = _mix_loss(cos, Cpad, B, C, y1, y2_arg, ptr, stride, 0.0, m, margin_type)
        assert torch.equal(rows, rows_ref) and torch.equal(loss, loss_ref), (float(loss), float(loss_ref))
        assert torch.equal(dcos.view(torch.int16), ref.view(torch.int16))
    if margin_type == 1:                                                # smoothing has no meaning under ArcFace: refused, nothing launched
        with pytest.raises(_lib.LafsHipError, match="CosFace"):
            _mix_loss(cos, Cpad, B, C, y1, y2, lam_rows, 1, 0.1, m, margin_type)


@pytest.mark.parametrize("B,C", [(8, 50), (8, 1000), (16, 205990)])
def test_mix_loss_kernel_against_the_dense_fp64_oracle(B, C):
    """eps = 0.1, a lambda per row (1.0, 0.0 and rows with a1 == a2 among them), C = 50 / 1000 / 205 990 (not a multiple of the chunk
    width; 50 leaves most chunks short or empty): loss, per-row losses and the bf16 gradient against tests/mixup_oracle.py in fp64 on
    the same fp32 cosines, pad columns zeroed.  Bounds: those tests/test_gpu_finetune.py holds the bf16 kernel to (loss 1e-5
    relative, gradient 4e-3 relative L2 = the bf16 rounding of the output).  The off * sum_k z_k term does not need a wider loss
    bound: sum_k z_k is a fp32 sum of C terms of size <= s (1 + m) = 89.6, folded as ~C/4096 sequential adds per lane and a
    17-level tree, so its error is below (C/4096 + 17) 2^-24 sum|z| <= 68 * 6e-8 * 205990 * 89.6 = 75 at C = 205 990, and
    off = eps / C = 4.9e-7 scales that to 3.7e-5 -- against 1e-5 * loss = 7e-4 at this C's loss of ~70."""
    eps = 0.1
    cos, y, Cpad = _cos_and_labels(B, C, 77 + C)
    y[2] = y[B - 3]                                                     # a1 == a2 with a lambda strictly inside (0, 1)
    g = torch.Generator().manual_seed(C)
    lam = torch.rand(B, generator=g)
    lam[0], lam[1], lam[B - 1] = 1.0, 0.0, 1.0
    y1 = y.to(DEV, torch.int32)
    loss, rows, dcos = _mix_loss(cos.to(DEV), Cpad, B, C, y1, None, lam.to(DEV), 1, eps, 0.4, 0)
    ref_loss, ref_rows, ref_g = mo.loss_and_dcos(cos[:, :C], y, lam.double(), eps)
    e_loss = abs(float(loss) - float(ref_loss)) / abs(float(ref_loss))
    e_rows = float(((rows.cpu().double() - ref_rows).abs() / ref_rows.abs()).max())
    e_grad = rel_l2(dcos[:, :C].float(), ref_g)
    print(f"[mix loss vs fp64, C={C}] loss {float(loss):.6f} vs {float(ref_loss):.6f}: rel {e_loss:.2e}; worst row {e_rows:.2e}; gradient rel-L2 {e_grad:.2e}")
    assert e_loss < 1e-5, (float(loss), float(ref_loss))
    assert e_rows < 1e-5                                                # every row on its own: no row's error hides behind another's
    assert e_grad < 4e-3
    assert float(dcos[:, C:].float().abs().max()) == 0.0
    # eps > 0 really is in the result: the unsmoothed loss of the same rows is far outside the bound
    l0, _, _ = _mix_loss(cos.to(DEV), Cpad, B, C, y1, None, lam.to(DEV), 1, 0.0, 0.4, 0)
    assert abs(float(l0) - float(ref_loss)) / abs(float(ref_loss)) > 1e-3


def _small_model(C, with_loss=True):
    return ViT_face_landmark_patch8(loss_type="CosFace" if with_loss else "None", GPU_ID=None, num_class=C, image_size=112, patch_size=8,
                                    dim=128, depth=2, heads=3, mlp_dim=256, dropout=0.0, emb_dropout=0.0, with_land=False, drop_path_rate=0.0)


def _params(B, kind):
    """Explicit per-row parameters: CutMix rows, blended rows and untouched rows in one batch."""
    lam, cut, box = np.ones(B, np.float32), np.zeros(B, bool), np.zeros((B, 4), np.int32)
    if kind == "elem":                                                  # every row on its own
        cut[[0, 5]] = True
        box[0], box[5] = (10, 70, 24, 112), (0, 33, 5, 40)
        lam[[1, 2, 6]] = (0.3, 0.85, 0.55)
    else:                                                               # pair: rows b and B-1-b share everything
        for b, bx in ((0, (16, 80, 8, 72)), (2, (40, 112, 0, 50))):
            cut[[b, B - 1 - b]] = True
            box[b] = box[B - 1 - b] = bx
        lam[[1, B - 2]] = 0.4
    for b in np.nonzero(cut)[0]:
        lam[b] = 1.0 - (box[b, 1] - box[b, 0]) * (box[b, 3] - box[b, 2]) / (112.0 * 112.0)
    return lam, cut, box


@pytest.mark.parametrize("eps", [0.1, 0.0])
def test_engine_with_cutmix_elem_mode_and_smoothing_against_oracle(eps):
    """u8 batch -> per-row CutMix / blend -> Part-fViT -> CosFace on the (smoothed) dense target -> soft-target CE -> backward: the
    HIP engine with explicit per-row parameters against the CPU oracle's autograd; tolerances of
    test_finetune_micro_step_against_oracle."""
    from lafs_cvpr2024_amd.finetune_engine import FinetuneEngine
    from oracle import margin, partfvit
    torch.manual_seed(5)
    B, C = 8, 1000
    model = _small_model(C)
    P = {k: v.clone().requires_grad_(True) for k, v in model.state_dict().items()}
    u8 = torch.randint(0, 256, (B, 3, 112, 112), dtype=torch.uint8)
    labels = torch.tensor([3, 999, 17, 3, 500, 0, 42, 999])
    eng = FinetuneEngine(model, B, acc_step=1, device=DEV, cutmix_alpha=1.0, mix_mode="elem", label_smoothing=eps)
    assert eng.mix_rows
    lam, cut, box = _params(B, "elem")
    loss = eng.micro_step(u8.to(DEV), labels.to(DEV), mix=(lam, cut, box))
    cfg = partfvit.PartFViTConfig(patch_size=8, dim=128, depth=2, heads=3, mlp_dim=256, num_patches=196)
    x = mo.mix_images(u8.float() / 255 * 2 - 1, torch.from_numpy(lam), cut, box)
    torch.testing.assert_close(eng.x.cpu(), x, rtol=1e-5, atol=1e-6)
    tgt = mo.dense_target(labels, C, lam, eps, dtype=torch.float32)
    emb = partfvit.forward_embedding(P, x, cfg)
    ref = margin.soft_target_cross_entropy(margin.cosface_logits(emb, P["loss.weight"], tgt), tgt)
    ref.backward()
    print(f"[engine cutmix/elem eps={eps}] loss {float(loss.item()):.5f} oracle {ref.item():.5f}")
    assert abs(float(loss.item()) - float(ref)) / float(ref) < 5e-3, (float(loss.item()), float(ref))
    named = dict(model.named_parameters())
    keys = ("loss.weight", "patch_to_embedding.weight", "transformer.layers.0.0.fn.fn.to_qkv.weight", "transformer.layers.1.1.fn.fn.net.3.weight",
            "pos_embedding", "cls_token", "mlp_head.0.weight", "transformer.layers.0.1.fn.fn.net.0.bias")
    gate_errors(f"fine-tune micro step (cutmix, elem, eps {eps}) vs oracle", {k: rel_l2(named[k].grad, P[k].grad) for k in keys}, GATE_FT)


def test_captured_step_with_drawn_parameters_equals_the_eager_step():
    """Graph replay picks up each micro-step's parameter table: an accumulation window of three micro-steps whose parameters are
    DRAWN (elem mode, mixup and CutMix switching, prob 1: every micro-step another table), captured against eager under one seed.
    Bit for bit: the mixed images, every loss, the bf16 class gradient of each micro-step and the accumulated class-table gradient
    (GEMM outputs, fixed summation order).  The trunk's bias / LayerNorm / embedding gradients are summed with atomics in both forms
    (tests/test_gpu_finetune.py, deferred-gradient test): fp32 round-off."""
    from lafs_cvpr2024_amd.finetune_engine import FinetuneEngine
    B, C = 8, 3000
    res = {}
    for mode in ("graph", "eager"):
        torch.manual_seed(4)
        model = _small_model(C)
        model.train()
        eng = FinetuneEngine(model, B, acc_step=3, mixup_alpha=0.8, mixup_prob=1.0, device=DEV, use_graph=(mode == "graph"),
                             cutmix_alpha=1.0, mix_mode="elem", label_smoothing=0.1)
        g = torch.Generator(device=DEV).manual_seed(9)
        np.random.seed(2024)
        steps = []
        for it in range(3):
            u8 = torch.randint(0, 256, (B, 3, 112, 112), device=DEV, dtype=torch.uint8, generator=g)
            y = torch.randint(0, C, (B,), device=DEV, generator=g)
            loss = eng.micro_step(u8, y).clone()
            steps.append(dict(loss=loss, x=eng.x.clone(), dcos=eng.dcos.clone(), mix=tuple(a.copy() for a in eng._mix)))
        torch.cuda.synchronize()
        if mode == "graph":
            assert len(eng._graphs) == 2, "two captured variants: first / later micro-step of a window"
        res[mode] = dict(steps=steps, grads={k: p.grad.clone() for k, p in model.named_parameters() if p.grad is not None})
    a, b = res["graph"], res["eager"]
    tables = [np.concatenate([m.astype(np.float64).ravel() for m in s["mix"]]) for s in a["steps"]]
    assert not np.array_equal(tables[0], tables[1]) and not np.array_equal(tables[1], tables[2])     # the micro-steps do differ
    assert any(s["mix"][1].any() for s in a["steps"]) and any((~s["mix"][1] & (s["mix"][0] != 1)).any() for s in a["steps"])
    for sa, sb in zip(a["steps"], b["steps"]):
        assert all(np.array_equal(p, q) for p, q in zip(sa["mix"], sb["mix"]))
        assert torch.equal(sa["x"], sb["x"])
        assert torch.equal(sa["loss"], sb["loss"]), (float(sa["loss"]), float(sb["loss"]))
        assert torch.equal(sa["dcos"].view(torch.int16), sb["dcos"].view(torch.int16))
    assert torch.equal(a["grads"]["loss.weight"], b["grads"]["loss.weight"])
    for k, ga in a["grads"].items():
        assert float((ga - b["grads"][k]).abs().max()) <= 1e-6 * float(ga.abs().max()), k


def test_sharded_head_with_cutmix_and_pair_mode_matches_the_unsharded_soft_oracle():
    """FinetuneEngine(sharded_head=PartialFC, sample rate 1) with CutMix in pair mode: the shard kernels' per-row lambda carries the
    area-corrected lambdas; loss and gradients equal the unsharded CosFace(soft) + soft-target CE of the oracle on the same mixed
    batch.  Label smoothing on the sharded head, and with ArcFace, is refused."""
    from lafs_cvpr2024_amd.finetune_engine import FinetuneEngine
    from lafs_cvpr2024_amd.partial_fc import PartialFC
    from oracle import margin, partfvit
    B, C = 8, 512
    torch.manual_seed(8)
    bare = _small_model(C, with_loss=False)
    P = {k: v.clone().requires_grad_(True) for k, v in bare.state_dict().items()}
    u8 = torch.randint(0, 256, (B, 3, 112, 112), dtype=torch.uint8)
    labels = torch.randint(0, C, (B,))
    labels[1] = labels[B - 2]
    head = PartialFC(128, C, B, sample_rate=1.0, device=DEV)
    W = head.weight.detach().cpu().clone().requires_grad_(True)
    eng = FinetuneEngine(bare, B, acc_step=1, device=DEV, sharded_head=head, cutmix_alpha=1.0, mix_mode="pair")
    lam, cut, box = _params(B, "pair")
    loss = float(eng.micro_step(u8.to(DEV), labels.to(DEV), mix=(lam, cut, box)).item())
    cfg = partfvit.PartFViTConfig(patch_size=8, dim=128, depth=2, heads=3, mlp_dim=256, num_patches=196)
    x = mo.mix_images(u8.float() / 255 * 2 - 1, torch.from_numpy(lam), cut, box)
    tgt = mo.dense_target(labels, C, lam, 0.0, dtype=torch.float32)
    emb = partfvit.forward_embedding(P, x, cfg)
    ref = margin.soft_target_cross_entropy(margin.cosface_logits(emb, W, tgt), tgt)
    ref.backward()
    assert abs(loss - float(ref)) < 5e-3 * abs(float(ref)), (loss, float(ref))
    named = dict(bare.named_parameters())
    for k in ("patch_to_embedding.weight", "transformer.layers.0.0.fn.fn.to_qkv.weight", "transformer.layers.1.1.fn.fn.net.3.weight"):
        assert rel_l2(named[k].grad, P[k].grad) < 3e-2, k
    assert rel_l2(head.arena.view(head.arena.grad, "weight", (C, 128)), W.grad) < 3e-2
    with pytest.raises(_lib.LafsHipError, match="class-sharded head"):
        FinetuneEngine(bare, B, acc_step=1, device=DEV, sharded_head=head, label_smoothing=0.1)
    with pytest.raises(_lib.LafsHipError, match="ArcFace"):
        FinetuneEngine(_small_model(C), B, acc_step=1, device=DEV, margin_type=1, label_smoothing=0.1)


def test_default_engine_issues_the_launches_it_issued_before(monkeypatch):
    """Reference defaults (cutmix 0, mode batch, smoothing 0): the engine calls lafs_mixup_normalize and lafs_margin_softmax_ce_bf16
    and neither of the per-row entry points; with a per-row option it calls those instead."""
    from lafs_cvpr2024_amd import finetune_engine as fe
    B, C = 8, 1000
    seen = []
    real = fe.call
    monkeypatch.setattr(fe, "call", lambda name, *a: (seen.append(name), real(name, *a))[1])
    u8 = torch.randint(0, 256, (B, 3, 112, 112), dtype=torch.uint8, device=DEV)
    y = torch.randint(0, C, (B,), device=DEV)
    for kw, want, never in ((dict(), {"lafs_mixup_normalize", "lafs_margin_softmax_ce_bf16"}, {"lafs_mix_normalize", "lafs_margin_softmax_ce_mix_bf16"}),
                            (dict(label_smoothing=0.1), {"lafs_mix_normalize", "lafs_margin_softmax_ce_mix_bf16"},
                             {"lafs_mixup_normalize", "lafs_margin_softmax_ce_bf16"})):
        torch.manual_seed(3)
        eng = fe.FinetuneEngine(_small_model(C), B, acc_step=1, device=DEV, use_graph=False, **kw)
        assert eng.mix_rows == bool(kw) and (eng.mixer is None) == (not kw)
        seen.clear()
        eng.micro_step(u8, y, lam=0.3)
        names = set(seen)
        assert want <= names and not (never & names), sorted(names)
        assert eng.part_ws.numel() == B * (48 if kw else 32)
