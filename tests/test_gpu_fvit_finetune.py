"""fViT (ViTs_face_overlap) in FinetuneEngine: the micro-step against an fp32 CPU restatement, against the autograd module path, the
captured step against the eager one, and the class-sharded head.

The CPU yardstick (`cpu_features` / `case`) restates the step in fp32: F.unfold(12, stride 8, padding 4) -> patch_to_embedding -> cls + position rows
-> oracle.partfvit.transformer (fViT uses the same Transformer class and key names) -> F.batch_norm on the cls rows ->
oracle.margin's mixup / CosFace / soft-target CE; autograd gives the gradients.  Gates are relative L2 per tensor, 2x the worst value
observed on MI355X (DESIGN.md section 2 has the table); the yardstick is always the CPU result, never this build's own output.
                                                     observed   gate
  loss (relative), lam 1.0 / 0.3                     9.9e-4     2.0e-3    (6.0e-4 / 9.9e-4)
  parameter gradients (9 tensors), lam 1.0 / 0.3     4.3e-2     8.7e-2    (2.8e-2 patch_to_embedding.bias / 4.3e-2 cls_token)
  last block's fc2 bias gradient (see below)         1.3e-2     2.6e-2    (7.5e-3 / 1.3e-2)
  running_mean / running_var                         3.2e-3     6.3e-3    (running_var 7.8e-6)
At lam 1.0 the gradients sit where F26's do (2.8e-2 observed there); the blend of two noise images at lam 0.3 has less contrast, the
cls rows of the batch lie closer together and BatchNorm amplifies the bf16 error of the trunk more.

One tensor has no relative error (tests/test_gpu_fvit.py has the derivation): in training mode BatchNorm's input gradient sums to zero
per column, so the gradient of the LAST block's fc2 bias vanishes identically, whatever the head.  The test first checks on the CPU
numbers that it does (norm below 1e-4 of the neighbouring to_out bias gradient's), then holds this build's value as an absolute error
over that neighbour's norm.  It is the only tensor left out of the relative gates.

The backbone weights are the F26 fixture's (tests/fvit_cases.py), not the constructor's: with cls_token / pos_embedding ~ N(0, 1) and
noise images the cls rows of a batch differ by ~1e-3 of their size, the batch variance is ~0, BatchNorm multiplies the gradient by
eps ** -0.5, and the "vanishing" sum keeps an fp32 residue of 1e-2 of its neighbour on the CPU itself (measured: 1.3e-2 / 2.0e-2 at
lam 1.0 / 0.3) -- no yardstick for anything.  With the fixture's trained-scale weights the CPU residue is 1.6e-6 / 4.2e-6.
"""
import pytest
import torch
import torch.nn.functional as F

pytestmark = pytest.mark.gpu

from conftest import gate_errors, sub  # noqa: E402
from fvit_cases import FVIT_CFG, load_fvit  # noqa: E402
from lafs_cvpr2024_amd.face_pre_pro.ViT_face import ViTs_face_overlap  # noqa: E402
from lafs_cvpr2024_amd.vision_transformer import attach_arena  # noqa: E402

DEV = "cuda"
B, C = 8, 1000
GATE_LOSS, GATE_GRAD, GATE_BN, GATE_ZERO_SUM = 2.0e-3, 8.7e-2, 6.3e-3, 2.6e-2
ZERO_SUM, ZERO_SUM_SCALE = "transformer.layers.1.1.fn.fn.net.3.bias", "transformer.layers.1.0.fn.fn.to_out.0.bias"
KEYS = ("loss.weight", "patch_to_embedding.weight", "patch_to_embedding.bias", "pos_embedding", "cls_token", "mlp_head.0.weight",
        "mlp_head.0.bias", "transformer.layers.0.0.fn.fn.to_qkv.weight", "transformer.layers.0.1.fn.fn.net.3.weight")


def rel_l2(a, b):
    a, b = a.detach().double().cpu(), b.detach().double().cpu()
    return ((a - b).norm() / (b.norm() + 1e-30)).item()


_FX = {}


def fvit(loss_type="CosFace", num_class=C, p=0.0):
    """The small model with the F26 fixture's backbone weights; `loss.weight` keeps the constructor's (seeded) xavier draw."""
    if not _FX:
        _FX.update({k: (v.float() if v.dtype.is_floating_point else v) for k, v in sub(load_fvit(), "p.").items()})
    m = ViTs_face_overlap(pad=4, **{**FVIT_CFG, "loss_type": loss_type, "num_class": num_class, "dropout": p, "emb_dropout": p},
                          drop_path_rate=p)
    missing = m.load_state_dict(_FX, strict=False)
    assert not missing.unexpected_keys and set(missing.missing_keys) <= {"loss.weight"}
    return m


def nbt(model):
    return int(model.state_dict()["mlp_head.0.num_batches_tracked"])


# ------------------------------------------------------------------------------------------------ the CPU yardstick
def cpu_features(P, x, rm, rv, training):
    """fp32 restatement of ViTs_face_overlap.forward_features (x already scaled); rm / rv are updated in place in training mode."""
    from oracle import partfvit
    cfg = partfvit.PartFViTConfig(patch_size=8, dim=FVIT_CFG["dim"], depth=FVIT_CFG["depth"], heads=FVIT_CFG["heads"],
                                  mlp_dim=FVIT_CFG["mlp_dim"], num_patches=196)
    t = F.linear(F.unfold(x, 12, stride=8, padding=4).transpose(1, 2), P["patch_to_embedding.weight"], P["patch_to_embedding.bias"])
    n = t.shape[1]
    t = torch.cat((P["cls_token"].expand(x.shape[0], -1, -1), t), dim=1) + P["pos_embedding"][:, :n + 1]
    t = partfvit.transformer(P, t, cfg)
    return F.batch_norm(t[:, 0], rm, rv, P["mlp_head.0.weight"], P["mlp_head.0.bias"], training, 0.1, 1e-5)


_CASE = {}


def case(lam):
    """One batch, one initial state and the CPU step on them for this lambda: computed once, shared, never modified."""
    if lam not in _CASE:
        from oracle import margin
        torch.manual_seed(5)
        init = {k: v.clone() for k, v in fvit().state_dict().items()}
        u8 = torch.randint(0, 256, (B, 3, 112, 112), dtype=torch.uint8)
        labels = torch.tensor([3, 999, 17, 3, 500, 0, 42, 999])
        P = {k: v.clone().requires_grad_(True) for k, v in init.items() if v.dtype.is_floating_point and "running_" not in k}
        rm, rv = init["mlp_head.0.running_mean"].clone(), init["mlp_head.0.running_var"].clone()
        x, tgt = margin.mixup_batch(u8.float() / 255 * 2 - 1, labels, C, lam)
        emb = cpu_features(P, x, rm, rv, True)
        loss = margin.soft_target_cross_entropy(margin.cosface_logits(emb, P["loss.weight"], tgt), tgt)
        loss.backward()
        _CASE[lam] = dict(init=init, u8=u8, labels=labels, loss=float(loss.detach()), grad={k: p.grad.clone() for k, p in P.items()},
                          running_mean=rm, running_var=rv)
    return _CASE[lam]


@pytest.mark.parametrize("lam", [1.0, 0.3])
def test_fvit_micro_step_against_the_cpu_yardstick(lam):
    """u8 batch -> mixup -> window embedding -> trunk -> BatchNorm1d (batch statistics) -> CosFace -> soft-target CE -> backward."""
    from lafs_cvpr2024_amd.finetune_engine import FinetuneEngine
    ref = case(lam)
    model = fvit()
    model.load_state_dict(ref["init"], strict=True)
    model.train()
    eng = FinetuneEngine(model, B, acc_step=1, device=DEV)
    eng.zero_after_step = True
    loss = float(eng.micro_step(ref["u8"].to(DEV), ref["labels"].to(DEV), lam=lam).item())
    named, bn = dict(model.named_parameters()), model.mlp_head[0]
    # the identically vanishing sum: the CPU numbers confirm it vanishes; this build's error against the neighbouring sum's norm
    scale = float(ref["grad"][ZERO_SUM_SCALE].double().norm())
    assert float(ref["grad"][ZERO_SUM].double().norm()) < 1e-4 * scale
    e_zero = float((named[ZERO_SUM].grad.detach().double().cpu() - ref["grad"][ZERO_SUM].double()).norm()) / scale
    # (measure everything before any gate fires)
    e_loss = abs(loss - ref["loss"]) / abs(ref["loss"])
    errs = {k: rel_l2(named[k].grad, ref["grad"][k]) for k in KEYS}
    e_bn = {k: rel_l2(getattr(bn, k), ref[k]) for k in ("running_mean", "running_var")}
    print(f"[fViT fine-tune, lam {lam}] loss {loss:.6f} vs {ref['loss']:.6f} ({e_loss:.3e}), vanishing fc2 bias {e_zero:.3e}, "
          f"running_mean {e_bn['running_mean']:.3e}, running_var {e_bn['running_var']:.3e}")
    for k in KEYS:
        print(f"[fViT fine-tune, lam {lam}]   grad {k}: {errs[k]:.3e}")
    gate_errors("fViT fine-tune loss", {"loss": e_loss}, GATE_LOSS)
    gate_errors("fViT fine-tune gradients", errs, GATE_GRAD)
    gate_errors("fViT fine-tune vanishing fc2-bias gradient (absolute, over the neighbouring sum's norm)", {ZERO_SUM: e_zero}, GATE_ZERO_SUM)
    gate_errors("fViT fine-tune BatchNorm buffers", e_bn, GATE_BN)
    assert nbt(model) == 1 and eng.bn_forward == 0
    # one AdamW step runs and moves the weights by about lr
    w0 = named["patch_to_embedding.weight"].detach().clone()
    eng.optimizer_step(lr=1e-3, weight_decay=0.1)
    d = (named["patch_to_embedding.weight"].detach() - w0).abs().max().item()
    assert 0.5e-3 < d < 2.5e-3, d
    assert float(eng.arena.grad.abs().max()) == 0.0


@pytest.mark.parametrize("training", [False, True])
def test_fvit_engine_matches_the_module_path(training):
    """FinetuneEngine on an fViT == the autograd module path (pinned to the reference by F26 and F10) on the same batch, with the
    head on running statistics (eval mode) and on batch statistics (training mode)."""
    from lafs_cvpr2024_amd.finetune_engine import FinetuneEngine
    torch.manual_seed(6)
    u8 = torch.randint(0, 256, (B, 3, 112, 112), dtype=torch.uint8, device=DEV)
    labels = torch.tensor([3, 999, 17, 3, 500, 0, 42, 999], device=DEV)
    keys = ("patch_to_embedding.weight", "loss.weight", "mlp_head.0.weight", "transformer.layers.1.0.fn.fn.to_qkv.weight")
    m1 = fvit(); m1.train(training)
    eng = FinetuneEngine(m1, B, acc_step=1, device=DEV)
    state = {k: v.clone() for k, v in m1.state_dict().items()}
    loss1 = float(eng.micro_step(u8, labels, lam=1.0).item())
    g1 = {k: dict(m1.named_parameters())[k].grad.clone() for k in keys}
    m2 = fvit(); m2.load_state_dict(state); attach_arena(m2, DEV); m2.train(training)
    logits, emb = m2.forward_features(u8.float() / 255 * 2 - 1, label=labels)
    assert logits.shape == (B, C) and emb.shape == (B, 128)
    loss2 = F.cross_entropy(logits, labels)
    loss2.backward()
    loss2 = loss2.detach()
    bad = {k: rel_l2(g1[k], dict(m2.named_parameters())[k].grad) for k in keys}
    print(f"[fViT engine vs module, training={training}] loss", loss1, float(loss2), "gradient rel-L2", {k: f"{v:.2e}" for k, v in bad.items()})
    assert abs(loss1 - float(loss2)) < 5e-3 * abs(float(loss2)), (loss1, float(loss2))
    assert all(v < 5e-2 for v in bad.values()), bad
    b1, b2 = m1.mlp_head[0], m2.mlp_head[0]
    assert nbt(m1) == nbt(m2) == int(training)
    for k in ("running_mean", "running_var"):                               # written in training mode only, by both paths
        assert torch.equal(getattr(b2, k).cpu(), state["mlp_head.0." + k].cpu()) == (not training), k
        assert torch.equal(getattr(b1, k).cpu(), state["mlp_head.0." + k].cpu()) == (not training), k


def test_captured_fvit_step_equals_the_eager_step():
    """The fViT micro-step as hipGraphs against the same engine run eagerly: three accumulation windows of two micro-steps with live
    dropout / DropPath / mixup, with the tolerances of the Part-fViT test (tests/test_gpu_finetune.py).  In addition both runs count
    six BatchNorm forwards, and the running statistics agree after the FIRST micro-step: the eager warm-up body in front of the first
    capture updates them in place, so a warm-up that leaks counts the first batch twice (10 % at momentum 0.1)."""
    from lafs_cvpr2024_amd.finetune_engine import FinetuneEngine
    Bw = 16
    res = {}
    for mode in ("graph", "eager", "eager2"):
        torch.manual_seed(4)
        model = fvit(p=0.1)
        model.train()
        eng = FinetuneEngine(model, Bw, acc_step=2, device=DEV, use_graph=(mode == "graph"))
        g = torch.Generator(device=DEV).manual_seed(9)
        losses, first = [], None
        for it in range(6):
            u8 = torch.randint(0, 256, (Bw, 3, 112, 112), device=DEV, dtype=torch.uint8, generator=g)
            y = torch.randint(0, C, (Bw,), device=DEV, generator=g)
            losses.append(float(eng.micro_step(u8, y, lam=(0.3 if it % 3 == 0 else 1.0)).item()))
            if it == 0:
                first = {k: getattr(model.mlp_head[0], k).clone() for k in ("running_mean", "running_var")}
            if it % 2 == 1:
                eng.optimizer_step(lr=1e-3, weight_decay=0.1)
        torch.cuda.synchronize()
        if mode == "graph":
            assert len(eng._graphs) == 2, "two captured variants: first / later micro-step of a window"
        assert nbt(model) == 6
        res[mode] = dict(losses=losses, master=eng.arena.master.clone(), first=first)
    a, b, b2 = res["graph"], res["eager"], res["eager2"]
    noise = max(abs(x - y) / abs(y) for x, y in zip(b2["losses"], b["losses"]))
    e_first = {k: rel_l2(a["first"][k], b["first"][k]) for k in a["first"]}
    print("[fViT graph vs eager] losses", a["losses"], b["losses"], "eager run-to-run", noise, "statistics after the first micro-step", e_first)
    assert all(v < 1e-5 for v in e_first.values()), e_first
    tol0 = 1e-5
    assert abs(a["losses"][0] - b["losses"][0]) < tol0 * abs(b["losses"][0]) and abs(a["losses"][1] - b["losses"][1]) < tol0 * abs(b["losses"][1])
    for x, y in zip(a["losses"][2:], b["losses"][2:]):
        assert abs(x - y) < max(2e-3, 5 * noise) * abs(y), (a["losses"], b["losses"])
    d = (a["master"] - b["master"]).abs()
    dn = (b2["master"] - b["master"]).abs()
    frac, frac_n = float((d > 1e-5).float().mean()), float((dn > 1e-5).float().mean())
    assert float(d.max()) <= 3 * 2.2 * 1e-3 and frac < max(2e-2, 1.5 * frac_n + 1e-3), (float(d.max()), frac, frac_n)


def test_fvit_engine_with_sharded_head_single_rank():
    """FinetuneEngine(sharded_head=PartialFC) on an fViT built with loss_type='None' at world 1 == the dense CosFace engine path on
    the same weights (hard labels)."""
    from lafs_cvpr2024_amd.finetune_engine import FinetuneEngine
    from lafs_cvpr2024_amd.partial_fc import PartialFC
    Cs = 512
    torch.manual_seed(8)
    dense = fvit(num_class=Cs)
    bare = fvit(loss_type="None", num_class=Cs)
    bare.load_state_dict({k: v for k, v in dense.state_dict().items() if not k.startswith("loss.")})
    u8 = torch.randint(0, 256, (B, 3, 112, 112), dtype=torch.uint8, device=DEV)
    labels = torch.randint(0, Cs, (B,), device=DEV)
    e1 = FinetuneEngine(dense, B, acc_step=1, device=DEV)
    l1 = float(e1.micro_step(u8, labels, lam=1.0).item())
    head = PartialFC(128, Cs, B, sample_rate=1.0, device=DEV)
    with torch.no_grad():
        head.weight.copy_(dense.loss.weight.detach())
    head.arena.refresh_shadows()
    e2 = FinetuneEngine(bare, B, acc_step=1, device=DEV, sharded_head=head)
    e2.zero_after_step = True
    l2 = float(e2.micro_step(u8, labels, lam=1.0).item())
    assert abs(l1 - l2) < 5e-3 * abs(l1), (l1, l2)
    g1, g2 = dict(dense.named_parameters()), dict(bare.named_parameters())
    for k in ("patch_to_embedding.weight", "transformer.layers.0.0.fn.fn.to_qkv.weight", "transformer.layers.1.1.fn.fn.net.3.weight",
              "mlp_head.0.weight"):
        assert rel_l2(g2[k].grad, g1[k].grad) < 3e-2, k
    assert rel_l2(head.arena.view(head.arena.grad, "weight", (Cs, 128)), g1["loss.weight"].grad) < 3e-2
    assert nbt(dense) == nbt(bare) == 1
    e2.optimizer_step(lr=1e-3)
    assert float(head.arena.grad.abs().max()) == 0.0 and float(e2.arena.grad.abs().max()) == 0.0
