"""fViT (ViTs_face_overlap) in the evaluation tools: LFW-style verification and IJB feature extraction against the module path, both
leaving the model and a running fine-tune untouched; the attention read-out against an fp32 CPU restatement; tools/attention_maps.py
--arch fvit; and one full-size run of train_largescale.py --net VITs whose saved checkpoint the verification entry point scores to the
same accuracy string (the BatchNorm buffers travel through the checkpoint).

The read-out gate is relative L2 over the whole [B, heads, n+1, n+1] tensor against softmax(dim ** -0.5 q k^T) of the CPU restatement
behind the blocks in front, 2x the worst value observed on MI355X:
                                                     observed   gate
  attention probabilities, block 0 / last block      1.3e-3     2.5e-3    (1.15e-3 / 1.26e-3; Part-fViT's GATE_F24_ATTN: 1.0e-3 observed)
The backbone weights are the F26 fixture's (tests/fvit_cases.py), as in tests/test_gpu_fvit_finetune.py.
"""
import os
import re
import subprocess
import sys
import time

import numpy as np
import pytest
import torch
import torch.nn.functional as F

sys.path.insert(0, os.path.dirname(__file__))
pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tools"))

from conftest import gate_errors, sub  # noqa: E402
from fvit_cases import FVIT_CFG, load_fvit  # noqa: E402
from lafs_cvpr2024_amd import ijb_evaluation as J  # noqa: E402
from lafs_cvpr2024_amd import verification as V  # noqa: E402
from lafs_cvpr2024_amd.face_pre_pro.ViT_face import ViTs_face_overlap  # noqa: E402
from lafs_cvpr2024_amd.vision_transformer import attach_arena  # noqa: E402

DEV = "cuda"
GATE_ATTN = 2.5e-3

_FX = {}


def rel_l2(a, b):
    a, b = torch.as_tensor(a).double().cpu(), torch.as_tensor(b).double().cpu()
    return ((a - b).norm() / (b.norm() + 1e-30)).item()


def fvit(loss_type="None", num_class=10, p=0.0, weights="fixture"):
    """The small model with non-trivial running statistics (the fixture's, behind its two training groups) and the F26 fixture's
    backbone weights -- or, with weights="constructor", the (seeded) draw of the constructor, as the Part-fViT tests use it."""
    if not _FX:
        fx = load_fvit()
        _FX.update({k: (v.float() if v.dtype.is_floating_point else v) for k, v in sub(fx, "p.").items()})
        _FX.update({"mlp_head.0." + k: fx["bn." + k] for k in ("running_mean", "running_var", "num_batches_tracked")})
    m = ViTs_face_overlap(pad=4, **{**FVIT_CFG, "loss_type": loss_type, "num_class": num_class, "dropout": p, "emb_dropout": p},
                          drop_path_rate=p)
    missing = m.load_state_dict(_FX if weights == "fixture" else {k: v for k, v in _FX.items() if ".running_" in k or "num_batches" in k},
                                strict=False)
    if weights != "fixture":
        return m
    assert not missing.unexpected_keys and set(missing.missing_keys) <= {"loss.weight"}
    return m


def bits(t):
    return t.detach().reshape(-1).contiguous().view(torch.uint8).cpu()


def buffers(m):
    """The BatchNorm buffers as they are, without the state_dict hook of an engine."""
    return {k: v.detach().clone() for k, v in m.named_buffers()}


# ----------------------------------------------------------------------------------------------------------------- verification
@pytest.mark.parametrize("weights,n_img,batch", [("constructor", 24, 12), ("fixture", 32, 16), ("fixture", 20, 10)])
def test_verification_features_match_the_module_path(weights, n_img, batch):
    """The evaluator's per-copy features against m(xs), m(xs.flip(3)), below 1e-5 -- with evaluator batches of n_img / 2 images, so that
    its passes (the batch and its mirror: 2 x batch rows) and the module's have the same number of rows.  The trunk's LayerNorm forward
    switches kernels at 4096 token rows (functional.LN_TWO_ROW_MIN) and the two sum in different orders; bf16 roundings behind them carry
    that far above 1e-5, so passes on different sides of the switch are not the same computation, whoever runs them.  Measured on
    MI355X, module path against itself, 24 images in one pass (4728 token rows) against passes of 8 / 16 / 20 / 21 images (1576 / 3152 /
    3940 / 4137 rows): 5.6e-4 / 5.2e-4 / 6.2e-4 / 0 with the fixture's weights, 3.9e-7 / 4.8e-7 / 4.3e-7 / 0 with the constructor's.
    The shape of the Part-fViT test this one mirrors (tests/test_gpu_verification.py: 24 images, evaluator batches of 8 = 16 rows
    against 24) straddles the switch: the constructor's weights gave 3.9e-7 on the plain copy and 6.3e-5 on the mirrored one there.
    Cases: the constructor's weights as in that test, and trained-scale weights (the F26 fixture's) on either side of the switch:
    24 and 32 rows (4728 / 6304 token rows), 20 rows (3940)."""
    torch.manual_seed(4)
    m = fvit(p=0.1, weights=weights)
    attach_arena(m, DEV)
    x = torch.randint(0, 256, (n_img, 3, 112, 112), dtype=torch.uint8, generator=torch.Generator().manual_seed(5))
    issame = np.arange(n_img // 2) % 2 == 0
    ev = V.VerificationEvaluator(m, batch, DEV)
    ev.keep_features = True
    assert m.training
    before = buffers(m)
    res = ev(x, issame)
    assert np.isfinite(res[2]) and 0.0 <= res[0] <= 1.0
    assert m.training and m._drop_step == 0
    after = buffers(m)
    assert set(before) == {"mlp_head.0." + k for k in ("running_mean", "running_var", "num_batches_tracked")}
    assert all(torch.equal(bits(before[k]), bits(after[k])) for k in before)
    m.eval()
    with torch.no_grad():
        xs = (x.float() / 255.0 - 0.5).to(DEV)
        e0, e1 = m(xs).cpu(), m(xs.flip(3)).cpu()
    errs = (rel_l2(ev.features[0], e0), rel_l2(ev.features[1], e1))
    print(f"[fViT verification vs module, {weights} weights, {n_img} images] per-copy rel-L2 {errs[0]:.2e} / {errs[1]:.2e}")
    assert max(errs) < 1e-5, errs
    assert all(torch.equal(bits(before[k]), bits(buffers(m)[k])) for k in before)


def _training_state(eng, m):
    """Every device tensor the engine and its arena hold (one level into dicts), the model's buffers (read without the state_dict hook,
    which would flush num_batches_tracked) and the host counters a later step reads."""
    st = {}
    for name, obj in (("eng", eng), ("arena", eng.arena)):
        for k, v in vars(obj).items():
            if isinstance(v, torch.Tensor):
                st[f"{name}.{k}"] = v.clone()
            elif isinstance(v, dict):
                st.update({f"{name}.{k}.{kk}": vv.clone() for kk, vv in v.items() if isinstance(vv, torch.Tensor)})
    st.update({"buf." + k: v.clone() for k, v in m.named_buffers()})
    host = dict(micro=eng.micro, since_opt=eng._since_opt, hp=dict(eng._hp), bn_forward=eng.bn_forward, drop_step=m._drop_step,
                training=m.training)
    return st, host


def test_evaluation_does_not_perturb_fvit_training():
    """An evaluation between two optimizer steps leaves every tensor and counter a later step reads bit-identical."""
    from lafs_cvpr2024_amd.finetune_engine import FinetuneEngine
    B = 8
    g = torch.Generator().manual_seed(9)
    xs = [torch.randint(0, 256, (B, 3, 112, 112), dtype=torch.uint8, generator=g).to(DEV) for _ in range(3)]
    ys = [torch.randint(0, 1000, (B,), generator=g).to(DEV) for _ in range(3)]
    val = torch.randint(0, 256, (20, 3, 112, 112), dtype=torch.uint8, generator=g)
    torch.manual_seed(11)
    m = fvit(loss_type="CosFace", num_class=1000, p=0.1)
    eng = FinetuneEngine(m, B, acc_step=1, mixup_prob=0.5, device=DEV)
    m.train()
    np.random.seed(3)
    losses = [float(eng.step(xs[0], ys[0], lr=1e-3).item())]
    torch.cuda.synchronize()
    before, host0 = _training_state(eng, m)
    assert len(before) > 25 and host0["bn_forward"] == 1 and "buf.mlp_head.0.running_var" in before
    rng = np.random.get_state()
    res = V.VerificationEvaluator(m, 10, DEV)(val, np.arange(10) % 2 == 0, engine=eng)
    torch.cuda.synchronize()
    after, host1 = _training_state(eng, m)
    assert np.isfinite(res[2]) and 0.0 <= res[0] <= 1.0
    assert host0 == host1, (host0, host1)
    assert all(a == b for a, b in zip(rng[1], np.random.get_state()[1]))        # the mixup draws are not consumed
    bad = [k for k in before if not torch.equal(bits(before[k]), bits(after[k]))]
    assert not bad, bad
    for k in (1, 2):
        losses.append(float(eng.step(xs[k], ys[k], lr=1e-3).item()))
    assert all(np.isfinite(losses)), losses
    assert int(m.state_dict()["mlp_head.0.num_batches_tracked"]) == int(_FX["mlp_head.0.num_batches_tracked"]) + 3


# ----------------------------------------------------------------------------------------------------------------- IJB
def test_ijb_features_match_the_module_path_and_leave_the_model_untouched():
    import make_synthetic_ijb as syn
    torch.manual_seed(4)
    m = fvit(p=0.1)
    attach_arena(m, DEV)
    n = 10
    imgs, lmk = syn.images(n), syn.dataset(n)["lmk"].astype(np.float32)
    before = {k: v.detach().clone() for k, v in m.state_dict().items()}
    ev = J.IJBEvaluator(m, 4, DEV)
    ev.keep_aligned = True
    assert m.training
    feats = ev.features(imgs, lmk).cpu()
    assert m.training and m._drop_step == 0
    after = m.state_dict()
    assert before.keys() == after.keys() and all(torch.equal(bits(before[k]), bits(after[k])) for k in before)
    m.eval()
    div, mul, add = V.NORMS[ev.norm]
    d32 = lambda v: torch.tensor(v, dtype=torch.float32)
    with torch.no_grad():
        xs = (ev.aligned.float() / d32(div) * d32(mul) + d32(add)).to(DEV)
        e0, e1 = m(xs).cpu(), m(xs.flip(3)).cpu()
    D = e0.shape[1]
    errs = (rel_l2(feats[:, :D], e0), rel_l2(feats[:, D:], e1))
    assert feats.shape == (n, 2 * D) and max(errs) < 1e-5, errs


# ----------------------------------------------------------------------------------------------------------------- read-out
def cpu_attention(P, x, layer):
    """softmax(dim ** -0.5 q k^T) of block `layer` behind the blocks in front of it, fp32 on the CPU: [B, heads, n+1, n+1]."""
    from oracle import partfvit
    cfg = partfvit.PartFViTConfig(patch_size=8, dim=FVIT_CFG["dim"], depth=layer, heads=FVIT_CFG["heads"], mlp_dim=FVIT_CFG["mlp_dim"],
                                  num_patches=196)
    t = F.linear(F.unfold(x, 12, stride=8, padding=4).transpose(1, 2), P["patch_to_embedding.weight"], P["patch_to_embedding.bias"])
    Bn, n, D = t.shape
    t = torch.cat((P["cls_token"].expand(Bn, -1, -1), t), dim=1) + P["pos_embedding"][:, :n + 1]
    t = partfvit.transformer(P, t, cfg)                                      # the first `layer` blocks
    a = f"transformer.layers.{layer}.0.fn."
    h = F.layer_norm(t, (D,), P[a + "norm.weight"], P[a + "norm.bias"], cfg.ln_eps)
    q, k, _ = F.linear(h, P[a + "fn.to_qkv.weight"]).chunk(3, dim=-1)
    sp = lambda u: u.view(Bn, n + 1, cfg.heads, cfg.dim_head).transpose(1, 2)
    return (sp(q) @ sp(k).transpose(-1, -2) * cfg.scale).softmax(dim=-1)


def test_attention_readout_against_the_cpu_restatement():
    m = fvit()
    attach_arena(m, DEV)
    x = load_fvit()["x0"].float()
    with pytest.raises(RuntimeError, match="eval"):
        m.get_selfattention(x.to(DEV))
    m.eval()
    before = buffers(m)
    P = {k: v.detach().float().cpu() for k, v in m.state_dict().items()}
    errs = {}
    for layer in (0, -1):
        attn = m.get_selfattention(x.to(DEV), layer=layer)
        assert isinstance(attn, torch.Tensor) and attn.shape == (2, 3, 197, 197) and attn.dtype == torch.float32
        errs[f"block {layer % 2}"] = rel_l2(attn, cpu_attention(P, x, layer % 2))
        assert float((attn.sum(-1) - 1).abs().max()) < 1e-5
        row0 = m.get_selfattention(x.to(DEV), layer=layer, cls_only=True)
        assert row0.shape == (2, 3, 1, 197) and torch.equal(bits(row0), bits(attn[:, :, :1]))
    assert torch.equal(bits(m.get_selfattention(x.to(DEV))), bits(attn))     # the default is the last block
    print("[fViT attention read-out]", {k: f"{v:.3e}" for k, v in errs.items()})
    gate_errors("fViT attention read-out", errs, GATE_ATTN)
    assert all(torch.equal(bits(before[k]), bits(buffers(m)[k])) for k in before)


def test_attention_maps_tool_draws_fvit(tmp_path):
    out = tmp_path / "maps"
    cmd = [sys.executable, os.path.join(ROOT, "tools", "attention_maps.py"), "--arch", "fvit", "--random-init", "--dims", "128,2,3,256",
           "--num", "2", "--out", str(out)]
    p = subprocess.run(cmd, capture_output=True, text=True, env=dict(os.environ, PYTHONPATH=ROOT), timeout=300)
    assert p.returncode == 0, p.stdout[-3000:] + p.stderr[-3000:]
    from PIL import Image
    for b in range(2):
        for h in range(3):
            w = np.load(out / f"img{b}_head{h}.npy")
            assert w.shape == (14, 14) and w.dtype == np.float32 and np.all(w >= 0) and 0 < float(w.sum()) <= 1.0 + 1e-5
            with Image.open(out / f"img{b}_head{h}.png") as im:
                assert im.size == (112, 112)
    assert not (out / "img0_theta.npy").exists()


# ----------------------------------------------------------------------------------------------------------------- the CLI, full size
def test_train_largescale_vits_then_verification_entry_point(tmp_path):
    """The only slow test: nine micro-steps of the released configuration (three optimizer steps, one evaluation behind the third), then
    the saved checkpoint through `python -m lafs_cvpr2024_amd.verification --net VITs`."""
    import make_synthetic_bin
    val, outdir = tmp_path / "val", tmp_path / "out"
    outdir.mkdir()
    env = dict(os.environ, PYTHONPATH=ROOT)
    make_synthetic_bin.make(str(val / "lfw.bin"), 20)
    arch = ["--net", "VITs", "--num_class", "32", "--batch_size", "8", "--val_batch_size", "20"]
    cmd = [sys.executable, os.path.join(ROOT, "train_largescale.py"), "--epochs", "1", "--steps_per_epoch", "9", "--val_path", str(val),
           "--target", "lfw", "--ver_freq", "3", "--outdir", str(outdir)] + arch
    t0 = time.time()
    p = subprocess.run(cmd, capture_output=True, text=True, env=env, timeout=600)
    t1 = time.time()
    assert p.returncode == 0, p.stdout[-3000:] + p.stderr[-3000:]
    log = p.stdout
    acc = dict(re.findall(r"\[lfw\]\[(\d+)\]Accuracy-Flip: (\S+)", log))
    assert sorted(int(b) for b in acc) == [9], log                 # optimizer step 3 (acc_step 3, divisor max(1, 3 // 3))
    assert os.path.exists(outdir / "Backbone_VITs_Epoch_1.pth")
    ckpts = sorted(f for f in os.listdir(outdir) if f.endswith("_checkpoint.pth"))
    assert ckpts and all(f.startswith("Backbone_VITs_Epoch_1_Batch_9_") for f in ckpts), (ckpts, log)
    sd = torch.load(outdir / ckpts[0], map_location="cpu", weights_only=False)
    assert int(sd["module.mlp_head.0.num_batches_tracked"]) == 9 and tuple(sd["module.loss.weight"].shape) == (32, 768)
    assert float((sd["module.mlp_head.0.running_mean"]).abs().max()) > 0
    q = subprocess.run([sys.executable, "-m", "lafs_cvpr2024_amd.verification", "--checkpoint", str(outdir / ckpts[0]), "--val_path", str(val),
                        "--target", "lfw"] + arch, capture_output=True, text=True, env=env, timeout=600, cwd=ROOT)
    assert q.returncode == 0, q.stdout[-3000:] + q.stderr[-3000:]
    got = re.search(r"\[lfw\]\[0\]Accuracy-Flip: (\S+)", q.stdout).group(1)
    print(f"[fViT CLI] train_largescale.py --net VITs: {t1 - t0:.1f} s, verification entry point: {time.time() - t1:.1f} s; "
          + " | ".join(ln for ln in log.splitlines() if "samples/s" in ln))
    assert got == acc["9"], (got, acc, q.stdout)
