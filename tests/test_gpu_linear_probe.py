"""GPU: the linear probe -- lafs_softmax_ce_rank against the fp64 reference of tests/linear_cases.py, element by element, inside guard rows
and columns; one LinearProbe training step against fp64 products of the very bf16 operands it used and an fp64 SGD replay; a fit whose
outcome is a condition (separable classes: 100 %); and the eval_linear tool on random-init checkpoints of a DINO ViT and an fViT.
tests/test_oracle_linear_host.py shows on the CPU that the kernel's bounds mean something and that seeded faults fail them."""
import io
import json
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(__file__))
pytestmark = pytest.mark.gpu

import fp64_bounds as fb  # noqa: E402
import linear_cases as lc  # noqa: E402
import sgd_lars_cases as sc  # noqa: E402
from fp64_bounds import CHUNK, bf16, f32  # noqa: E402

DEV = "cuda"
GUARD = 64                                               # guard elements (128 B of bf16: the gradient rows stay 16-byte aligned)


def _bits(t):
    return t.view({4: torch.int32, 2: torch.int16}[t.element_size()])


class Guarded:
    """A flat device buffer of `fill` with `n` payload elements `off` elements in; `x` is the payload, `intact()` whether every other
    element still holds the fill."""

    def __init__(self, n, dtype, fill, off=GUARD):
        self.buf = torch.full((off + n + GUARD,), fill, dtype=dtype, device=DEV)
        self.x = self.buf[off:off + n]
        self.start = _bits(self.buf).clone()
        self.mask = torch.ones(self.buf.numel(), dtype=torch.bool, device=DEV)
        self.mask[off:off + n] = False

    def intact(self):
        return torch.equal(_bits(self.buf)[self.mask], self.start[self.mask])

    def untouched(self):
        return torch.equal(_bits(self.buf), self.start)


# ------------------------------------------------------------------------------------------------ the kernel
@pytest.mark.parametrize("c", lc.CASES, ids=lambda c: c["id"])
def test_kernel_against_fp64_reference(c):
    from lafs_cvpr2024_amd import _lib, ops
    d = lc.inputs(c)
    B, C, ld, lddl = c["B"], c["C"], c["ld"], c["lddl"]
    # logits [B, ld] whose columns [C, ld) hold the sentinel; with ld = C + 3 the base is one float off a 16-byte boundary as well
    lg = Guarded(B * ld, f32, lc.SENTINEL, off=GUARD + (1 if ld != C else 0))
    z = lg.x.view(B, ld)
    z[:, :C] = d["z"].float().to(DEV)
    lg.start = _bits(lg.buf).clone()
    y = d["y"].to(torch.int32).to(DEV)
    need = int(_lib.lib().lafs_softmax_ce_rank_workspace_bytes(B, C))
    assert need > 0 and need % 4 == 0
    out = []
    for _ in range(2):
        dl, loss, rank, ws = (Guarded(B * lddl, bf16, lc.SENTINEL), Guarded(B, f32, lc.SENTINEL), Guarded(B, torch.int32, -77),
                              Guarded(need // 4, f32, lc.SENTINEL))
        ops.softmax_ce_rank(z, y, C, d["gs"], dl.x.view(B, lddl), loss.x, rank.x, ws.x)
        torch.cuda.synchronize()
        for name, g in (("dlogits", dl), ("row_loss", loss), ("row_rank", rank), ("workspace", ws)):
            assert g.intact(), f"{c['id']}: a guard of `{name}` was written"
        assert lg.untouched(), f"{c['id']}: the logits are read-only"
        out.append((loss.x.clone(), rank.x.clone(), dl.x.view(B, lddl).clone()))
    for a, b in zip(out[0], out[1]):
        assert torch.equal(_bits(a), _bits(b)), f"{c['id']}: two calls on equal inputs differ"
    worst = lc.judge(c, d, *out[0])
    print(f"{c['id']}: worst |err|/bound {worst:.3f}")
    # no gradient asked for: the same loss and rank, and a gradient buffer nobody touches
    dl, loss, rank, ws = Guarded(B * lddl, bf16, lc.SENTINEL), Guarded(B, f32, lc.SENTINEL), Guarded(B, torch.int32, -77), Guarded(need // 4, f32, 0.0)
    ops.softmax_ce_rank(z, y, C, d["gs"], None, loss.x, rank.x, ws.x)
    torch.cuda.synchronize()
    assert dl.untouched() and loss.intact() and rank.intact() and ws.intact() and lg.untouched()
    assert torch.equal(_bits(loss.x), _bits(out[0][0])) and torch.equal(rank.x, out[0][1])


def test_bad_arguments_are_refused():
    from lafs_cvpr2024_amd import _lib, ops
    z = torch.zeros(4, 16, device=DEV)
    y = torch.zeros(4, dtype=torch.int32, device=DEV)
    with pytest.raises(_lib.LafsHipError):                   # lddl % 8 != 0
        ops.softmax_ce_rank(z, y, 10, 1.0, torch.zeros(4, 12, dtype=bf16, device=DEV))
    with pytest.raises(_lib.LafsHipError):                   # lddl < C
        ops.softmax_ce_rank(z, y, 16, 1.0, torch.zeros(4, 8, dtype=bf16, device=DEV))
    with pytest.raises(_lib.LafsHipError):                   # a short workspace
        ops.softmax_ce_rank(z, y, 16, 1.0, None, ws=torch.zeros(4, device=DEV))


# ------------------------------------------------------------------------------------------------ one training step
def test_one_training_step_against_fp64():
    from lafs_cvpr2024_amd.linear_probe import LinearProbe
    B, F, C = 24, 40, 37
    gen = torch.Generator().manual_seed(3)
    feats = torch.randn(B, F, generator=gen)
    labels = torch.randint(0, C, (B,), generator=gen)
    labels[[4, 11, 23]] = -1
    labels[0], labels[1] = 0, C - 1
    probe = LinearProbe(F, C, DEV, seed=1)
    assert (probe.Fp, probe.Cp) == (64, 40)
    a = probe.arena
    w0 = probe.params.weight.data.cpu()
    assert bool((w0[C:] == 0).all()) and bool((w0[:, F:] == 0).all()) and abs(float(w0[:C, :F].std()) - 0.01) < 2e-3
    assert bool((probe.params.bias.data == 0).all())
    probe.set_lr(0.1)
    cached = probe.cache(feats, labels)
    idx = torch.arange(B, device=DEV)
    hp = probe.hyper.double()
    c = dict(id="step", B=B, C=C, ld=probe.Cp, lddl=probe.Cp)
    for it in range(2):                                      # the second step starts from a non-zero momentum buffer
        before = {k: getattr(a, k).double().view(a.n_chunks, CHUNK).clone() for k in ("master", "exp_avg")}
        w16, bias = probe.w_bf16.double().clone(), probe.b.double().clone()
        step0 = a.seg_step.clone()
        probe.step(cached, idx, n_target=B - 3)
        torch.cuda.synchronize()
        x, dl, logits = probe.last_x_bf16.double(), probe.last_dlogits.double(), probe.last_logits
        assert torch.equal(x[:, :F], feats.to(bf16).double().to(DEV)) and bool((x[:, F:] == 0).all())
        # the logits: the bf16 operands' product; the loss kernel on those very logits
        fb.check(f"step {it}: logits", logits, *fb.gemm(x, None, w16, bias))
        d = {"z": logits[:, :C].double().cpu(), "y": labels.clone(), "gs": float(torch.tensor(1.0 / (B - 3), dtype=f32))}
        exp = lc.reference(c, d)
        fb.check(f"step {it}: dlogits", dl.cpu(), *exp["dl"])
        assert bool((dl[[4, 11, 23]] == 0).all()) and bool((dl[:, C:] == 0).all())
        # dW and db: fp64 products of the bf16 operands the step used
        fb.check(f"step {it}: dW", probe.dW, *fb.gemm_tn(dl, x))
        fb.check(f"step {it}: db", probe.db, *fb.colsum(dl))
        # the update: an fp64 SGD-with-momentum replay from the state before, on the kernel's own fp32 gradient
        g = a.grad.double().view(a.n_chunks, CHUNK)
        out = sc.step64("sgd", before["master"], g, before["exp_avg"], None, a.chunk_seg, a.seg_flags, step0, hp, a.n_seg)
        fb.check(f"step {it}: param", a.master.view(a.n_chunks, CHUNK), *out["param"])
        fb.check(f"step {it}: momentum", a.exp_avg.view(a.n_chunks, CHUNK), *out["mom"])
        fb.check(f"step {it}: param_bf16", a.shadow.view(a.n_chunks, CHUNK), *out["param16"], True)
        assert torch.equal(a.seg_step.long(), out["seg_step"]) and a.seg_step.tolist() == [it + 1, it + 1]
        assert not torch.equal(a.master.double().view(a.n_chunks, CHUNK), before["master"])
        w = probe.params.weight.data
        assert bool((w[C:] == 0).all()) and bool((w[:, F:] == 0).all()), "the pad rows and columns of the weight stay zero"


# ------------------------------------------------------------------------------------------------ a fit whose outcome is a condition
def _separable(seed=0):
    """8 classes in 64 dimensions: centres 4 x unit vectors, noise 0.3 randn, 48 rows per class in record order (identity by identity)."""
    gen = torch.Generator().manual_seed(seed)
    centres = torch.randn(8, 64, generator=gen)
    centres = 4 * centres / centres.norm(dim=1, keepdim=True)
    labels = np.repeat(np.arange(8) * 11 + 5, 48)        # identities 5, 16, 27, ...: re-indexed by the split
    feats = centres.repeat_interleave(48, dim=0) + 0.3 * torch.randn(8 * 48, 64, generator=gen)
    return feats, labels


def _fit(feats, labels, shots):
    from lafs_cvpr2024_amd.linear_probe import LinearProbe, probe_split
    train_i, val_i, y_train, y_val, n_class = probe_split(labels, holdout=8, shots=shots)
    probe = LinearProbe(64, n_class, DEV, seed=0)
    probe.fit(feats[train_i], y_train, epochs=10, batch_size=64, lr=0.4, seed=0)      # lr * 64 / 256 = 0.1
    return probe, probe.evaluate(feats[val_i], y_val), len(train_i), len(val_i)


def test_fit_on_separable_classes():
    feats, labels = _separable()
    probe, (top1, top5, loss), n_train, n_val = _fit(feats, labels, 0)
    print(f"\nseparable fit: top1 {top1}, top5 {top5}, loss {loss:.3e} ({n_train} / {n_val})")
    assert (n_train, n_val, probe.C) == (320, 64, 8)
    assert top1 == 100.0 and top5 == 100.0
    assert loss < 0.01
    again, res2, _, _ = _fit(feats, labels, 0)
    assert torch.equal(_bits(again.arena.master), _bits(probe.arena.master)), "two fits from the same seed differ"
    assert res2 == (top1, top5, loss)
    few, (t1, t5, _), n_train, n_val = _fit(feats, labels, 2)
    assert (n_train, n_val) == (16, 64) and 0.0 <= t1 <= t5 <= 100.0
    assert not torch.equal(_bits(few.arena.master), _bits(probe.arena.master))


# ------------------------------------------------------------------------------------------------ the tool
@pytest.fixture(scope="module")
def rec_dir(tmp_path_factory):
    """8 identities x 6 synthetic images in the RecordIO layout (as tests/test_gpu_knn_eval.py)."""
    from PIL import Image
    from lafs_cvpr2024_amd import recordio as R
    out = tmp_path_factory.mktemp("linear_rec")
    n_ids, per = 8, 6
    rng = np.random.RandomState(0)
    w = R.IndexedRecordWriter(str(out / "train.idx"), str(out / "train.rec"))
    n_img = n_ids * per
    w.write_idx(0, R.pack(R.IRHeader(2, [n_img + 1, n_img + 1 + n_ids], 0, 0), b""))
    yy, xx = np.mgrid[0:112, 0:112]
    key = 1
    for ident in range(n_ids):
        base = np.stack([127 + 90 * np.sin(xx / (5.0 + ident % 7) + c) * np.cos(yy / (6.0 + c) - ident) for c in range(3)], -1)
        for _ in range(per):
            img = np.clip(base + rng.randn(112, 112, 3) * 25, 0, 255).astype(np.uint8)
            b = io.BytesIO()
            Image.fromarray(img).save(b, format="JPEG", quality=95)
            w.write_idx(key, R.pack(R.IRHeader(0, float(ident), key, 0), b.getvalue()))
            key += 1
    for ident in range(n_ids):
        w.write_idx(n_img + 1 + ident, R.pack(R.IRHeader(2, [1 + ident * per, 1 + (ident + 1) * per], n_img + 1 + ident, 0), b""))
    w.close()
    return out


def _random_checkpoint(arch, path):
    """A lafs_train.py checkpoint of a random-init teacher: its `args` and the backbone's keys under `backbone.`."""
    from lafs_cvpr2024_amd import lafs_train as L
    args = L.get_args_parser().parse_args((f"--out_dim 512 --output_dir {path.parent} " + arch).split())
    torch.manual_seed(0)
    backbone = L.build_backbones(args)[1]
    torch.save({"teacher": {"backbone." + k: v for k, v in backbone.state_dict().items()}, "args": args}, path)


@pytest.mark.parametrize("arch,extra", [("--arch vit_small --views dino", ["--n_last_blocks", "2"]), ("--arch fvit --fvit_dims 128,2,2,256", [])],
                         ids=["vit_small", "fvit"])
def test_tool_on_a_random_init_checkpoint(tmp_path, rec_dir, arch, extra, capsys):
    from lafs_cvpr2024_amd import eval_linear
    ck = tmp_path / "checkpoint.pth"
    _random_checkpoint(arch, ck)
    argv = ["--checkpoint", str(ck), "--data_path", str(rec_dir), "--epochs", "3", "--batch_size", "16", "--lr", "0.5", "--num_workers", "0"] + extra
    res = eval_linear.main(argv)
    first = (tmp_path / "linear.json").read_bytes()
    line = [l for l in capsys.readouterr().out.splitlines() if l.startswith("Linear probe: Top1 ")]
    assert len(line) == 1 and "(8 classes, 40 / 8)" in line[0]
    d = json.loads(first)
    assert set(d) == {"top1", "top5", "loss", "train_top1", "n_train", "n_val", "n_class"}
    assert (d["n_train"], d["n_val"], d["n_class"]) == (40, 8, 8) and d == {k: res[k] for k in d}
    assert 0.0 <= d["top1"] <= d["top5"] <= 100.0 and 0.0 <= d["train_top1"] <= 100.0 and np.isfinite(d["loss"]) and d["loss"] > 0
    eval_linear.main(argv)
    assert (tmp_path / "linear.json").read_bytes() == first                 # a second run: the same bytes
    if "fvit" in arch:
        with pytest.raises(ValueError, match="n_last_blocks"):
            eval_linear.main(argv + ["--n_last_blocks", "2"])
