"""GPU: the verification path (csrc/verify.hip, lafs_cvpr2024_amd/verification.py) against torch, the reference's golden values
(F21a: perform_val's metric at full scale; F21b: the F13 Part-fViT through perform_val) and the independent CPU oracle; evaluation
leaves the fine-tune state bit-identical; two ranks give one rank's histogram; train_largescale.py --val_path end to end."""
import os
import re
import subprocess
import sys

import numpy as np
import pytest
import torch
import torch.distributed as dist
import torch.multiprocessing as mp

sys.path.insert(0, os.path.dirname(__file__))
pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

import verification_oracle as O  # noqa: E402
from conftest import load_golden, sub  # noqa: E402
from lafs_cvpr2024_amd import verification as V  # noqa: E402
from lafs_cvpr2024_amd.face_pre_pro.ViT_face import ViT_face_landmark_patch8  # noqa: E402
from lafs_cvpr2024_amd.ops import _p, call  # noqa: E402
from lafs_cvpr2024_amd.vision_transformer import attach_arena  # noqa: E402

DEV = "cuda"


def rel_l2(a, b):
    a, b = torch.as_tensor(a).double().cpu(), torch.as_tensor(b).double().cpu()
    return ((a - b).norm() / (b.norm() + 1e-30)).item()


@pytest.mark.parametrize("B", [2, 128])
@pytest.mark.parametrize("norm", ["reference", "train"])
def test_flip_normalize_bit_identical_to_torch(B, norm):
    g = torch.Generator().manual_seed(B)
    x = torch.randint(0, 256, (B, 3, 112, 112), dtype=torch.uint8, generator=g)
    x[0, 0, 0, :16] = torch.arange(16, dtype=torch.uint8) * 17
    xd = x.to(DEV)
    out = torch.full((2 * B, 3, 112, 112), float("nan"), device=DEV)
    div, mul, add = V.NORMS[norm]
    call("lafs_eval_flip_normalize", _p(xd), _p(out), B, 112, div, mul, add)
    torch.cuda.synchronize()
    d32 = lambda v: torch.tensor(v, dtype=torch.float32)
    ref = x.float() / d32(div) * d32(mul) + d32(add)                 # torch's CPU arithmetic, one rounding per operation
    if norm == "reference":
        assert torch.equal(ref, x.float() / 255.0 - 0.5)             # utils.py:314 as the reference writes it
    exp = torch.cat([ref, ref.flip(3)])
    assert torch.equal(out.cpu(), exp)


def _tail(feat, B, pair0, P, bounds, same, hist, norms, dist_out=None, emb=None):
    thr = torch.tensor(V.THRESHOLDS, dtype=torch.float64, device=DEV)
    call("lafs_verify_tail", _p(feat), feat.shape[1], B, feat.shape[1], pair0, P, _p(thr), len(V.THRESHOLDS), _p(bounds), 10, _p(same),
         _p(hist), _p(norms), _p(dist_out), _p(emb))


def test_verify_tail_reproduces_reference_f21a():
    """F21a's per-copy tables as the trunk's output: dist to 1e-12, the histogram's metric EXACTLY the reference's."""
    fx = load_golden("f21a_verification_metric")
    t0, t1, issame = fx["t0"], fx["t1"], fx["issame"].numpy()
    N, P, B = t0.shape[0], t0.shape[0] // 2, 110
    bounds = torch.tensor(V.fold_bounds(P), device=DEV)
    same = torch.tensor(issame.astype(np.uint8), device=DEV)
    hist = torch.zeros(10, 2, 401, device=DEV, dtype=torch.int32)
    norms = torch.zeros(2, N, device=DEV, dtype=torch.float64)
    dist_out = torch.full((P,), -1.0, device=DEV, dtype=torch.float64)
    emb = torch.zeros(N, t0.shape[1], device=DEV, dtype=torch.float32)
    for i0 in range(0, N, B):
        feat = torch.cat([t0[i0:i0 + B], t1[i0:i0 + B]]).to(DEV).contiguous()
        _tail(feat, B, i0 // 2, P, bounds, same, hist, norms, dist_out, emb)
    torch.cuda.synchronize()
    d, ref = dist_out.cpu().numpy(), fx["dist"].numpy()
    assert np.all(np.abs(d - ref) <= 1e-12 * np.abs(ref)), float(np.max(np.abs(d - ref) / np.maximum(np.abs(ref), 1e-300)))
    assert np.sum(ref == 0) > 0 and np.array_equal(d == 0, ref == 0)
    e_ref, _, _ = O.embeddings_and_dist(t0.numpy(), t1.numpy())
    assert float(np.abs(emb.cpu().numpy() - e_ref).max()) < 1e-6
    am, sd, xn, bm, tpr, fpr = V.evaluate(hist.cpu().numpy(), float(norms.sum()), float(norms.numel()))
    assert np.array_equal(V.metrics_from_hist(hist.cpu().numpy())[2], fx["accuracy"].numpy())
    assert am == float(fx["acc_mean"]) and sd == float(fx["acc_std"]) and bm == float(fx["best_threshold_mean"])
    assert np.array_equal(tpr, fx["tpr"].numpy()) and np.array_equal(fpr, fx["fpr"].numpy())
    assert abs(xn - float(fx["xnorm"])) <= 1e-12 * float(fx["xnorm"])


def _f13_model():
    from conftest import det_fill
    fx = load_golden("f13_partfvit_land")
    m = ViT_face_landmark_patch8(loss_type="None", GPU_ID=None, num_class=10, image_size=112, patch_size=8, dim=128, depth=2,
                                 heads=3, mlp_dim=256, dropout=0.0, emb_dropout=0.0, with_land=True)
    det_fill(m.stn); det_fill(m.output_layer)
    m.load_state_dict(sub(fx, "p."), strict=False)
    attach_arena(m, DEV)
    m.eval()
    return m


def test_f21b_partfvit_end_to_end_against_reference():
    fx = load_golden("f21b_verification_partfvit")
    m = _f13_model()
    ev = V.VerificationEvaluator(m, 10, DEV)
    ev.keep_features = True
    res = ev(fx["x_u8"], fx["issame"].numpy())
    feats, ref = ev.features, fx["emb"]
    errs = [rel_l2(feats[c], ref[c]) for c in range(2)]
    xerr = abs(res[2] - float(fx["xnorm"])) / float(fx["xnorm"])
    print(f"[F21b] per-copy embeddings rel-L2 {errs[0]:.2e} / {errs[1]:.2e}, xnorm rel {xerr:.2e}, accuracy {res[0]:.4f} "
          f"(reference {float(fx['acc_mean']):.4f})")
    assert max(errs) < 2e-2 and xerr < 2e-2, (errs, xerr)
    o = O.perform_val(feats[0].numpy(), feats[1].numpy(), fx["issame"].numpy())
    assert res[0] == o[0] and res[1] == o[1] and res[3] == o[3]
    assert np.array_equal(res[4], o[4]) and np.array_equal(res[5], o[5])
    assert abs(res[2] - o[2]) <= 1e-12 * o[2]


def test_without_landmark_branch_matches_module_path():
    torch.manual_seed(4)
    m = ViT_face_landmark_patch8(loss_type="None", GPU_ID=None, num_class=10, image_size=112, patch_size=8, dim=128, depth=2,
                                 heads=3, mlp_dim=256, dropout=0.1, emb_dropout=0.1, with_land=False, drop_path_rate=0.1)
    attach_arena(m, DEV)
    x = torch.randint(0, 256, (24, 3, 112, 112), dtype=torch.uint8, generator=torch.Generator().manual_seed(5))
    issame = np.arange(12) % 2 == 0
    ev = V.VerificationEvaluator(m, 8, DEV)
    ev.keep_features = True
    assert m.training
    ev(x, issame)
    assert m.training and m._drop_step == 0
    m.eval()
    with torch.no_grad():
        xs = (x.float() / 255.0 - 0.5).to(DEV)
        e0, e1 = m(xs).cpu(), m(xs.flip(3)).cpu()
    assert rel_l2(ev.features[0], e0) < 1e-5 and rel_l2(ev.features[1], e1) < 1e-5, (rel_l2(ev.features[0], e0), rel_l2(ev.features[1], e1))


def _ft_pair_model(seed):
    from conftest import det_fill_random
    torch.manual_seed(seed)
    m = ViT_face_landmark_patch8(loss_type="CosFace", GPU_ID=None, num_class=1000, image_size=112, patch_size=8, dim=128, depth=2,
                                 heads=3, mlp_dim=256, dropout=0.1, emb_dropout=0.1, with_land=True, drop_path_rate=0.1)
    det_fill_random(m.stn); det_fill_random(m.output_layer)
    return m


def _training_state(eng, m):
    """Every device tensor the engine, its arena and its landmark plan hold (one level into dicts), the model's buffers (read without
    the state_dict hook, which would flush num_batches_tracked) and the host counters a later step reads."""
    st = {}
    for name, obj in (("eng", eng), ("arena", eng.arena), ("cnn", eng.cnn)):
        for k, v in vars(obj).items():
            if isinstance(v, torch.Tensor):
                st[f"{name}.{k}"] = v.clone()
            elif isinstance(v, dict):
                st.update({f"{name}.{k}.{kk}": vv.clone() for kk, vv in v.items() if isinstance(vv, torch.Tensor)})
    st.update({"buf." + k: v.clone() for k, v in m.named_buffers()})
    host = dict(micro=eng.micro, since_opt=eng._since_opt, hp=dict(eng._hp), n_forward=eng.cnn.n_forward, cnn_step=eng.cnn.step,
                drop_step=m._drop_step, training=m.training)
    return st, host


def test_evaluation_does_not_perturb_training():
    """An evaluation between two optimizer steps leaves every tensor and counter a later step reads bit-identical.  (Two identical
    engines cannot be compared bit for bit instead: with the landmark branch training, the engine itself is not run-to-run
    deterministic -- its fp32 atomics -- so two runs without any evaluation already differ from the second step on.)"""
    from lafs_cvpr2024_amd.finetune_engine import FinetuneEngine
    B = 8
    g = torch.Generator().manual_seed(9)
    xs = [torch.randint(0, 256, (B, 3, 112, 112), dtype=torch.uint8, generator=g).to(DEV) for _ in range(3)]
    ys = [torch.randint(0, 1000, (B,), generator=g).to(DEV) for _ in range(3)]
    val = torch.randint(0, 256, (20, 3, 112, 112), dtype=torch.uint8, generator=g)
    m = _ft_pair_model(11)
    eng = FinetuneEngine(m, B, acc_step=1, mixup_prob=0.5, device=DEV)
    m.train()
    np.random.seed(3)
    losses = [float(eng.step(xs[0], ys[0], lr=1e-3).item())]
    torch.cuda.synchronize()
    before, host0 = _training_state(eng, m)
    assert len(before) > 40 and any(k.startswith("cnn.") for k in before)
    rng = np.random.get_state()
    res = V.VerificationEvaluator(m, 10, DEV)(val, np.arange(10) % 2 == 0, engine=eng)
    torch.cuda.synchronize()
    after, host1 = _training_state(eng, m)
    assert np.isfinite(res[2]) and 0.0 <= res[0] <= 1.0
    assert host0 == host1, (host0, host1)
    assert all(a == b for a, b in zip(rng[1], np.random.get_state()[1]))        # the mixup draws are not consumed
    bits = lambda t: t.detach().reshape(-1).contiguous().view(torch.uint8)    # (never-written buffers may hold NaN patterns)
    bad = [k for k in before if not torch.equal(bits(before[k]), bits(after[k]))]
    assert not bad, bad
    for k in (1, 2):
        losses.append(float(eng.step(xs[k], ys[k], lr=1e-3).item()))
    assert all(np.isfinite(losses)), losses


def _free_port():
    import socket
    with socket.socket(socket.AF_INET, socket.SOCK_STREAM) as sk:
        sk.bind(("127.0.0.1", 0))
        return sk.getsockname()[1]


def _dp_data():
    g = torch.Generator().manual_seed(31)
    return torch.randint(0, 256, (30, 3, 112, 112), dtype=torch.uint8, generator=g), np.arange(15) % 3 != 0


def _dp_worker(rank, world, port, out):
    os.environ["MASTER_ADDR"], os.environ["MASTER_PORT"] = "127.0.0.1", str(port)
    torch.cuda.set_device(0)
    dist.init_process_group("gloo", rank=rank, world_size=world)
    m = _ft_pair_model(13)
    attach_arena(m, DEV)
    x, issame = _dp_data()
    res = {}
    for B in (10, 30):                             # 3 batches over 2 ranks (1 + 2); 1 batch (rank 0 gets none)
        ev = V.VerificationEvaluator(m, B, DEV)
        r = ev(x, issame)
        res[B] = (ev.last_hist, r[2], r[0])
    torch.save(res, out + f".{rank}")
    dist.barrier()
    dist.destroy_process_group()


def test_two_ranks_give_one_rank_histogram(tmp_path):
    out = str(tmp_path / "ver")
    mp.spawn(_dp_worker, args=(2, _free_port(), out), nprocs=2, join=True)
    r0, r1 = torch.load(out + ".0", weights_only=False), torch.load(out + ".1", weights_only=False)
    m = _ft_pair_model(13)
    attach_arena(m, DEV)
    x, issame = _dp_data()
    for B in (10, 30):
        ev = V.VerificationEvaluator(m, B, DEV)
        r = ev(x, issame)
        for rr in (r0, r1):
            assert np.array_equal(rr[B][0], ev.last_hist)
            assert abs(rr[B][1] - r[2]) <= 1e-12 * r[2] and rr[B][2] == r[0]


def test_train_largescale_with_verification_end_to_end(tmp_path):
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    import make_synthetic_bin
    rec, val, outdir = tmp_path / "rec", tmp_path / "val", tmp_path / "out"
    outdir.mkdir()
    env = dict(os.environ, PYTHONPATH=ROOT)
    subprocess.run([sys.executable, os.path.join(ROOT, "tools", "make_synthetic_rec.py"), str(rec), "8", "8"], check=True, env=env,
                   timeout=120)
    make_synthetic_bin.make(str(val / "lfw.bin"), 30)
    arch = ["--num_class", "32", "--batch_size", "8", "--val_batch_size", "20"]
    cmd = [sys.executable, os.path.join(ROOT, "train_largescale.py"), "--data", "recordio", "--data_path", str(rec), "--epochs", "2",
           "--num_workers", "0", "--val_path", str(val), "--target", "lfw", "--ver_freq", "3", "--outdir", str(outdir)] + arch
    p = subprocess.run(cmd, capture_output=True, text=True, env=env, timeout=900)
    assert p.returncode == 0, p.stdout[-3000:] + p.stderr[-3000:]
    log = p.stdout
    acc = dict(re.findall(r"\[lfw\]\[(\d+)\]Accuracy-Flip: (\S+)", log))
    assert len(re.findall(r"\[lfw\]\[\d+\]XNorm: ", log)) == len(acc) == len(re.findall(r"\[lfw\]\[\d+\]Best-Threshold: ", log)) == 3, log
    assert sorted(int(b) for b in acc) == [9, 12, 15]           # optimizer steps 3, 4, 5 (acc_step 3, divisor max(1, 3 // 3))
    ckpts = sorted(f for f in os.listdir(outdir) if f.endswith("_checkpoint.pth"))
    assert ckpts, log                                           # the first evaluation always improves on highest_acc = 0 (unless 0)
    ck = ckpts[0]
    b = re.search(r"_Batch_(\d+)_", ck).group(1)
    q = subprocess.run([sys.executable, "-m", "lafs_cvpr2024_amd.verification", "--checkpoint", str(outdir / ck), "--val_path", str(val),
                        "--target", "lfw"] + arch, capture_output=True, text=True, env=env, timeout=600, cwd=ROOT)
    assert q.returncode == 0, q.stdout[-3000:] + q.stderr[-3000:]
    got = re.search(r"\[lfw\]\[0\]Accuracy-Flip: (\S+)", q.stdout).group(1)
    assert got == acc[b], (got, acc, q.stdout)
