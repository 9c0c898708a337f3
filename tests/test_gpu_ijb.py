"""GPU tests of the IJB-B / IJB-C evaluation (csrc/ijb.hip, lafs_cvpr2024_amd/ijb_evaluation.py) against the numpy oracle
(tests/ijb_oracle.py) and the reference's recorded results (tests/golden/f22a_ijb_protocol.npz, f22b_ijb_partfvit.npz)."""
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(__file__))
pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tools"))

import ijb_oracle as IO  # noqa: E402
import make_synthetic_ijb as syn  # noqa: E402
from conftest import det_fill, load_golden, sub  # noqa: E402
from lafs_cvpr2024_amd import ijb_evaluation as J  # noqa: E402
from lafs_cvpr2024_amd.face_pre_pro.ViT_face import ViT_face_landmark_patch8  # noqa: E402
from lafs_cvpr2024_amd.ops import _p, call  # noqa: E402
from lafs_cvpr2024_amd.verification import NORMS  # noqa: E402
from lafs_cvpr2024_amd.vision_transformer import attach_arena  # noqa: E402

DEV = "cuda"
SETTINGS = [("", True, True), ("noflip_", False, True), ("nodet_", True, False)]


def rel_l2(a, b):
    a, b = torch.as_tensor(a).double().cpu(), torch.as_tensor(b).double().cpu()
    return ((a - b).norm() / (b.norm() + 1e-30)).item()


def f22a():
    fx = {k: (v.numpy() if hasattr(v, "numpy") else v) for k, v in load_golden("f22a_ijb_protocol").items()}
    return fx, syn.protocol_inputs(int(fx["seed"]), int(fx["T"]), int(fx["D"]), int(fx["n_ident"]), float(fx["noise"]))


# ----------------------------------------------------------------------------------------------------------------- kernel 1
def align_on_device(imgs, maps, norm="reference", S=112):
    B = len(imgs)
    sizes = np.array([im.size for im in imgs], dtype=np.int64)
    offs = np.r_[0, np.cumsum(sizes)]
    src = torch.from_numpy(np.concatenate([im.reshape(-1) for im in imgs])).to(DEV)
    d_off = torch.from_numpy(offs[:B].copy()).to(DEV)
    d_hw = torch.tensor([im.shape[:2] for im in imgs], dtype=torch.int32, device=DEV)
    d_map = torch.from_numpy(np.asarray(maps, dtype=np.float32).reshape(B, 6)).to(DEV)
    out = torch.full((2 * B, 3, S, S), float("nan"), device=DEV)
    al = torch.full((B, 3, S, S), 7, device=DEV, dtype=torch.uint8)
    div, mul, add = NORMS[norm]
    call("lafs_ijb_align_flip_normalize", _p(src), int(offs[-1]), _p(d_off), _p(d_hw), _p(d_map), B, S, div, mul, add, _p(out), _p(al))
    torch.cuda.synchronize()
    return out.cpu().numpy(), al.cpu().numpy()


def _maps(kind, n):
    """Inverse maps (output pixel -> source pixel) of each case for images 0..n-1."""
    out = []
    for k in range(n):
        H, W = syn.size(k)
        if kind == "rotation":
            th = np.deg2rad(10.0 + 7 * k)
            c, s = np.cos(th), np.sin(th)
            out.append([c, -s, W / 2 - 56 * c + 56 * s, s, c, H / 2 - 56 * s - 56 * c])
        elif kind == "scale":
            z = 0.7 + 0.13 * k
            out.append([z, 0, 3.25 + k, 0, z, 1.5 + 2 * k])
        elif kind == "border":                                    # the window leaves the image on every side, partly or wholly
            out.append([1.9, 0.3, -40.5 - 30 * k, -0.2, 2.1, -35.25 + 100 * k])
        else:                                                     # the landmark transform the evaluator uses
            out.append(J.similarity_from_landmarks(syn.landmarks(k).astype(np.float32))[1].reshape(-1))
    return np.asarray(out, dtype=np.float32)


@pytest.mark.parametrize("kind,n,norm", [("rotation", 5, "reference"), ("scale", 5, "train"), ("border", 4, "reference"),
                                         ("landmarks", 1, "reference"), ("landmarks", 64, "reference")])
def test_align_equals_the_float32_oracle_on_every_pixel(kind, n, norm):
    imgs = [syn.crop(k, k % 8) for k in range(n)]
    assert n == 1 or len({im.shape for im in imgs}) > 1
    maps = _maps(kind, n)
    out, al = align_on_device(imgs, maps, norm)
    x_ref, al_ref = IO.align_flip_normalize(imgs, maps, norm=norm)
    if kind == "border":
        assert any(not a.any() for a in al_ref) and any(a.any() and not a[:, 0, 0].any() for a in al_ref)
    else:
        assert all(a.any() for a in al_ref)
    assert np.array_equal(al, al_ref), int((al != al_ref).sum())
    assert np.array_equal(out, x_ref)
    assert np.array_equal(out[n:], out[:n][..., ::-1])


def test_align_identity_map_returns_the_image():
    imgs = [syn.crop(k, k) for k in (2, 9)]
    out, al = align_on_device(imgs, [[1, 0, 0, 0, 1, 0], [1, 0, 5, 0, 1, 3]])
    assert np.array_equal(al[0], imgs[0][:112, :112].transpose(2, 0, 1))
    assert np.array_equal(al[1], imgs[1][3:115, 5:117].transpose(2, 0, 1))
    ref = torch.from_numpy(al).float() / 255.0 - 0.5
    assert torch.equal(torch.from_numpy(out[:2]), ref)


def test_align_refuses_an_image_outside_the_buffer():
    """An offset / size that would read past the packed buffer gives a zero image, not a read out of bounds."""
    img = syn.crop(1, 1)
    src = torch.from_numpy(img.reshape(-1).copy()).to(DEV)
    d_off = torch.tensor([0, 64], dtype=torch.int64, device=DEV)
    d_hw = torch.tensor([img.shape[:2], img.shape[:2]], dtype=torch.int32, device=DEV)
    d_map = torch.tensor([[1, 0, 0, 0, 1, 0]] * 2, dtype=torch.float32, device=DEV)
    out = torch.empty(4, 3, 112, 112, device=DEV)
    al = torch.full((2, 3, 112, 112), 7, device=DEV, dtype=torch.uint8)
    call("lafs_ijb_align_flip_normalize", _p(src), img.size, _p(d_off), _p(d_hw), _p(d_map), 2, 112, 255.0, 1.0, -0.5, _p(out), _p(al))
    torch.cuda.synchronize()
    assert np.array_equal(al[0].cpu().numpy(), img[:112, :112].transpose(2, 0, 1)) and not al[1].any()


# ----------------------------------------------------------------------------------------------------------------- kernels 2, 3
def pool_on_device(feats, faceness, templates, medias, flip, det):
    order, ms, ts, uq = J.build_csr(templates, medias)
    N, D, T = feats.shape[0], feats.shape[1] // 2, len(uq)
    d_feats, d_face, d_order, d_ms, d_ts = (torch.from_numpy(np.ascontiguousarray(a)).to(DEV) for a in (feats, faceness, order, ms, ts))
    sums = torch.full((T, D), float("nan"), device=DEV)
    unit = torch.full((T, D), float("nan"), device=DEV, dtype=torch.float64)
    call("lafs_ijb_template_pool", _p(d_feats), 2 * D, _p(d_face), N, _p(d_order), _p(d_ms), len(ms) - 1, _p(d_ts), T, D,
         int(flip), int(det), _p(sums), _p(unit))
    torch.cuda.synchronize()
    return sums.cpu().numpy(), unit.cpu().numpy(), uq


@pytest.mark.parametrize("tag,flip,det", SETTINGS)
def test_template_pool_sums_are_bit_equal_to_the_reference(tag, flip, det):
    fx, (feats, faceness, templates, medias, _, _, _) = f22a()
    sums, unit, uq = pool_on_device(feats, faceness, templates, medias, flip, det)
    assert np.array_equal(uq, fx[tag + "uq"])
    assert np.array_equal(sums, fx[tag + "sums"])
    ref = IO.unit_rows(fx[tag + "sums"])
    err = float(np.abs(unit - ref).max())
    print(f"[F22a {tag or 'default'}] unit rows max abs error {err:.2e}")
    assert err <= 1e-13


def test_template_pool_at_the_widest_row_and_a_zero_row():
    """D = 1024 (four columns per thread), D = 1000 (a masked tail), and a template whose rows cancel: it stays zero."""
    rng = np.random.RandomState(5)
    for D in (1024, 1000):
        N = 60
        feats = rng.randn(N, 2 * D).astype(np.float32)
        templates = rng.randint(0, 7, N) * 1000 + 3
        medias = rng.randint(0, 4, N)
        zt = templates == templates[0]
        feats[zt, D:] = -feats[zt, :D]
        faceness = rng.uniform(0.2, 1, N).astype(np.float32)
        sums, unit, uq = pool_on_device(feats, faceness, templates, medias, True, True)
        s_ref, uq_ref = IO.template_sums(feats, faceness, templates, medias)
        assert np.array_equal(uq, uq_ref) and np.array_equal(sums, s_ref)
        z = int(np.searchsorted(uq, templates[0]))
        assert not sums[z].any() and not unit[z].any()
        assert float(np.abs(unit - IO.unit_rows(s_ref)).max()) <= 1e-13


@pytest.mark.parametrize("tag,flip,det", SETTINGS)
def test_pair_scores_and_protocol_against_the_reference(tag, flip, det):
    fx, (feats, faceness, templates, medias, p1, p2, label) = f22a()
    uq = fx[tag + "uq"]
    unit = torch.from_numpy(IO.unit_rows(fx[tag + "sums"])).to(DEV)
    i1, i2 = (torch.from_numpy(J.template_rows(uq, p)).to(DEV) for p in (p1, p2))
    out = torch.full((len(p1),), float("nan"), device=DEV, dtype=torch.float64)
    call("lafs_ijb_pair_scores", _p(unit), len(uq), unit.shape[1], _p(i1), _p(i2), len(p1), _p(out))
    torch.cuda.synchronize()
    err = float(np.abs(out.cpu().numpy() - fx[tag + "scores"]).max())
    print(f"[F22a {tag or 'default'}] pair scores max abs error {err:.2e}")
    assert err <= 1e-12
    # the whole protocol through the public function
    scores, sums, uq2 = J.protocol(feats, faceness, templates, medias, p1, p2, flip, det, device=DEV)
    assert np.array_equal(uq2, uq) and np.array_equal(sums, fx[tag + "sums"])
    assert float(np.abs(scores - fx[tag + "scores"]).max()) <= 1e-12
    fpr, tpr = J.roc_points(label, scores)
    assert np.array_equal(fpr, fx[tag + "fpr"]) and np.array_equal(tpr, fx[tag + "tpr"])
    idx, _, cells = J.tar_at_far(fpr, tpr)
    assert np.array_equal(idx, fx[tag + "idx"]) and cells == list(fx[tag + "table"])


def test_pair_scores_odd_width_and_bad_index():
    rng = np.random.RandomState(6)
    unit = rng.randn(9, 37)
    i1 = np.array([0, 3, 8, 2, 9, -1], dtype=np.int32)
    i2 = np.array([1, 3, 0, 7, 0, 2], dtype=np.int32)
    d_unit, d_i1, d_i2 = (torch.from_numpy(a).to(DEV) for a in (unit, i1, i2))
    out = torch.zeros(6, device=DEV, dtype=torch.float64)
    call("lafs_ijb_pair_scores", _p(d_unit), 9, 37, _p(d_i1), _p(d_i2), 6, _p(out))
    torch.cuda.synchronize()
    o = out.cpu().numpy()
    assert float(np.abs(o[:4] - np.sum(unit[i1[:4]] * unit[i2[:4]], -1)).max()) <= 1e-12
    assert np.isnan(o[4]) and np.isnan(o[5])


def test_protocol_rejects_an_unknown_template():
    fx, (feats, faceness, templates, medias, p1, p2, _) = f22a()
    bad = p1.copy()
    bad[5] = templates.max() + 1
    with pytest.raises(ValueError):
        J.protocol(feats, faceness, templates, medias, bad, p2, device=DEV)


# ----------------------------------------------------------------------------------------------------------------- the model
def _f13_model():
    fx = load_golden("f13_partfvit_land")
    m = ViT_face_landmark_patch8(loss_type="None", GPU_ID=None, num_class=10, image_size=112, patch_size=8, dim=128, depth=2,
                                 heads=3, mlp_dim=256, dropout=0.0, emb_dropout=0.0, with_land=True)
    det_fill(m.stn); det_fill(m.output_layer)
    m.load_state_dict(sub(fx, "p."), strict=False)
    attach_arena(m, DEV)
    m.eval()
    return m


def test_f22b_partfvit_end_to_end_against_reference():
    fx = {k: (v.numpy() if hasattr(v, "numpy") else v) for k, v in load_golden("f22b_ijb_partfvit").items()}
    n = int(fx["n"])
    ds, imgs = syn.dataset(n), syn.images(n)
    assert np.array_equal(ds["sizes"], fx["sizes"]) and np.array_equal(ds["lmk"], fx["lmk"]) and np.array_equal(ds["tid"], fx["tid"])
    assert np.array_equal(ds["mid"], fx["mid"]) and np.array_equal(ds["p1"], fx["p1"]) and np.array_equal(ds["p2"], fx["p2"])
    lmk = ds["lmk"].astype(np.float32)
    ev = J.IJBEvaluator(_f13_model(), 16, DEV)                    # 40 images: two full batches and a short one
    ev.keep_aligned = True
    feats = ev.features(imgs, lmk).cpu().numpy()
    al_ref = np.stack([IO.align(im, J.similarity_from_landmarks(l)[1]) for im, l in zip(imgs, lmk)])
    assert np.array_equal(ev.aligned.numpy(), al_ref)
    print(f"[F22b] aligned crops differing from the fixture's in {int((al_ref.reshape(n, -1).sum(1) != fx['aligned_sum']).sum())} of {n} images")
    D = feats.shape[1] // 2
    errs = [rel_l2(feats[:, :D], fx["emb"][:, :D]), rel_l2(feats[:, D:], fx["emb"][:, D:])]
    print(f"[F22b] per-copy embeddings rel-L2 {errs[0]:.2e} / {errs[1]:.2e}")
    assert max(errs) < 2e-2, errs
    scores, sums, uq = J.protocol(feats, fx["faceness"], ds["tid"], ds["mid"], ds["p1"], ds["p2"], device=DEV)
    o_scores, o_sums, o_uq = IO.protocol(feats, fx["faceness"], ds["tid"], ds["mid"], ds["p1"], ds["p2"])
    assert np.array_equal(uq, o_uq) and np.array_equal(uq, fx["uq"]) and np.array_equal(sums, o_sums)
    assert float(np.abs(scores - o_scores).max()) <= 1e-12
    print(f"[F22b] scores against the reference's: max abs {float(np.abs(scores - fx['scores']).max()):.2e}; table "
          f"{J.tar_at_far(*J.roc_points(ds['label'], scores))[2]} (reference {list(fx['table'])})")


def test_evaluation_leaves_the_model_untouched():
    torch.manual_seed(4)
    m = ViT_face_landmark_patch8(loss_type="None", GPU_ID=None, num_class=10, image_size=112, patch_size=8, dim=128, depth=2,
                                 heads=3, mlp_dim=256, dropout=0.1, emb_dropout=0.1, with_land=False, drop_path_rate=0.1)
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
    assert before.keys() == after.keys() and all(torch.equal(before[k], after[k]) for k in before)
    m.eval()
    with torch.no_grad():
        xs = (ev.aligned.float() / 255.0 - 0.5).to(DEV)
        e0, e1 = m(xs).cpu(), m(xs.flip(3)).cpu()
    D = e0.shape[1]
    assert rel_l2(feats[:, :D], e0) < 1e-5 and rel_l2(feats[:, D:], e1) < 1e-5, (rel_l2(feats[:, :D], e0), rel_l2(feats[:, D:], e1))


def test_module_entry_point_on_the_synthetic_tree(tmp_path):
    tree, res = tmp_path / "ijb", tmp_path / "res"
    env = dict(os.environ, PYTHONPATH=ROOT)
    subprocess.run([sys.executable, os.path.join(ROOT, "tools", "make_synthetic_ijb.py"), str(tree), "24"], check=True, env=env, timeout=120)
    from lafs_cvpr2024_amd import train_largescale as tl
    arch = ["--num_class", "32"]
    torch.manual_seed(7)
    backbone = tl.build_backbone(tl.get_args_parser().parse_args(arch))
    ckpt = tmp_path / "ckpt.pth"
    torch.save({"module." + k: v for k, v in backbone.state_dict().items()}, ckpt)
    del backbone
    feats = tmp_path / "feats.npz"
    cmd = [sys.executable, os.path.join(ROOT, "IJB_evaluation.py"), "--checkpoint", str(ckpt), "--image_path", str(tree), "--target", "IJBC",
           "--result_dir", str(res), "--job", "synthetic", "--batch_size", "10", "--save_features", str(feats)] + arch
    p = subprocess.run(cmd, capture_output=True, text=True, env=env, timeout=900, cwd=str(tmp_path))
    assert p.returncode == 0, p.stdout[-3000:] + p.stderr[-3000:]
    scores = np.load(res / "synthetic" / "ijbc.npy")
    ds = syn.dataset(24)
    assert scores.shape == (len(ds["label"]),) and scores.dtype == np.float64 and np.all(np.abs(scores) <= 1 + 1e-12)
    lines = [l for l in p.stdout.splitlines() if "|" in l]
    assert len(lines) == 2 and lines[0].startswith("Methods") and lines[1].startswith("ijbc-IJBC"), p.stdout
    cells = [c.strip() for c in lines[1].split("|")][1:]
    assert cells == J.tar_at_far(*J.roc_points(ds["label"], scores))[2]
    # the protocol alone from the saved features gives the same file
    q = subprocess.run([sys.executable, "-m", "lafs_cvpr2024_amd.ijb_evaluation", "--features", str(feats), "--image_path", str(tree),
                        "--target", "IJBC", "--result_dir", str(res), "--job", "again"], capture_output=True, text=True, env=env,
                       timeout=600, cwd=ROOT)
    assert q.returncode == 0, q.stdout[-3000:] + q.stderr[-3000:]
    assert np.array_equal(np.load(res / "again" / "ijbc.npy"), scores)
