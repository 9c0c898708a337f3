"""CPU checks of the IJB-B / IJB-C evaluation: the numpy oracle (tests/ijb_oracle.py) against the reference's recorded results
(tests/golden/f22a_ijb_protocol.npz), and the product's host functions (readers, similarity transform, CSR, ROC and table)."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(__file__))
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tools"))

import ijb_oracle as IO  # noqa: E402
import make_synthetic_ijb as syn  # noqa: E402
from conftest import load_golden  # noqa: E402
from lafs_cvpr2024_amd import ijb_evaluation as J  # noqa: E402

SETTINGS = [("", True, True), ("noflip_", False, True), ("nodet_", True, False)]


def f22a():
    fx = {k: (v.numpy() if hasattr(v, "numpy") else v) for k, v in load_golden("f22a_ijb_protocol").items()}
    inputs = syn.protocol_inputs(int(fx["seed"]), int(fx["T"]), int(fx["D"]), int(fx["n_ident"]), float(fx["noise"]))
    assert np.array_equal(inputs[2], fx["templates"]) and np.array_equal(inputs[3], fx["medias"])
    assert np.array_equal(inputs[4], fx["p1"]) and np.array_equal(inputs[5], fx["p2"]) and np.array_equal(inputs[6], fx["label"])
    return fx, inputs


@pytest.mark.parametrize("tag,flip,det", SETTINGS)
def test_oracle_protocol_reproduces_the_reference(tag, flip, det):
    fx, (feats, faceness, templates, medias, p1, p2, label) = f22a()
    scores, sums, uq = IO.protocol(feats, faceness, templates, medias, p1, p2, flip, det)
    assert np.array_equal(uq, fx[tag + "uq"])
    assert sums.dtype == np.float32 and np.array_equal(sums, fx[tag + "sums"])
    err = float(np.abs(scores - fx[tag + "scores"]).max())
    print(f"[F22a {tag or 'default'}] oracle scores max abs error {err:.2e}")
    assert err <= 1e-12
    for roc, tar in ((IO.roc_points, IO.tar_at_far), (J.roc_points, J.tar_at_far)):
        fpr, tpr = roc(label, scores)
        assert np.array_equal(fpr, fx[tag + "fpr"]) and np.array_equal(tpr, fx[tag + "tpr"])
        idx, _, cells = tar(fpr, tpr)
        assert np.array_equal(idx, fx[tag + "idx"]) and cells == list(fx[tag + "table"])
    assert len(set(fx[tag + "table"])) > 1


def test_roc_points_with_tied_scores():
    fx, _ = f22a()
    assert len(np.unique(fx["tie_scores"])) < len(fx["tie_scores"]) // 10
    for roc in (IO.roc_points, J.roc_points):
        fpr, tpr = roc(fx["label"], fx["tie_scores"])
        assert np.array_equal(fpr, fx["tie_fpr"]) and np.array_equal(tpr, fx["tie_tpr"])


def test_roc_points_rejects_bad_input():
    with pytest.raises(ValueError):
        J.roc_points([1, 1, 1], [0.1, 0.2, 0.3])
    with pytest.raises(ValueError):
        J.roc_points([1, 0], [0.1, float("nan")])
    with pytest.raises(ValueError):
        J.roc_points([1, 0, 1], [0.1, 0.2])


def test_tar_at_far_tie_takes_the_lowest_reversed_index():
    fpr = np.array([0.0, 0.0, 0.2, 0.2, 1.0])
    tpr = np.array([0.0, 0.5, 0.6, 0.9, 1.0])
    idx, t, cells = J.tar_at_far(fpr, tpr, [0.1, 0.2, 1e-6])
    # reversed fpr: [1, .2, .2, 0, 0]; |fpr - 0.1| ties between .2 and 0 -> the first .2 (reversed index 1, tpr .9)
    assert list(idx) == [1, 1, 3] and list(t) == [0.9, 0.9, 0.5] and cells == ["90.00", "90.00", "50.00"]


# ----------------------------------------------------------------------------------------------------------------- Umeyama
def _transform(th, s, t, pts):
    R = np.array([[np.cos(th), -np.sin(th)], [np.sin(th), np.cos(th)]])
    return pts @ (s * R).T + t, np.hstack([s * R, np.asarray(t, float)[:, None]])


@pytest.mark.parametrize("fn", [J.similarity_from_landmarks, IO.similarity])
def test_similarity_recovers_a_known_transform(fn):
    src = np.array([[30.5, 41.0], [90.25, 44.0], [61.0, 80.0], [38.0, 110.5], [85.0, 113.0]])
    dst, M = _transform(0.37, 0.61, [12.5, -7.25], src)
    fwd, inv = fn(src, dst)
    assert np.abs(fwd - M).max() < 1e-9
    back = dst @ inv[:, :2].T + inv[:, 2]
    assert np.abs(back - src).max() < 1e-9


def test_similarity_default_target_is_the_shifted_arcface_template():
    assert J.ARCFACE_SRC.dtype == np.float32 and np.array_equal(J.ARCFACE_SRC, IO.ARCFACE_SRC)
    assert J.ARCFACE_SRC[0, 0] == np.float32(30.2946) + np.float32(8.0)
    fwd, _ = J.similarity_from_landmarks(J.ARCFACE_SRC)
    assert np.abs(fwd - np.array([[1.0, 0, 0], [0, 1.0, 0]])).max() < 1e-9


def test_similarity_of_mirrored_points_is_a_proper_rotation():
    src = np.array(J.ARCFACE_SRC, dtype=np.float64)
    mirrored = src * [-1.0, 1.0] + [112.0, 0.0]
    fwd, _ = J.similarity_from_landmarks(mirrored)
    A = fwd[:, :2]
    assert np.linalg.det(A) > 0
    s = np.sqrt(np.linalg.det(A))
    assert np.abs(A.T @ A - s * s * np.eye(2)).max() < 1e-9


def test_similarity_is_a_least_squares_minimum_and_agrees_with_the_oracle():
    rng = np.random.RandomState(3)
    for k in range(5):
        src = syn.landmarks(k) + rng.randn(5, 2) * 2.0
        fwd, inv = J.similarity_from_landmarks(src)
        fo, io = IO.similarity(src)
        assert np.abs(fwd - fo).max() < 1e-9 and np.abs(inv - io).max() < 1e-9
        a, b, tx, ty = fwd[0, 0], fwd[1, 0], fwd[0, 2], fwd[1, 2]
        assert abs(fwd[1, 1] - a) < 1e-12 and abs(fwd[0, 1] + b) < 1e-12
        r0 = IO.residual(fwd, src)
        for i in range(4):
            for e in (1e-4, -1e-4):
                q = [a, b, tx, ty]
                q[i] += e
                M = np.array([[q[0], -q[1], q[2]], [q[1], q[0], q[3]]])
                assert IO.residual(M, src) > r0


def test_similarity_rejects_degenerate_landmarks():
    with pytest.raises(ValueError):
        J.similarity_from_landmarks(np.ones((5, 2)))
    with pytest.raises(ValueError):
        J.similarity_from_landmarks(np.zeros((68, 2)))
    with pytest.raises(ValueError):
        J.similarity_from_landmarks(np.full((5, 2), np.nan))


# ----------------------------------------------------------------------------------------------------------------- readers, CSR
def test_readers_round_trip_the_synthetic_tree(tmp_path):
    ds = syn.make(str(tmp_path), 24, "ijbb")
    meta = J.read_meta(str(tmp_path), "IJBB")
    assert meta["names"][0] == "1.png" and len(meta["names"]) == 24
    assert np.array_equal(meta["templates"], ds["tid"]) and np.array_equal(meta["medias"], ds["mid"])
    assert np.array_equal(meta["p1"], ds["p1"]) and np.array_equal(meta["p2"], ds["p2"]) and np.array_equal(meta["label"], ds["label"])
    assert meta["landmarks"].dtype == np.float32 and np.array_equal(meta["landmarks"], ds["lmk"].astype(np.float32))
    assert np.array_equal(meta["faceness"], ds["faceness"].astype(np.float32))
    with pytest.raises(ValueError):
        J.read_meta(str(tmp_path), "LFW")
    with pytest.raises(FileNotFoundError):
        J.read_meta(str(tmp_path), "IJBC")


def test_readers_reject_malformed_files(tmp_path):
    syn.make(str(tmp_path), 8, "ijbc")
    meta = tmp_path / "meta"
    good = {f: (meta / f).read_text() for f in os.listdir(meta)}

    def broken(name, text):
        for f, t in good.items():
            (meta / f).write_text(t)
        (meta / name).write_text(text)
        with pytest.raises(ValueError):
            J.read_meta(str(tmp_path), "IJBC")

    tm, pl, ls = "ijbc_face_tid_mid.txt", "ijbc_template_pair_label.txt", "ijbc_name_5pts_score.txt"
    broken(tm, good[tm] + "9.png 1\n")                                 # a column short
    broken(tm, good[tm].replace(" 907 ", " x907 ", 1))                 # not an integer
    broken(tm, "\n".join(good[tm].splitlines()[:-1]) + "\n")           # one image fewer than the landmark file
    broken(pl, good[pl] + "1 2 3 4\n")
    broken(pl, good[pl] + "907 13 2\n")                                # a label that is neither 0 nor 1
    broken(pl, "")
    broken(ls, good[ls] + "9.png 1 2 3 0.5\n")
    broken(ls, good[ls].replace("1.png ", "1.png nan ", 1).replace(" 0.", " ", 1))
    first = good[ls].splitlines()[0].split()
    broken(ls, " ".join(first[:1] + ["inf"] + first[2:]) + "\n" + "\n".join(good[ls].splitlines()[1:]) + "\n")
    for f, t in good.items():
        (meta / f).write_text(t)
    J.read_meta(str(tmp_path), "IJBC")


def test_csr_lists_every_image_once_in_the_reference_order():
    fx, (_, _, templates, medias, _, _, _) = f22a()
    order, media_start, template_start, uq = J.build_csr(templates, medias)
    assert order.dtype == media_start.dtype == template_start.dtype == np.int32
    assert np.array_equal(np.sort(order), np.arange(len(templates)))
    assert np.array_equal(uq, np.unique(templates))
    assert media_start[0] == 0 and media_start[-1] == len(templates) and np.all(np.diff(media_start) > 0)
    assert template_start[0] == 0 and template_start[-1] == len(media_start) - 1 and np.all(np.diff(template_start) > 0)
    for ti, t in enumerate(uq):                                        # image2template_feature's own visiting order
        (ind_t,) = np.where(templates == t)
        segs = range(template_start[ti], template_start[ti + 1])
        ums = np.unique(medias[ind_t])
        assert len(segs) == len(ums)
        for mi, u in zip(segs, ums):
            assert np.array_equal(order[media_start[mi]:media_start[mi + 1]], ind_t[medias[ind_t] == u])


def test_unknown_template_id_raises():
    uq = np.array([3, 10, 42])
    assert list(J.template_rows(uq, [42, 3, 10, 3])) == [2, 0, 1, 0]
    for bad in ([3, 11], [100], [-5]):
        with pytest.raises(ValueError):
            J.template_rows(uq, bad)


def test_per_image_normalisation_is_refused():
    with pytest.raises(NotImplementedError):
        J.protocol(np.zeros((2, 4), np.float32), np.ones(2, np.float32), [1, 2], [1, 1], [1], [2], use_norm_score=False)


def test_oracle_alignment_identity_and_border():
    img = syn.crop(3, 1)
    H, W = img.shape[:2]
    out = IO.align(img, [1, 0, 0, 0, 1, 0])
    assert np.array_equal(out, img[:112, :112].transpose(2, 0, 1))
    out = IO.align(img, [1, 0, W - 50, 0, 1, H - 40])                  # most of the window lies outside: border value 0
    assert np.array_equal(out[:, :40, :50], img[H - 40:, W - 50:].transpose(2, 0, 1)) and not out[:, 40:, :].any() and not out[:, :, 50:].any()
    half = IO.align(img, [1, 0, -0.5, 0, 1, 0])                        # half a pixel: the mean of two neighbours, ties to even
    exp = np.rint((np.concatenate([np.zeros((H, 1, 3)), img[:, :-1]], 1).astype(np.float32) + img) * np.float32(0.5))
    assert np.array_equal(half, exp[:112, :112].astype(np.uint8).transpose(2, 0, 1))


def test_table_row_is_plain_text():
    txt = J.table_row("ijbc", "IJBC", ["1.00", "2.00", "3.00", "4.00", "5.00", "97.58"])
    head, row = txt.splitlines()
    assert [c.strip() for c in head.split("|")] == ["Methods", "1e-06", "1e-05", "0.0001", "0.001", "0.01", "0.1"]
    assert [c.strip() for c in row.split("|")] == ["ijbc-IJBC", "1.00", "2.00", "3.00", "4.00", "5.00", "97.58"]
