#!/usr/bin/env python3
"""Write a small synthetic tree in the layout IJB_evaluation.py reads (reference IJB_evaluation.py:669-703):

    <dir>/loose_crop/<k>.png                 loose crops of differing sizes
    <dir>/meta/ijbc_face_tid_mid.txt         name tid mid
    <dir>/meta/ijbc_template_pair_label.txt  tid1 tid2 label
    <dir>/meta/ijbc_name_5pts_score.txt      name x1 y1 ... x5 y5 faceness
    <dir>/meta/ijbc_1N_gallery_G1.csv        TEMPLATE_ID,SUBJECT_ID,FILENAME per image: templates 0-3
    <dir>/meta/ijbc_1N_gallery_G2.csv        the same for templates 4-7
    <dir>/meta/ijbc_1N_probe_mixed.csv       templates 8-15, and one row whose subject is in neither gallery

for end-to-end runs of `python -m lafs_cvpr2024_amd.ijb_evaluation`.  Everything comes from closed forms of the image index (no random
state), so the tests and the fixture generator rebuild the same images instead of committing them.
usage: tools/make_synthetic_ijb.py DIR [images] [ijbc|ijbb]"""
import os
import sys

import numpy as np

ARCFACE = np.array([[38.2946, 51.6963], [73.5318, 51.5014], [56.0252, 71.7366], [41.5493, 92.3655], [70.7299, 92.2041]])
N_TEMPLATES = 16
# sparse, unsorted template ids; templates j and j + 8 show the same identity
TIDS = np.array([907, 13, 402, 77, 5120, 230, 1999, 64, 3001, 12, 868, 4410, 31, 2750, 555, 1203])


def size(k):
    return 120 + (k * 37) % 81, 120 + (k * 53 + 11) % 81            # (H, W) in 120 .. 200


def crop(k, ident):
    """uint8 [H, W, 3]: a smooth pattern of the identity plus a small deterministic texture of the image."""
    H, W = size(k)
    yy, xx = np.mgrid[0:H, 0:W].astype(np.float64)
    u, v = xx * (112.0 / W), yy * (112.0 / H)
    base = np.stack([127 + 90 * np.sin(u / (5.0 + ident % 7) + c) * np.cos(v / (6.0 + c) - ident) for c in range(3)], -1)
    tex = ((xx * 73 + yy * 151 + k * 31) % 13 - 6)[..., None] + np.arange(3) * ((k % 3) - 1)
    return np.clip(base + tex, 0, 255).astype(np.uint8)


def landmarks(k):
    """Five points [5, 2] (x, y): the ArcFace template under a rotation, a scale and a shift into the crop, slightly perturbed,
    rounded to the three decimals the meta file keeps."""
    H, W = size(k)
    th = np.deg2rad(((k * 7) % 31) - 15.0)
    s = min(H, W) / 112.0 * (0.8 + 0.05 * (k % 5))
    R = np.array([[np.cos(th), -np.sin(th)], [np.sin(th), np.cos(th)]])
    centre = np.array([W / 2.0 + (k % 7) - 3.0, H / 2.0 + (k % 5) - 2.0])
    wobble = np.stack([np.sin(np.arange(5) * 1.3 + k), np.cos(np.arange(5) * 0.7 - k)], 1) * 0.8
    return np.round((ARCFACE - 56.0) @ R.T * s + centre + wobble, 3)


def dataset(n=40):
    """-> dict(sizes [n,2], ident [n], lmk [n,5,2], faceness [n], tid [n], mid [n], p1, p2, label)."""
    k = np.arange(n)
    tj = k % N_TEMPLATES
    ident = tj % 8
    mid = np.where(k < N_TEMPLATES, 100 + k, 300 + tj)           # a template's later images share one media
    faceness = np.round(0.55 + 0.45 * np.abs(np.sin(k * 0.9 + 0.3)), 4)
    used = np.unique(tj)
    a, b = np.triu_indices(len(used), 1)
    p1, p2 = TIDS[used[a]], TIDS[used[b]]
    swap = (a + b) % 2 == 1                                       # either order occurs
    p1, p2 = np.where(swap, p2, p1), np.where(swap, p1, p2)
    label = (used[a] % 8 == used[b] % 8).astype(np.int64)
    return dict(sizes=np.array([size(i) for i in k]), ident=ident, lmk=np.stack([landmarks(i) for i in k]), faceness=faceness,
                tid=TIDS[tj], mid=mid, p1=p1, p2=p2, label=label)


SUBJECTS = 1000 + 7 * np.arange(8)                                # subject id of identity 0 .. 7
UNKNOWN_SUBJECT = 9999


def identification_lists(n=40):
    """The 1:N lists over the templates that have images among the first n: G1 = templates 0-3, G2 = templates 4-7, probes = templates
    8-15 (template j + 8 shows the identity of template j) plus template 0 under a subject that neither gallery holds.
    -> dict(g1_tids, g1_sids, g2_tids, g2_sids, probe_tids, probe_sids), one entry per template."""
    used = np.unique(np.arange(n) % N_TEMPLATES)
    pick = lambda lo, hi: used[(used >= lo) & (used < hi)]
    g1, g2, pr = pick(0, 4), pick(4, 8), pick(8, 16)
    extra = used[:1] if len(pr) else used[:0]
    return dict(g1_tids=TIDS[g1], g1_sids=SUBJECTS[g1 % 8], g2_tids=TIDS[g2], g2_sids=SUBJECTS[g2 % 8],
                probe_tids=np.r_[TIDS[pr], TIDS[extra]], probe_sids=np.r_[SUBJECTS[pr % 8], [UNKNOWN_SUBJECT] * len(extra)])


def images(n=40):
    ds = dataset(n)
    return [crop(i, int(ds["ident"][i])) for i in range(n)]


def protocol_inputs(seed=22, T=96, D=384, n_ident=32, noise=9.0):
    """Seeded image features for the protocol alone (fixture F22a; the tests rebuild them from the stored arguments): T templates with
    sparse unsorted ids over n_ident identities, media of 1 and of 3 or more images, one single-image template, every unordered
    template pair once.  -> (img_feats f32 [N, 2D], faceness, templates, medias, p1, p2, label)."""
    rng = np.random.RandomState(seed)
    tids = rng.choice(100000, T, replace=False)
    sizes = np.r_[1, rng.randint(2, 31, T - 1)]
    t_of, m_of = [], []
    for j in range(T):
        t_of += [tids[j]] * sizes[j]
        m_of += list(5000 + rng.randint(0, sizes[j] // 3 + 1, sizes[j]))
    perm = rng.permutation(len(t_of))
    templates, medias = np.array(t_of)[perm], np.array(m_of)[perm]
    ident = {tids[j]: j % n_ident for j in range(T)}
    centres = rng.randn(n_ident, D)
    who = np.array([ident[t] for t in templates])
    orig = (centres[who] + noise * rng.randn(len(who), D)).astype(np.float32)
    flipc = (orig + rng.randn(len(who), D)).astype(np.float32)
    img_feats = np.concatenate([orig, flipc], 1)
    faceness = rng.uniform(0.3, 1.0, len(who)).astype(np.float32)
    a, b = np.triu_indices(T, 1)
    swap = rng.rand(len(a)) < 0.5
    a, b = np.where(swap, b, a), np.where(swap, a, b)
    pp = rng.permutation(len(a))
    p1, p2 = tids[a[pp]], tids[b[pp]]
    label = np.array([int(ident[x] == ident[y]) for x, y in zip(p1, p2)])
    return img_feats, faceness, templates, medias, p1, p2, label


def make(root, n=40, target="ijbc"):
    from PIL import Image
    ds = dataset(n)
    os.makedirs(os.path.join(root, "loose_crop"), exist_ok=True)
    os.makedirs(os.path.join(root, "meta"), exist_ok=True)
    names = ["%d.png" % (i + 1) for i in range(n)]
    for i, name in enumerate(names):
        Image.fromarray(crop(i, int(ds["ident"][i]))).save(os.path.join(root, "loose_crop", name), format="PNG")
    with open(os.path.join(root, "meta", target + "_face_tid_mid.txt"), "w") as f:
        for i, name in enumerate(names):
            f.write("%s %d %d\n" % (name, ds["tid"][i], ds["mid"][i]))
    with open(os.path.join(root, "meta", target + "_template_pair_label.txt"), "w") as f:
        for a, b, l in zip(ds["p1"], ds["p2"], ds["label"]):
            f.write("%d %d %d\n" % (a, b, l))
    with open(os.path.join(root, "meta", target + "_name_5pts_score.txt"), "w") as f:
        for i, name in enumerate(names):
            f.write("%s %s %.4f\n" % (name, " ".join("%.3f" % v for v in ds["lmk"][i].reshape(-1)), ds["faceness"][i]))
    ls = identification_lists(n)
    for key, fname in (("g1", "_1N_gallery_G1.csv"), ("g2", "_1N_gallery_G2.csv"), ("probe", "_1N_probe_mixed.csv")):
        with open(os.path.join(root, "meta", target + fname), "w") as f:
            f.write("TEMPLATE_ID,SUBJECT_ID,FILENAME\n")
            for t, sid in zip(ls[key + "_tids"], ls[key + "_sids"]):                 # one row per image, as the dataset's lists have
                for i in np.flatnonzero(ds["tid"] == t):
                    f.write("%d,%d,%s\n" % (t, sid, names[i]))
    return ds


if __name__ == "__main__":
    out = sys.argv[1]
    n = int(sys.argv[2]) if len(sys.argv) > 2 else 40
    tgt = sys.argv[3].lower() if len(sys.argv) > 3 else "ijbc"
    ds = make(out, n, tgt)
    print(f"wrote {n} loose crops, {len(np.unique(ds['tid']))} templates and {len(ds['label'])} pairs to {out}")
