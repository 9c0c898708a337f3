"""IJB-B / IJB-C template verification, TAR@FAR (reference IJB_evaluation.py) on the HIP kernels of csrc/ijb.hip.

    meta files -> per batch of B loose crops: Pillow decode (thread pool) -> one pinned staging buffer -> one H2D copy
      -> lafs_ijb_align_flip_normalize: similarity-aligned 112 x 112 crops, scaled, then the same batch mirrored (f32 [2B,3,112,112])
      -> the extraction of verification.py (frozen CNN plan, theta, patch gather, packed Part-fViT trunk in eval mode)
      -> rows [emb(orig) | emb(flip)] of img_feats f32 [N, 2D], kept on the device
    protocol: lafs_ijb_template_pool (flip sum, faceness weight, media mean, template sum in numpy's float32 order; float64 unit rows)
      -> lafs_ijb_pair_scores (float64 dot product per pair) -> roc_points / tar_at_far on the host -> the reference's table row.

The reference's switches use_norm_score = use_detector_score = use_flip_test = True (:63-65) are the defaults; `flip` and
`detector_score` can be turned off, use_norm_score=False (per-image L2 normalisation, a value the reference hard-codes away) is not
built.  Only the 5-landmark form of Embedding.get is restated: its 68-landmark branch (:202-208) is never reached by the reference's
own file format.  The model is evaluated as backbone.eval() runs it, without touching its state (see verification.py).

1:N identification (`--protocol 1N`): the same pooled rows, searched instead of paired.
    meta/<t>_1N_gallery_G1.csv, _G2.csv, _1N_probe_mixed.csv -> per gallery: lafs_ijb_search (every probe template against every gallery
      template in float64 on the device; top-k, mate score, mate rank and best non-mate per probe; the score matrix is never stored)
      -> cmc (closed-set rank-1/5/10) and tpir_at_fpir (open-set TPIR@FPIR) on the host -> one table row, means over G1 and G2.
The reference stops at 1:1: the 1:N protocol has no counterpart in the reference; metric definitions are this project's, stated in the
docstrings of cmc and tpir_at_fpir; the csv layout is restated from the public IJB-C protocol as remembered: PARITY UNPINNED.

Single process only: data-parallel extraction is out of scope.

Deliberate deviations from the reference:
  * images are decoded with Pillow (the reference uses cv2.imread): PARITY UNPINNED;
  * the alignment is float32 bilinear interpolation with border value 0; cv2.warpAffine works in fixed point on a 1/32 pixel
    coordinate grid, and OpenCV is not available to compare against: PARITY UNPINNED;
  * the similarity transform is Umeyama's closed form restated (skimage.transform.SimilarityTransform.estimate implements the same
    publication; skimage is not available to compare against): PARITY UNPINNED;
  * a pair that names a template id without images raises ValueError (the reference silently scores it with row 0, :548-550);
  * no ROC image is drawn; the table row is printed as plain text;
  * a short last batch is run short (the reference builds a second Embedding for it);
  * at real scale, pair scores a few ulp apart can order differently from the reference's, which can move a TAR by one pair in
    millions.
"""
import argparse
import csv
import math
import os
import time
from concurrent.futures import ThreadPoolExecutor
from fractions import Fraction

import numpy as np

FARS = [10 ** -6, 10 ** -5, 10 ** -4, 10 ** -3, 10 ** -2, 10 ** -1]          # IJB_evaluation.py:795
ARCFACE_SRC = np.array([[30.2946, 51.6963], [65.5318, 51.5014], [48.0252, 71.7366], [33.5493, 92.3655], [62.7299, 92.2041]],
                       dtype=np.float32)
ARCFACE_SRC[:, 0] += 8.0                                                      # :144-150
IMAGE_SIZE = 112
MAX_WORKERS = 16
CMC_RANKS = (1, 5, 10)
FPIRS = (0.01, 0.1)
MAX_TOP_K = 64                                                                # lafs_ijb_search's limit


# ----------------------------------------------------------------------------------------------------------------- readers
def _rows(path, n_cols):
    rows = []
    with open(path) as f:
        for ln, line in enumerate(f, 1):
            parts = line.split()
            if not parts:
                continue
            if len(parts) != n_cols:
                raise ValueError(f"{path}:{ln}: expected {n_cols} columns, got {len(parts)}")
            rows.append(parts)
    if not rows:
        raise ValueError(f"{path}: no rows")
    return rows


def _ints(path, rows, col):
    try:
        return np.array([int(r[col]) for r in rows], dtype=np.int64)
    except ValueError as e:
        raise ValueError(f"{path}: column {col + 1} must hold integers ({e})") from None


def read_template_media_list(path):
    """`name tid mid` per image (:275-280) -> (names, templates int64 [N], medias int64 [N])."""
    rows = _rows(path, 3)
    return [r[0] for r in rows], _ints(path, rows, 1), _ints(path, rows, 2)


def read_template_pair_list(path):
    """`tid1 tid2 label` per pair (:286-294) -> (p1, p2, label) int64 [P]."""
    rows = _rows(path, 3)
    label = _ints(path, rows, 2)
    if np.any((label != 0) & (label != 1)):
        raise ValueError(f"{path}: labels must be 0 or 1")
    return _ints(path, rows, 0), _ints(path, rows, 1), label


def read_landmark_score_list(path):
    """`name x1 y1 ... x5 y5 faceness` per image (:423-428, :455) -> (names, landmarks float32 [N,5,2], faceness float32 [N])."""
    rows = _rows(path, 12)
    try:
        vals = np.array([[float(v) for v in r[1:]] for r in rows], dtype=np.float64)
    except ValueError as e:
        raise ValueError(f"{path}: landmarks and score must be numbers ({e})") from None
    if not np.all(np.isfinite(vals)):
        raise ValueError(f"{path}: landmarks and score must be finite")
    return [r[0] for r in rows], vals[:, :10].astype(np.float32).reshape(-1, 5, 2), vals[:, 10].astype(np.float32)


def read_meta(image_path, target):
    """The three files of <image_path>/meta for target 'IJBC' / 'IJBB' (:669-703), checked against one another."""
    if target not in ("IJBC", "IJBB"):
        raise ValueError("target must be IJBC or IJBB")
    t = target.lower()
    meta = os.path.join(image_path, "meta")
    names_t, templates, medias = read_template_media_list(os.path.join(meta, f"{t}_face_tid_mid.txt"))
    p1, p2, label = read_template_pair_list(os.path.join(meta, f"{t}_template_pair_label.txt"))
    names, lmk, faceness = read_landmark_score_list(os.path.join(meta, f"{t}_name_5pts_score.txt"))
    if len(names) != len(names_t):
        raise ValueError(f"{meta}: {len(names_t)} rows of tid / mid but {len(names)} rows of landmarks")
    return dict(names=names, templates=templates, medias=medias, p1=p1, p2=p2, label=label, landmarks=lmk, faceness=faceness)


def read_template_subject_csv(path):
    """One `*_1N_*.csv` list -> (template ids int64 [T], subject ids int64 [T]), one row per template in order of first appearance.
    Read with the csv module and keyed on the header names TEMPLATE_ID and SUBJECT_ID; other columns are ignored and the column order
    is free.  The files list one row per image, so rows are deduplicated; a template listed with two subjects raises.  The layout is
    restated from the public IJB-C protocol as remembered, UNPINNED: no file of the dataset was available to check it against."""
    if not os.path.isfile(path):
        raise ValueError(f"{path}: no such file")
    seen = {}
    with open(path, newline="") as f:
        rd = csv.DictReader(f)
        names = [n.strip() for n in (rd.fieldnames or [])]
        for col in ("TEMPLATE_ID", "SUBJECT_ID"):
            if col not in names:
                raise ValueError(f"{path}: no column {col} in the header {names}")
        rd.fieldnames = names
        for row in rd:
            try:
                t, sid = int(row["TEMPLATE_ID"]), int(row["SUBJECT_ID"])
            except (TypeError, ValueError):
                raise ValueError(f"{path}:{rd.line_num}: TEMPLATE_ID and SUBJECT_ID must be integers, got "
                                 f"{row['TEMPLATE_ID']!r}, {row['SUBJECT_ID']!r}") from None
            if seen.setdefault(t, sid) != sid:
                raise ValueError(f"{path}:{rd.line_num}: template {t} is listed with subjects {seen[t]} and {sid}")
    if not seen:
        raise ValueError(f"{path}: no rows")
    return np.array(list(seen.keys()), dtype=np.int64), np.array(list(seen.values()), dtype=np.int64)


def read_identification_lists(image_path, target):
    """<image_path>/meta/<t>_1N_gallery_G1.csv, <t>_1N_gallery_G2.csv and <t>_1N_probe_mixed.csv for target 'IJBC' / 'IJBB'
    -> dict(g1_tids, g1_sids, g2_tids, g2_sids, probe_tids, probe_sids).  File names and layout UNPINNED (read_template_subject_csv)."""
    if target not in ("IJBC", "IJBB"):
        raise ValueError("target must be IJBC or IJBB")
    t = target.lower()
    meta = os.path.join(image_path, "meta")
    out = {}
    for key, name in (("g1", f"{t}_1N_gallery_G1.csv"), ("g2", f"{t}_1N_gallery_G2.csv"), ("probe", f"{t}_1N_probe_mixed.csv")):
        out[key + "_tids"], out[key + "_sids"] = read_template_subject_csv(os.path.join(meta, name))
    return out


# ----------------------------------------------------------------------------------------------------------------- geometry
def similarity_from_landmarks(lmk5, dst=ARCFACE_SRC):
    """Least-squares similarity transform (rotation, uniform scale, translation) that maps the 5 landmarks onto `dst`, in float64:
    S. Umeyama, "Least-squares estimation of transformation parameters between two point patterns", IEEE TPAMI 13(4), 1991, with
    scale estimation and the det < 0 reflection fix, as Embedding.get asks of skimage (:211-213).  PARITY UNPINNED against skimage.
    -> (forward 2x3: landmark -> template, inverse 2x3: output pixel -> source pixel)."""
    src, dst = np.asarray(lmk5, dtype=np.float64), np.asarray(dst, dtype=np.float64)
    if src.shape != dst.shape or src.ndim != 2 or src.shape[1] != 2 or src.shape[0] < 2:
        raise ValueError(f"expected two point sets of one shape [n, 2], got {src.shape} and {dst.shape}")
    if not np.all(np.isfinite(src)):
        raise ValueError("landmarks must be finite")
    n = src.shape[0]
    mu_s, mu_d = src.mean(axis=0), dst.mean(axis=0)
    sc, dc = src - mu_s, dst - mu_d
    cov = dc.T @ sc / n
    d = np.ones(2)
    if np.linalg.det(cov) < 0:
        d[1] = -1.0
    U, sv, Vt = np.linalg.svd(cov)
    rank = np.linalg.matrix_rank(cov)
    if rank == 0:
        raise ValueError("degenerate landmarks: all points coincide")
    if rank == 1:
        if np.linalg.det(U) * np.linalg.det(Vt) > 0:
            R = U @ Vt
        else:
            R = U @ np.diag([1.0, -1.0]) @ Vt
            d = np.array([1.0, -1.0])
    else:
        R = U @ np.diag(d) @ Vt
    scale = float(sv @ d) / sc.var(axis=0).sum()
    if not np.isfinite(scale) or scale <= 0:
        raise ValueError("degenerate landmarks: no similarity transform")
    A = scale * R
    t = mu_d - A @ mu_s
    Ai = np.linalg.inv(A)
    return np.hstack([A, t[:, None]]), np.hstack([Ai, (-Ai @ t)[:, None]])


# ----------------------------------------------------------------------------------------------------------------- ROC
def roc_points(label, scores):
    """sklearn.metrics.roc_curve(label, scores) with its default drop_intermediate=True (:799), restated: stable descending sort,
    the last index of every distinct score, tps / fps there, the points where a second difference of fps or tps is non-zero plus
    both ends, (0, 0) prepended.  -> (fpr, tpr) ascending."""
    y = np.asarray(label) == 1
    s = np.asarray(scores, dtype=np.float64)
    if y.shape != s.shape or s.ndim != 1 or s.size == 0:
        raise ValueError("label and scores must be one-dimensional and of one length")
    if np.any(np.isnan(s)):
        raise ValueError("scores hold NaN")
    if not y.any() or y.all():
        raise ValueError("the ROC needs pairs of both labels")
    idx = np.argsort(s, kind="mergesort")[::-1]
    s, y = s[idx], y[idx]
    last = np.r_[np.flatnonzero(np.diff(s)), y.size - 1]
    tps = np.cumsum(y, dtype=np.float64)[last]
    fps = 1 + last - tps
    if len(fps) > 2:
        keep = np.flatnonzero(np.r_[True, np.logical_or(np.diff(fps, 2), np.diff(tps, 2)), True])
        fps, tps = fps[keep], tps[keep]
    tps, fps = np.r_[0, tps], np.r_[0, fps]
    return fps / fps[-1], tps / tps[-1]


def tar_at_far(fpr, tpr, fars=FARS):
    """The table rule of :801-814: both arrays reversed (larger fpr first, for equal fpr the larger tpr first), then per FAR the point
    with the smallest |fpr - FAR|, on a tie the lowest index of the reversed arrays.  -> (indices into the reversed arrays, tpr at
    them, the table's '%.2f' % (100 tpr) strings)."""
    fr, tr = np.flipud(np.asarray(fpr)), np.flipud(np.asarray(tpr))
    idx = np.array([int(np.argmin(np.abs(fr - x))) for x in fars])
    return idx, tr[idx], ["%.2f" % (tr[i] * 100) for i in idx]


def table_row(method, target, cells, fars=FARS):
    """One table row as plain text (the reference prints a PrettyTable, :796-815)."""
    head = ["Methods"] + [str(x) for x in fars]
    row = ["%s-%s" % (method, target)] + list(cells)
    w = [max(len(a), len(b)) for a, b in zip(head, row)]
    return "\n".join(" | ".join(c.ljust(k) for c, k in zip(r, w)) for r in (head, row))


# ----------------------------------------------------------------------------------------------------------------- protocol
def build_csr(templates, medias):
    """The order image2template_feature visits the images in (:507-519: np.unique templates, np.unique media inside, np.where indices):
    -> (order int32 [N] sorted by (template, media, index), media_start int32 [M + 1] into order, template_start int32 [T + 1] into
    the media segments, unique_templates [T])."""
    templates, medias = np.asarray(templates), np.asarray(medias)
    if templates.ndim != 1 or templates.shape != medias.shape or templates.size == 0:
        raise ValueError("templates and medias must be one-dimensional, of one length and not empty")
    if templates.size >= 2 ** 31:
        raise ValueError("too many images")
    n = templates.size
    order = np.lexsort((np.arange(n), medias, templates))
    ts, ms = templates[order], medias[order]
    new_t = np.r_[True, ts[1:] != ts[:-1]]
    new_m = new_t | np.r_[True, ms[1:] != ms[:-1]]
    m_first = np.flatnonzero(new_m)
    media_start = np.r_[m_first, n].astype(np.int32)
    template_start = np.r_[np.searchsorted(m_first, np.flatnonzero(new_t)), len(m_first)].astype(np.int32)
    return order.astype(np.int32), media_start, template_start, ts[new_t]


def template_rows(unique_templates, p):
    """Row of every template id of `p` in unique_templates; an id without images raises (the reference maps it to row 0)."""
    p = np.asarray(p)
    i = np.searchsorted(unique_templates, p)
    bad = (i >= len(unique_templates)) | (unique_templates[np.minimum(i, len(unique_templates) - 1)] != p)
    if np.any(bad):
        raise ValueError(f"pairs name template ids without images: {np.unique(p[bad])[:8].tolist()}")
    return i.astype(np.int32)


def protocol(img_feats, faceness, templates, medias, p1, p2, flip=True, detector_score=True, use_norm_score=True, device=None):
    """:731-768 on the device.  img_feats f32 [N, 2D] (numpy, or a torch tensor on any device), faceness f32 [N].
    -> (scores float64 [P], template sums float32 [T, D] before normalisation, unique_templates [T]), numpy arrays."""
    import torch
    from .ops import _p, call
    if not use_norm_score:
        raise NotImplementedError("use_norm_score=False (per-image L2 normalisation) is not built; the reference hard-codes it to True")
    dev = torch.device(device) if device is not None else torch.device("cuda", torch.cuda.current_device())
    feats = torch.as_tensor(img_feats).to(device=dev, dtype=torch.float32).contiguous()
    if feats.dim() != 2 or feats.shape[1] % 2:
        raise ValueError("img_feats must be [N, 2D]: rows [emb(orig) | emb(flip)]")
    N, D = feats.shape[0], feats.shape[1] // 2
    order, media_start, template_start, uq = build_csr(templates, medias)
    if len(order) != N or np.asarray(faceness).shape != (N,):
        raise ValueError(f"{N} feature rows but {len(order)} template ids and faceness of shape {np.asarray(faceness).shape}")
    i1, i2 = template_rows(uq, p1), template_rows(uq, p2)
    if i1.shape != i2.shape or i1.ndim != 1 or i1.size == 0:
        raise ValueError("p1 and p2 must be one-dimensional, of one length and not empty")
    T, P = len(uq), len(i1)
    score_w = torch.as_tensor(np.asarray(faceness, dtype=np.float32)).to(dev)
    d_order, d_ms, d_ts = (torch.from_numpy(a).to(dev) for a in (order, media_start, template_start))
    d_i1, d_i2 = torch.from_numpy(i1).to(dev), torch.from_numpy(i2).to(dev)
    sums = torch.empty(T, D, device=dev, dtype=torch.float32)
    unit = torch.empty(T, D, device=dev, dtype=torch.float64)
    scores = torch.empty(P, device=dev, dtype=torch.float64)
    call("lafs_ijb_template_pool", _p(feats), 2 * D, _p(score_w), N, _p(d_order), _p(d_ms), len(media_start) - 1, _p(d_ts), T, D,
         int(bool(flip)), int(bool(detector_score)), _p(sums), _p(unit))
    call("lafs_ijb_pair_scores", _p(unit), T, D, _p(d_i1), _p(d_i2), P, _p(scores))
    return scores.cpu().numpy(), sums.cpu().numpy(), uq


# ----------------------------------------------------------------------------------------------------------------- 1:N
def pool_templates(img_feats, faceness, templates, medias, flip=True, detector_score=True, device=None):
    """protocol()'s pooling alone -> (unit rows float64 [T, D] on the device, unique_templates [T])."""
    import torch
    from .ops import _p, call
    dev = torch.device(device) if device is not None else torch.device("cuda", torch.cuda.current_device())
    feats = torch.as_tensor(img_feats).to(device=dev, dtype=torch.float32).contiguous()
    if feats.dim() != 2 or feats.shape[1] % 2:
        raise ValueError("img_feats must be [N, 2D]: rows [emb(orig) | emb(flip)]")
    N, D = feats.shape[0], feats.shape[1] // 2
    order, media_start, template_start, uq = build_csr(templates, medias)
    if len(order) != N or np.asarray(faceness).shape != (N,):
        raise ValueError(f"{N} feature rows but {len(order)} template ids and faceness of shape {np.asarray(faceness).shape}")
    T = len(uq)
    score_w = torch.as_tensor(np.asarray(faceness, dtype=np.float32)).to(dev)
    d_order, d_ms, d_ts = (torch.from_numpy(a).to(dev) for a in (order, media_start, template_start))
    sums = torch.empty(T, D, device=dev, dtype=torch.float32)
    unit = torch.empty(T, D, device=dev, dtype=torch.float64)
    call("lafs_ijb_template_pool", _p(feats), 2 * D, _p(score_w), N, _p(d_order), _p(d_ms), len(media_start) - 1, _p(d_ts), T, D,
         int(bool(flip)), int(bool(detector_score)), _p(sums), _p(unit))
    return unit, uq


def mates(gallery_sids, probe_sids):
    """Position in the gallery of every probe's subject, -1: none -> int32 [Q].  Two gallery templates of one subject raise."""
    gs, ps = np.asarray(gallery_sids), np.asarray(probe_sids)
    if gs.ndim != 1 or ps.ndim != 1 or gs.size == 0 or ps.size == 0:
        raise ValueError("gallery and probe subject ids must be one-dimensional and not empty")
    order = np.argsort(gs, kind="mergesort")
    sg = gs[order]
    if np.any(sg[1:] == sg[:-1]):
        raise ValueError(f"subjects with more than one gallery template: {np.unique(sg[1:][sg[1:] == sg[:-1]])[:8].tolist()}")
    i = np.minimum(np.searchsorted(sg, ps), len(sg) - 1)
    return np.where(sg[i] == ps, order[i], -1).astype(np.int32)


def search(unit, probe_rows, gallery_rows, mate, k=10):
    """lafs_ijb_search on pooled rows: unit f64 [T, D] on the device, probe_rows / gallery_rows int32 rows of it, mate int32 [Q]
    positions in gallery_rows (-1: none).  -> dict of numpy arrays top_score / top_idx [Q, k], mate_score, mate_rank, best_nonmate [Q],
    with the semantics of include/lafs_hip.h."""
    import torch
    from ._lib import lib
    from .ops import _p, call
    pr, gr, mt = (np.ascontiguousarray(a, dtype=np.int32) for a in (probe_rows, gallery_rows, mate))
    if pr.ndim != 1 or gr.ndim != 1 or pr.size == 0 or gr.size == 0 or mt.shape != pr.shape:
        raise ValueError("probe and gallery rows must be one-dimensional and not empty, mate of the probes' length")
    if not 1 <= int(k) <= MAX_TOP_K:
        raise ValueError(f"k must be in [1, {MAX_TOP_K}], got {k}")
    if np.any((mt < -1) | (mt >= gr.size)):
        raise ValueError("mate must hold positions of the gallery list, or -1")
    if unit.dim() != 2 or unit.dtype != torch.float64 or not unit.is_contiguous():
        raise ValueError("unit must be a contiguous float64 [T, D] tensor")
    dev, (T, D), Q, G, k = unit.device, unit.shape, pr.size, gr.size, int(k)
    d_pr, d_gr, d_mt = (torch.from_numpy(a).to(dev) for a in (pr, gr, mt))
    top_score = torch.empty(Q, k, device=dev, dtype=torch.float64)
    top_idx = torch.empty(Q, k, device=dev, dtype=torch.int32)
    mate_score = torch.empty(Q, device=dev, dtype=torch.float64)
    mate_rank = torch.empty(Q, device=dev, dtype=torch.int32)
    best_nonmate = torch.empty(Q, device=dev, dtype=torch.float64)
    need = int(lib().lafs_ijb_search_workspace(Q, G, k))
    ws = torch.empty(max(need, 1), device=dev, dtype=torch.uint8) if need else None
    call("lafs_ijb_search", _p(unit), T, D, _p(d_pr), Q, _p(d_gr), G, _p(d_mt), k, _p(top_score), _p(top_idx), _p(mate_score),
         _p(mate_rank), _p(best_nonmate), _p(ws) if need else None, need)
    return dict(top_score=top_score.cpu().numpy(), top_idx=top_idx.cpu().numpy(), mate_score=mate_score.cpu().numpy(),
                mate_rank=mate_rank.cpu().numpy(), best_nonmate=best_nonmate.cpu().numpy())


def identify(img_feats, faceness, templates, medias, gallery_tids, gallery_sids, probe_tids, probe_sids, k=10, flip=True,
             detector_score=True, device=None):
    """One gallery's searches on the device: pools like protocol(), then scores every probe template against every gallery template
    (lafs_ijb_search).  A template id without images raises, as in 1:1; so do two gallery templates of one subject.
    -> dict of numpy arrays: top_score f64 / top_idx i32 [Q, k] (positions in gallery_tids, -1 / NaN past the gallery's end),
    mate_score f64 [Q], mate_rank i32 [Q] (0: a rank-1 hit, -1: no mate), best_nonmate f64 [Q], mate i32 [Q]."""
    gt, pt = np.asarray(gallery_tids), np.asarray(probe_tids)
    if gt.shape != np.asarray(gallery_sids).shape or pt.shape != np.asarray(probe_sids).shape:
        raise ValueError("template and subject ids must be of one length")
    mate = mates(gallery_sids, probe_sids)
    unit, uq = pool_templates(img_feats, faceness, templates, medias, flip, detector_score, device)
    out = search(unit, template_rows(uq, pt), template_rows(uq, gt), mate, k)
    out["mate"] = mate
    return out


def cmc(mate_rank, ranks=CMC_RANKS):
    """Closed-set identification rates: the share of the mated searches (mate_rank >= 0) with mate_rank < r, per r in ranks."""
    mr = np.asarray(mate_rank)
    mr = mr[mr >= 0]
    if mr.size == 0:
        raise ValueError("no mated searches")
    return np.array([np.count_nonzero(mr < r) / mr.size for r in ranks], dtype=np.float64)


def tpir_at_fpir(mate_score, mate_rank, nonmated_top, fpirs=FPIRS, rank=1):
    """Open-set identification as the IJB-C paper defines it, restated (this project's reading; PARITY UNPINNED).  mate_score / mate_rank:
    the mated searches; nonmated_top: the top score of every non-mated search.  A search alarms when its top score is > tau.  For an
    FPIR f over the |N| non-mated searches tau is the (floor(f |N|) + 1)-th largest non-mated top score (f read as the decimal it
    prints as, so 0.1 * 30 is 3), and -inf when that index exceeds |N|: the realised FPIR never exceeds f.  TPIR is the share of the
    mated searches with mate_rank < rank and mate_score > tau.  NaN top scores never alarm (they sort below every number) and a NaN
    mate score is never a hit.  -> (tpir float64 [len(fpirs)], tau float64 [len(fpirs)])."""
    ms, mr, nt = np.asarray(mate_score, dtype=np.float64), np.asarray(mate_rank), np.asarray(nonmated_top, dtype=np.float64)
    if ms.ndim != 1 or ms.shape != mr.shape or nt.ndim != 1:
        raise ValueError("mate_score and mate_rank must be one-dimensional and of one length, nonmated_top one-dimensional")
    if ms.size == 0:
        raise ValueError("no mated searches")
    if nt.size == 0:
        raise ValueError("no non-mated searches")
    if np.any(mr < 0):
        raise ValueError("a mated search has no mate rank")
    desc = np.sort(np.where(np.isnan(nt), -np.inf, nt))[::-1]
    tpir, taus = [], []
    for f in fpirs:
        if not 0 <= f <= 1:
            raise ValueError(f"an FPIR must be in [0, 1], got {f}")
        m = math.floor(Fraction(repr(float(f))) * nt.size)                 # alarms allowed
        tau = float(desc[m]) if m < nt.size else -np.inf
        with np.errstate(invalid="ignore"):
            tpir.append(np.count_nonzero((mr < rank) & (ms > tau)) / ms.size)
        taus.append(tau)
    return np.array(tpir, dtype=np.float64), np.array(taus, dtype=np.float64)


def identification_metrics(res, ranks=CMC_RANKS, fpirs=FPIRS):
    """One gallery's searches (identify's dict) -> dict(cmc, tpir, tau): a probe with a mate is a mated search, every other probe a
    non-mated one."""
    mated = res["mate"] >= 0
    tpir, tau = tpir_at_fpir(res["mate_score"][mated], res["mate_rank"][mated], res["top_score"][~mated, 0], fpirs)
    return dict(cmc=cmc(res["mate_rank"][mated], ranks), tpir=tpir, tau=tau)


def evaluate_identification(img_feats, meta, lists, k=10, flip=True, detector_score=True, device=None, ranks=CMC_RANKS, fpirs=FPIRS):
    """Every probe of lists (read_identification_lists) searched in G1 and in G2: mated in the gallery that holds its subject, non-mated
    in the other, non-mated in both when neither does.  -> dict(G1=..., G2=... (identification_metrics), mean=dict(cmc, tpir),
    searches=dict(G1=..., G2=... (identify's arrays)))."""
    if k < max(ranks):
        raise ValueError(f"k = {k} is smaller than the largest CMC rank {max(ranks)}")
    out = {"searches": {}}
    for g, key in (("G1", "g1"), ("G2", "g2")):
        res = identify(img_feats, meta["faceness"], meta["templates"], meta["medias"], lists[key + "_tids"], lists[key + "_sids"],
                       lists["probe_tids"], lists["probe_sids"], k, flip, detector_score, device)
        out["searches"][g] = res
        out[g] = identification_metrics(res, ranks, fpirs)
    out["mean"] = dict(cmc=(out["G1"]["cmc"] + out["G2"]["cmc"]) / 2, tpir=(out["G1"]["tpir"] + out["G2"]["tpir"]) / 2)
    return out


def identification_row(method, target, mean, ranks=CMC_RANKS, fpirs=FPIRS):
    """The 1:N table row as plain text, '%.2f' percentages like the 1:1 row."""
    head = ["Methods"] + ["rank-%d" % r for r in ranks] + ["TPIR@FPIR=%s" % f for f in fpirs]
    row = ["%s-%s" % (method, target)] + ["%.2f" % (100 * v) for v in list(mean["cmc"]) + list(mean["tpir"])]
    w = [max(len(a), len(b)) for a, b in zip(head, row)]
    return "\n".join(" | ".join(c.ljust(n) for c, n in zip(r, w)) for r in (head, row))


# ----------------------------------------------------------------------------------------------------------------- extraction
def _decode(path):
    from PIL import Image
    with Image.open(path) as im:
        return np.asarray(im.convert("RGB"))


class IJBEvaluator:
    def __init__(self, backbone, batch_size=360, device=None, norm="reference", workers=8, landmark_teacher=None):
        """backbone: ViT_face_landmark_patch8 (with or without the landmark branch) or ViTs_face_overlap; batch_size: loose crops per batch; norm:
        'reference' (x/255 - 0.5, :235) or 'train' (the fine-tune feed); workers: decode threads (at most 16); landmark_teacher: the
        frozen stage-1 CNN whose patches feed a backbone without a branch of its own (verification.landmark_plan)."""
        import torch
        from .verification import NORMS
        from .vision_transformer import attach_arena
        if batch_size <= 0:
            raise ValueError(f"the batch size must be positive, got {batch_size}")
        if norm not in NORMS:
            raise ValueError(f"norm must be one of {sorted(NORMS)}")
        self.device = torch.device(device) if device is not None else torch.device("cuda", torch.cuda.current_device())
        self.model, self.B, self.norm = backbone, int(batch_size), norm
        self.teacher = landmark_teacher
        self.workers = max(1, min(int(workers), MAX_WORKERS))
        self.arena = attach_arena(backbone, self.device)
        self.keep_aligned = False                  # test hook: keep the aligned uint8 crops (self.aligned [N,3,112,112], CPU)
        self.aligned = None
        self._meta = -(-40 * self.B // 16) * 16    # staging head: offsets i64 [B] | (H, W) i32 [B,2] | inverse maps f32 [B,6]
        self._stage = self._dev = None
        S = IMAGE_SIZE
        self._x = torch.empty(2 * self.B, 3, S, S, device=self.device, dtype=torch.float32)
        self._mosaic = torch.empty_like(self._x) if getattr(backbone, "with_land", False) or landmark_teacher is not None else None
        self._al = torch.empty(self.B, 3, S, S, device=self.device, dtype=torch.uint8)

    def _staging(self, n_bytes):
        import torch
        need = self._meta + n_bytes
        if self._stage is None or self._stage.numel() < need:
            cap = max(need, self._meta + self.B * 200 * 200 * 3)
            self._stage = torch.empty(cap, dtype=torch.uint8).pin_memory()
            self._dev = torch.empty(cap, dtype=torch.uint8, device=self.device)
        return self._stage, self._dev

    def _align_batch(self, imgs, lmk):
        """Loose crops (uint8 HWC arrays) + landmarks [n,5,2] -> the kernel's f32 [2n,3,112,112] (and self._al[:n])."""
        import torch
        from .ops import _p, call
        from .verification import NORMS
        n, B = len(imgs), self.B
        for im in imgs:
            if im.ndim != 3 or im.shape[2] != 3 or im.dtype != np.uint8 or im.shape[0] < 1 or im.shape[1] < 1:
                raise ValueError(f"a loose crop must be uint8 [H, W, 3], got {im.dtype} {im.shape}")
        sizes = np.array([im.shape[0] * im.shape[1] * 3 for im in imgs], dtype=np.int64)
        offs = np.r_[0, np.cumsum(sizes)]
        stage, devbuf = self._staging(int(offs[-1]))
        head = stage.numpy()
        head[:8 * n].view(np.int64)[:] = offs[:n]
        head[8 * B:8 * B + 8 * n].view(np.int32)[:] = np.array([im.shape[:2] for im in imgs], dtype=np.int32).reshape(-1)
        maps = np.stack([similarity_from_landmarks(l)[1] for l in lmk]).astype(np.float32)
        head[16 * B:16 * B + 24 * n].view(np.float32)[:] = maps.reshape(-1)
        for im, o in zip(imgs, offs):
            head[self._meta + o:self._meta + o + im.size] = im.reshape(-1)
        used = self._meta + int(offs[-1])
        devbuf[:used].copy_(stage[:used], non_blocking=True)
        d_off, d_hw, d_map = devbuf[:8 * B].view(torch.int64), devbuf[8 * B:16 * B].view(torch.int32), devbuf[16 * B:40 * B].view(torch.float32)
        x = self._x[: 2 * n]
        div, mul, add = NORMS[self.norm]
        call("lafs_ijb_align_flip_normalize", _p(devbuf[self._meta:]), int(offs[-1]), _p(d_off), _p(d_hw), _p(d_map), n, IMAGE_SIZE,
             div, mul, add, _p(x), _p(self._al))
        torch.cuda.current_stream().synchronize()          # the staging buffer is rewritten by the next batch
        return x

    def features(self, images, landmarks):
        """images: list of uint8 [H,W,3] RGB arrays, or of file paths (decoded with Pillow in the thread pool); landmarks [N,5,2].
        -> img_feats f32 [N, 2D] on the device, rows [emb(orig) | emb(flip)] (forward_db, :232-247)."""
        import torch
        from .verification import extract_features, landmark_plan
        landmarks = np.asarray(landmarks)
        N = len(images)
        if landmarks.shape != (N, 5, 2):
            raise ValueError(f"expected landmarks [{N}, 5, 2], got {landmarks.shape} (only the 5-landmark form is supported)")
        m, B, dev = self.model, self.B, self.device
        D = m._spec.trunk.dim
        out = torch.empty(N, 2 * D, device=dev, dtype=torch.float32)
        self.aligned = torch.empty(N, 3, IMAGE_SIZE, IMAGE_SIZE, dtype=torch.uint8) if self.keep_aligned else None
        with torch.no_grad(), ThreadPoolExecutor(self.workers) as pool, ThreadPoolExecutor(1) as ahead:
            m._arena.ensure_fresh()
            cnn = landmark_plan(m, dev, self.teacher)
            load = lambda i0: list(pool.map(lambda v: _decode(v) if isinstance(v, (str, os.PathLike)) else np.asarray(v),
                                            images[i0:i0 + B]))
            nxt = ahead.submit(load, 0)
            for i0 in range(0, N, B):
                imgs = nxt.result()
                if i0 + B < N:                                 # the next batch decodes while this one is on the device
                    nxt = ahead.submit(load, i0 + B)
                n = len(imgs)
                x = self._align_batch(imgs, landmarks[i0:i0 + n])
                feat = extract_features(m, self.arena, x, n, cnn, self._mosaic, dev)
                out[i0:i0 + n, :D] = feat[:n]
                out[i0:i0 + n, D:] = feat[n:2 * n]
                if self.aligned is not None:
                    self.aligned[i0:i0 + n] = self._al[:n].cpu()
        return out

    def __call__(self, image_dir, meta, flip=True, detector_score=True):
        """meta: read_meta's dict -> (scores, fpr, tpr, table cells); the features stay in self.img_feats."""
        paths = [os.path.join(image_dir, n) for n in meta["names"]]
        self.img_feats = self.features(paths, meta["landmarks"])
        return evaluate(self.img_feats, meta, flip, detector_score, self.device)


def evaluate(img_feats, meta, flip=True, detector_score=True, device=None):
    scores, _, _ = protocol(img_feats, meta["faceness"], meta["templates"], meta["medias"], meta["p1"], meta["p2"], flip, detector_score,
                            device=device)
    fpr, tpr = roc_points(meta["label"], scores)
    return scores, fpr, tpr, tar_at_far(fpr, tpr)[2]


# ----------------------------------------------------------------------------------------------------------------- entry point
def main(argv=None):
    """TAR@FAR (--protocol 11) or rank-k and TPIR@FPIR (--protocol 1N) of a saved fine-tune checkpoint (the `module.`-prefixed state
    dict train_largescale.py writes) on IJB-B / IJB-C."""
    import torch
    from . import train_largescale as tl
    from .vision_transformer import attach_arena
    p = argparse.ArgumentParser("Part-fViT / fViT IJB evaluation", parents=[tl.get_args_parser()], conflict_handler="resolve")
    p.add_argument("--checkpoint", default="", type=str, help="fine-tune checkpoint (not needed with --features)")
    p.add_argument("--image_path", required=True, type=str, help="directory with loose_crop/ and meta/")
    p.add_argument("--target", default="IJBC", type=str, choices=["IJBC", "IJBB"])
    p.add_argument("--result_dir", default=".", type=str)
    p.add_argument("--job", default="lafs", type=str)
    p.add_argument("--batch_size", default=360, type=int)
    p.add_argument("--workers", default=8, type=int, help="decode threads (at most 16)")
    p.add_argument("--no_flip", action="store_true", help="use_flip_test = False")
    p.add_argument("--no_detector_score", action="store_true", help="use_detector_score = False")
    p.add_argument("--save_features", default="", type=str, help="write img_feats and faceness to this .npz")
    p.add_argument("--features", default="", type=str, help="skip the extraction: read img_feats from this .npz")
    p.add_argument("--protocol", default="11", type=str, choices=["11", "1N"],
                   help="11: template verification, TAR@FAR; 1N: identification against G1 and G2, rank-k and TPIR@FPIR")
    args = p.parse_args(argv)
    device = torch.device("cuda", torch.cuda.current_device())
    meta = read_meta(args.image_path, args.target)
    lists = read_identification_lists(args.image_path, args.target) if args.protocol == "1N" else None
    t0 = time.time()
    if args.features:
        with np.load(args.features, allow_pickle=False) as z:
            feats = z["img_feats"]
        if feats.shape[0] != len(meta["names"]):
            raise SystemExit(f"{args.features}: {feats.shape[0]} feature rows for {len(meta['names'])} images")
    else:
        if not args.checkpoint:
            raise SystemExit("--checkpoint is required without --features")
        backbone = tl.build_backbone(args)
        sd = torch.load(args.checkpoint, map_location="cpu", weights_only=False)
        sd = {(k[len("module."):] if k.startswith("module.") else k): v for k, v in sd.items()}
        backbone.load_state_dict(sd)
        attach_arena(backbone, device)
        ev = IJBEvaluator(backbone, args.batch_size, device, norm=args.val_norm, workers=args.workers,
                          landmark_teacher=None if args.keep_land else tl.build_landmark_teacher(args))
        paths = [os.path.join(args.image_path, "loose_crop", n) for n in meta["names"]]
        feats = ev.features(paths, meta["landmarks"])
        torch.cuda.synchronize()
        print(f"[{args.target}] {len(paths)} images in {time.time() - t0:.2f} s")
        if args.save_features:
            np.savez(args.save_features, img_feats=feats.cpu().numpy(), faceness=meta["faceness"])
    t0 = time.time()
    save_path = os.path.join(args.result_dir, args.job)
    if args.protocol == "1N":
        res = evaluate_identification(feats, meta, lists, 10, not args.no_flip, not args.no_detector_score, device)
        os.makedirs(save_path, exist_ok=True)
        out = os.path.join(save_path, "%s_1N.npz" % args.target.lower())
        arrays = {"probe_tids": lists["probe_tids"], "probe_sids": lists["probe_sids"]}
        for g, key in (("G1", "g1"), ("G2", "g2")):
            arrays.update({f"{g}_gallery_tids": lists[key + "_tids"], f"{g}_gallery_sids": lists[key + "_sids"]})
            arrays.update({f"{g}_{name}": a for name, a in res["searches"][g].items()})
        np.savez(out, **arrays)
        print(f"[{args.target}] {2 * len(lists['probe_tids'])} searches in {time.time() - t0:.2f} s -> {out}")
        print(identification_row(args.target.lower(), args.target, res["mean"]))
        return
    scores, fpr, tpr, cells = evaluate(feats, meta, not args.no_flip, not args.no_detector_score, device)
    os.makedirs(save_path, exist_ok=True)
    out = os.path.join(save_path, "%s.npy" % args.target.lower())
    np.save(out, scores)
    print(f"[{args.target}] {len(scores)} pairs in {time.time() - t0:.2f} s -> {out}")
    print(table_row(args.target.lower(), args.target, cells))


if __name__ == "__main__":
    main()
