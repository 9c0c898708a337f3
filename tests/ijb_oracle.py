"""CPU restatement (numpy only) of the IJB-B / IJB-C evaluation, reference IJB_evaluation.py: the alignment in float32 in the operation
order of csrc/ijb.hip, the landmark similarity transform, the protocol (:731-751, :501-567) as per-column sequential float32 sums with
a float64 tail, and sklearn's roc_curve + the reference's table rule (:795-815).  Not a test module: tests import it."""
import numpy as np

f32 = np.float32
NORMS = {"reference": (255.0, 1.0, -0.5), "train": (1.0, 2.0 / 255.0, -1.0)}
ARCFACE_SRC = np.array([[30.2946, 51.6963], [65.5318, 51.5014], [48.0252, 71.7366], [33.5493, 92.3655], [62.7299, 92.2041]], dtype=f32)
ARCFACE_SRC[:, 0] += 8.0                                   # IJB_evaluation.py:144-150
FARS = [10 ** -6, 10 ** -5, 10 ** -4, 10 ** -3, 10 ** -2, 10 ** -1]     # :795


# ----------------------------------------------------------------------------------------------------------------- geometry
def similarity(src, dst=ARCFACE_SRC):
    """Least-squares proper similarity (rotation, uniform scale, translation) src -> dst, through complex numbers: with centred points
    z (src) and w (dst), the optimal a in w ~ a z is sum(w conj z) / sum |z|^2.  -> (forward 2x3, inverse 2x3) float64.  For points that
    are not mirrored this is the minimiser Umeyama's closed form returns."""
    src, dst = np.asarray(src, np.float64), np.asarray(dst, np.float64)
    ms, md = src.mean(0), dst.mean(0)
    z = (src[:, 0] - ms[0]) + 1j * (src[:, 1] - ms[1])
    w = (dst[:, 0] - md[0]) + 1j * (dst[:, 1] - md[1])
    a = np.sum(w * np.conj(z)) / np.sum(np.abs(z) ** 2)
    A = np.array([[a.real, -a.imag], [a.imag, a.real]])
    t = md - A @ ms
    Ai = np.linalg.inv(A)
    return np.hstack([A, t[:, None]]), np.hstack([Ai, (-Ai @ t)[:, None]])


def residual(M, src, dst=ARCFACE_SRC):
    src, dst = np.asarray(src, np.float64), np.asarray(dst, np.float64)
    return float(np.sum((src @ M[:, :2].T + M[:, 2] - dst) ** 2))


def align(img, inv, S=112):
    """img u8 [H,W,3], inv = the six coefficients of the inverse map (output pixel -> source) -> aligned u8 [3,S,S].  Float32, the
    operation order of ijb_align_kernel."""
    img = np.asarray(img)
    H, W = img.shape[:2]
    m = np.asarray(inv, dtype=f32).reshape(6)
    xs, ys = np.arange(S, dtype=f32)[None, :], np.arange(S, dtype=f32)[:, None]
    with np.errstate(all="ignore"):
        sx = (m[0] * xs + m[1] * ys) + m[2]
        sy = (m[3] * xs + m[4] * ys) + m[5]
        inside = (sx > f32(-1)) & (sx < f32(W)) & (sy > f32(-1)) & (sy < f32(H))
        sx, sy = np.where(inside, sx, f32(0)), np.where(inside, sy, f32(0))
        x0f, y0f = np.floor(sx), np.floor(sy)
        fx, fy = sx - x0f, sy - y0f
        gx, gy = f32(1) - fx, f32(1) - fy
        x0, y0 = x0f.astype(np.int64), y0f.astype(np.int64)

        def tap(dy, dx):
            yy, xx = y0 + dy, x0 + dx
            ok = inside & (yy >= 0) & (yy < H) & (xx >= 0) & (xx < W)
            v = img[np.clip(yy, 0, H - 1), np.clip(xx, 0, W - 1)].astype(f32)
            return np.where(ok[..., None], v, f32(0))

        gx, fx, gy, fy = gx[..., None], fx[..., None], gy[..., None], fy[..., None]
        top = tap(0, 0) * gx + tap(0, 1) * fx
        bot = tap(1, 0) * gx + tap(1, 1) * fx
        val = top * gy + bot * fy
        assert val.dtype == f32
        u = np.clip(np.rint(val), f32(0), f32(255))
    u = np.where(inside[..., None], u, f32(0))
    return u.astype(np.uint8).transpose(2, 0, 1).copy()


def normalize(u8, norm="reference"):
    """u8 [...] -> f32 x / div * mul + add, each operation rounded on its own."""
    div, mul, add = (f32(v) for v in NORMS[norm])
    return u8.astype(f32) / div * mul + add


def align_flip_normalize(images, invs, S=112, norm="reference"):
    """-> (f32 [2B,3,S,S]: the aligned batch, then the batch mirrored along W; u8 [B,3,S,S])."""
    al = np.stack([align(im, mv, S) for im, mv in zip(images, invs)])
    x = normalize(al, norm)
    return np.concatenate([x, x[..., ::-1]]), al


# ----------------------------------------------------------------------------------------------------------------- protocol
def template_sums(img_feats, faceness, templates, medias, flip=True, detector_score=True):
    """:731-751 and the sums of :501-528, every column accumulated sequentially in float32 in (template, media, image) order.
    -> (sums f32 [T, D], unique_templates)."""
    f = np.asarray(img_feats, dtype=f32)
    D = f.shape[1] // 2
    x = f[:, :D] + f[:, D:] if flip else f[:, :D].copy()
    if detector_score:
        x = x * np.asarray(faceness, dtype=f32)[:, None]
    assert x.dtype == f32
    templates, medias = np.asarray(templates), np.asarray(medias)
    uq = np.unique(templates)
    order = np.argsort(templates, kind="stable")
    starts = np.searchsorted(templates[order], uq)
    ends = np.append(starts[1:], len(order))
    sums = np.zeros((len(uq), D), f32)
    for ti in range(len(uq)):
        ind_t = order[starts[ti]:ends[ti]]                      # ascending image indices (stable sort) = np.where(templates == uqt)
        fm = medias[ind_t]
        acc = None
        for u in np.unique(fm):
            rows = ind_t[fm == u]
            m = x[rows[0]].copy()
            for r in rows[1:]:
                m += x[r]
            if len(rows) > 1:
                m = m / f32(len(rows))
            acc = m if acc is None else acc + m
        sums[ti] = acc
    return sums, uq


def unit_rows(sums):
    t = np.asarray(sums).astype(np.float64)
    n = np.sqrt(np.sum(t * t, axis=1))
    n[n == 0.0] = 1.0
    return t / n[:, None]


def pair_scores(unit, uq, p1, p2, chunk=100000):
    i1, i2 = np.searchsorted(uq, p1), np.searchsorted(uq, p2)
    if np.any(i1 >= len(uq)) or np.any(i2 >= len(uq)) or np.any(uq[i1] != p1) or np.any(uq[i2] != p2):
        raise ValueError("a pair names a template without images")
    out = np.zeros(len(i1))
    for s in range(0, len(i1), chunk):
        out[s:s + chunk] = np.sum(unit[i1[s:s + chunk]] * unit[i2[s:s + chunk]], -1)
    return out


def protocol(img_feats, faceness, templates, medias, p1, p2, flip=True, detector_score=True):
    """-> (scores f64 [P], template sums f32 [T, D], unique_templates)."""
    sums, uq = template_sums(img_feats, faceness, templates, medias, flip, detector_score)
    return pair_scores(unit_rows(sums), uq, np.asarray(p1), np.asarray(p2)), sums, uq


# ----------------------------------------------------------------------------------------------------------------- ROC
def roc_points(label, scores):
    """sklearn.metrics.roc_curve(label, scores) with drop_intermediate=True -> (fpr, tpr), ascending as sklearn returns them."""
    y = np.asarray(label) == 1
    s = np.asarray(scores, dtype=np.float64)
    idx = np.argsort(s, kind="mergesort")[::-1]
    s, y = s[idx], y[idx]
    thr = np.r_[np.where(np.diff(s))[0], y.size - 1]
    tps = np.cumsum(y.astype(np.float64))[thr]
    fps = 1 + thr - tps
    if len(fps) > 2:
        keep = np.where(np.r_[True, np.logical_or(np.diff(fps, 2), np.diff(tps, 2)), True])[0]
        fps, tps = fps[keep], tps[keep]
    tps, fps = np.r_[0, tps], np.r_[0, fps]
    return fps / fps[-1], tps / tps[-1]


def tar_at_far(fpr, tpr, fars=FARS):
    """:801-814: both arrays reversed, then per FAR the point with the smallest |fpr - FAR|, the lowest reversed index on a tie.
    -> (indices into the reversed arrays, tpr at them, the table's '%.2f' strings)."""
    fr, tr = np.flipud(fpr), np.flipud(tpr)
    idx = np.array([int(np.argmin(np.abs(fr - x))) for x in fars])
    return idx, tr[idx], ["%.2f" % (tr[i] * 100) for i in idx]
