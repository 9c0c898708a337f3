"""The fp64 oracle of lafs_landmark_mse (landmark supervision of the fine-tune step, reference train_largescale.py:825-843), the bounds
its fp32 kernel is held to, an fp32 emulation of the kernel's own order of operations, and the case grid of the GPU test.  numpy only:
shared by tests/test_pre_land_host.py (which shows that the oracle is torch's MSELoss, that the emulation passes and that seeded faults
fail) and tests/test_gpu_pre_land.py.

The kernel (csrc/finetune.hip landmark_mse_kernel), one workgroup of 1024 threads, N = 2 B n values = B n (x, y) pairs:
    w    = weight * grad_scale                                   1 rounding
    inv  = 1 / (111^2 N)                                         1 rounding (computed in double on the host, cast once); 2 inv is exact
    coef = w * (2 inv)                                           1 rounding
    per pair i (thread i % 1024, in index order):  dx = px - lx, dy = py - ly            1 rounding each
        sq = fma(dx, dx, sq); sq = fma(dy, dy, sq)                                     1 rounding each, ceil(B n / 1024) pairs per thread
        dtheta = fma(coef, d, dtheta)                                                  1 rounding
    butterfly over 64 lanes (6 additions), thread 0 adds the 16 wave sums in order (16 additions)
    loss_land = s * inv                                          1 rounding
    loss = fma(w, loss_land, loss)                               1 rounding
Operation count per pair: 2 subtractions, 4 fused multiply-adds (6 without dtheta: 2 + 2).
So:  a term of the sum of squares carries its difference's rounding twice (2 u) and passes through at most
     DEPTH = 2 ceil(B n / 1024) + 6 + 16 additions; all terms are >= 0, so the sum is off by at most (2 + DEPTH) u relative;
     loss_land: + 2 (inv, the product);   the loss term w loss_land: + 1 (w), and the fma's own rounding u |loss|;
     the gradient increment coef d: 4 roundings (w, inv, coef, d), and the fma's own rounding u |dtheta|.
`weight` and `grad_scale` are the fp32 values the kernel holds (f32c)."""
import math

import numpy as np

U = 2.0 ** -24
THREADS, WAVE = 1024, 64
SHAPES = [(1, 36), (2, 196), (5, 196), (8, 36), (128, 196)]
WEIGHTS = [0.0, 0.11, 1.0, 1000.0]
GRAD_SCALES = [1.0, 1.0 / 3.0]
INPUTS = ["uniform", "equal", "ends"]


def f32c(v):
    return float(np.float32(v))


def rel(k):
    """k roundings in sequence: (1 + u)^k - 1."""
    return (1.0 + U) ** k - 1.0


def depth(n_pairs):
    return 2 * math.ceil(n_pairs / THREADS) + 6 + THREADS // WAVE


def make_inputs(kind, B, n, seed=0):
    """(pred, label) f32 [B, n, 2] in [0, 111]: uniform; pred == label; values at the ends of the range (every pair of ends occurs)."""
    g = np.random.RandomState(1000 * B + n + seed)
    if kind == "uniform":
        return (g.uniform(0, 111, (B, n, 2)).astype(np.float32), g.uniform(0, 111, (B, n, 2)).astype(np.float32))
    if kind == "equal":
        p = g.uniform(0, 111, (B, n, 2)).astype(np.float32)
        return p, p.copy()
    if kind == "ends":
        ends = np.array([0.0, 111.0], dtype=np.float32)
        return ends[g.randint(0, 2, (B, n, 2))], ends[g.randint(0, 2, (B, n, 2))]
    raise ValueError(kind)


def oracle(pred, label, weight, grad_scale, dtheta=None, loss=None):
    """fp64: {"loss_land", "term" = weight grad_scale loss_land, "inc" = the gradient increment, "loss", "dtheta" (None without an old
    value)}.  weight / grad_scale: widened fp32 values."""
    p, l = np.asarray(pred, np.float64), np.asarray(label, np.float64)
    N = p.size
    d = p - l
    loss_land = float((d * d).sum() / (111.0 ** 2 * N))
    w = float(weight) * float(grad_scale)
    out = dict(loss_land=loss_land, term=w * loss_land, inc=w * 2.0 * d / (111.0 ** 2 * N), loss=None, dtheta=None)
    if loss is not None:
        out["loss"] = float(loss) + out["term"]
    if dtheta is not None:
        out["dtheta"] = np.asarray(dtheta, np.float64) + out["inc"]
    return out


def bounds(ref, n_pairs):
    """Element-wise bounds of the kernel's three outputs around `ref` (see the module docstring)."""
    dep = depth(n_pairs)
    out = dict(loss_land=rel(2 + dep + 2) * ref["loss_land"], loss=None, dtheta=None)
    if ref["loss"] is not None:
        out["loss"] = rel(2 + dep + 2 + 1) * abs(ref["term"]) + U * abs(ref["loss"])
    if ref["dtheta"] is not None:
        out["dtheta"] = rel(4) * np.abs(ref["inc"]) + U * np.abs(ref["dtheta"])
    return out


def within(got, ref, bound):
    """(ok, worst |err| / bound over the elements with a non-zero bound)."""
    got, ref, bound = (np.asarray(v, np.float64) for v in (got, ref, bound))
    err = np.abs(got - ref)
    nz = bound > 0
    ratio = float((err[nz] / bound[nz]).max()) if nz.any() else 0.0
    return bool(np.all(np.isfinite(got)) and np.all(err <= bound)), ratio


def _fma(a, b, c):
    """fp32 fma of fp32 operands (the fp64 product of two fp32 values is exact)."""
    return (a.astype(np.float64) * b.astype(np.float64) + c.astype(np.float64)).astype(np.float32)


def emulate_f32(pred, label, weight, grad_scale, dtheta=None, loss=None):
    """The kernel's arithmetic in its own order, in fp32: (loss_land, loss or None, dtheta or None)."""
    f = np.float32
    p, l = np.asarray(pred, f).reshape(-1, 2), np.asarray(label, f).reshape(-1, 2)
    n_pairs = p.shape[0]
    inv = f(1.0 / (111.0 * 111.0 * 2.0 * n_pairs))
    w = f(f(weight) * f(grad_scale))
    coef = f(w * f(f(2.0) * inv))
    d = (p - l).astype(f)
    rounds = math.ceil(n_pairs / THREADS)
    dpad = np.zeros((rounds * THREADS, 2), f)
    dpad[:n_pairs] = d
    dpad = dpad.reshape(rounds, THREADS, 2)
    sq = np.zeros(THREADS, f)
    for r in range(rounds):                                   # (a padded pair adds fma(0, 0, sq) = sq)
        sq = _fma(dpad[r, :, 0], dpad[r, :, 0], sq)
        sq = _fma(dpad[r, :, 1], dpad[r, :, 1], sq)
    lane = np.arange(THREADS)
    for o in (32, 16, 8, 4, 2, 1):
        sq = (sq + sq[lane ^ o]).astype(f)
    s = f(0.0)
    for k in range(THREADS // WAVE):
        s = f(s + sq[k * WAVE])
    loss_land = f(s * inv)
    new_loss = None if loss is None else f(np.float64(w) * np.float64(loss_land) + np.float64(f(loss)))
    new_d = None
    if dtheta is not None:
        old = np.asarray(dtheta, f).reshape(-1, 2)
        new_d = _fma(np.broadcast_to(coef, d.shape), d, old).reshape(np.asarray(dtheta).shape)
    return loss_land, new_loss, new_d


def check_case(got_loss_land, got_loss, got_dtheta, pred, label, weight, grad_scale, dtheta_old, loss_old):
    """All three outputs against the oracle: (ok, {name: worst ratio})."""
    ref = oracle(pred, label, f32c(weight), f32c(grad_scale), dtheta_old, loss_old)
    bnd = bounds(ref, np.asarray(pred).size // 2)
    ok, ratios = True, {}
    for name, got in (("loss_land", got_loss_land), ("loss", got_loss), ("dtheta", got_dtheta)):
        if ref[name] is None:
            continue
        o, ratios[name] = within(got, ref[name], bnd[name])
        ok = ok and o
    return ok, ratios
