"""Shared by the fViT tests (tests/test_gpu_unfold.py, test_gpu_bn1d.py, test_gpu_fvit.py, test_fvit_host.py): the F26 fixture
loader, the fixture model's configuration, the unfold / fold case grid and the fp64 BatchNorm1d oracle with its per-element bounds."""
import glob
import os

import torch

from conftest import GOLDEN, load_golden

f64 = torch.float64
U = 2.0 ** -24                      # fp32 unit roundoff
SLACK = 1.01                        # second-order terms of the first-order bounds below

FVIT_CFG = dict(loss_type="None", GPU_ID=None, num_class=10, image_size=112, patch_size=8, ac_patch_size=12, dim=128, depth=2, heads=3,
                mlp_dim=256, dropout=0, emb_dropout=0)


def fvit_fixture_files():
    return sorted(glob.glob(os.path.join(GOLDEN, "f26_fvit*.npz")))


def load_fvit():
    """F26 is stored in parts (no committed file above 1 MiB): f26_fvit.npz, f26_fvit_1.npz, ... with disjoint keys."""
    out = {}
    for path in fvit_fixture_files():
        part = load_golden(os.path.basename(path)[:-4])
        assert not set(part) & set(out), path
        out.update(part)
    return out


# (S, k, stride, pad, B): every way lafs_unfold_bf16 / lafs_fold_f32 can go wrong has a case
UNFOLD_CASES = [
    (16, 8, 8, 0, 3),       # must equal lafs_patchify(order=CHW) bit for bit
    (32, 16, 16, 0, 3),     # non-overlapping, k != 8, K = 768
    (16, 12, 8, 4, 3),      # n = 2; top / left padding only (the second window ends on the last pixel)
    (18, 12, 8, 4, 3),      # n = 2 by floor: the two bottom rows / right columns lie under no window
    (24, 12, 8, 2, 3),      # n = 3; padding used on all four sides
    (20, 12, 8, 4, 3),      # S % 8 != 0: rows not 16-byte aligned
    (21, 5, 3, 1, 3),       # odd everything, 3 k^2 = 75 -> ldp = 96
    (112, 12, 8, 4, 2),     # the fViT shapes
    (48, 12, 8, 4, 2),
]


def windows(S, k, stride, pad):
    return (S + 2 * pad - k) // stride + 1


# ------------------------------------------------------------------------------------------------ BatchNorm1d oracle
def _rs(v, eps):
    return (v.clamp_min(0) + eps) ** -0.5


def bn_stats(x, eps):
    """fp64 column statistics of x [n, D] and how far the kernel's fp32 values may lie from them.  The kernel (csrc/unfold.hip) forms
    mean = x0 + sum(x - x0) / n and var = sum (x - mean)^2 / n; every bound below counts the roundings of those formulas with the
    order-free worst case for the sums (n additions of n terms: n u sum|terms|).
      mean: n subtractions (u |d| each), the sum, one division, one addition
      var : c = x - mean inherits the mean's error (+ u |c|); squares, the sum, one division
      rstd: monotone in var, so the var interval maps to an rstd interval; + 4 u for the add, sqrt and divide"""
    n = x.shape[0]
    d = x - x[0]
    S = d.sum(0)
    mean = x.mean(0)
    e_mean = SLACK * ((n + 1) * U * d.abs().sum(0) / n + U * (S / n).abs() + U * mean.abs())
    c = x - mean
    var = (c * c).mean(0)
    ec = e_mean + U * c.abs()
    ca = c.abs() + ec
    e_var = SLACK * ((2 * c.abs() * ec + ec * ec).sum(0) / n + (1.0 / n + 1) * U * (ca * ca).sum(0) + U * var)
    rs = _rs(var, eps)
    e_rs = torch.maximum(_rs(var - e_var, eps) - rs, rs - _rs(var + e_var, eps)) + 4 * U * rs
    return mean, e_mean, var, e_var, rs, e_rs


def bn_xhat(x, mean, e_mean, rs, e_rs):
    """xhat = (x - mean) rstd as the kernels form it: one subtraction, one product."""
    c = x - mean
    ec = e_mean + U * c.abs()
    xh = c * rs
    return xh, SLACK * (ec * rs + c.abs() * e_rs + ec * e_rs + U * xh.abs())


def bn_forward_reference(x, gamma, beta, eps, momentum, rm, rv, training):
    """{name: (fp64 value, bound)} of everything lafs_bn1d_fwd writes; all arguments fp64 (the fp32 inputs widened exactly)."""
    n = x.shape[0]
    if training:
        mean, e_mean, var, e_var, rs, e_rs = bn_stats(x, eps)
    else:
        mean, e_mean, rs = rm, torch.zeros_like(rm), _rs(rv, eps)
        e_rs = 4 * U * rs
    xh, e_xh = bn_xhat(x, mean, e_mean, rs, e_rs)
    y = xh * gamma + beta
    out = {"y": (y, SLACK * (e_xh * gamma.abs() + U * (xh * gamma).abs() + U * y.abs())),
           "save_mean": (mean, e_mean), "save_rstd": (rs, e_rs)}
    if training:
        # (1 - m) old + m new: (1 - m) rounds, two products, one addition; the unbiased variance var * (n / (n - 1)) rounds twice more
        a, b = (1 - momentum) * rm, momentum * mean
        out["running_mean"] = (a + b, SLACK * (momentum * e_mean + 3 * U * (a.abs() + b.abs())))
        vu = var * n / (n - 1)
        e_vu = e_var * n / (n - 1) + 2 * U * vu
        a, b = (1 - momentum) * rv, momentum * vu
        out["running_var"] = (a + b, SLACK * (momentum * e_vu + 3 * U * (a.abs() + b.abs())))
    else:
        out["running_mean"], out["running_var"] = (rm, torch.zeros_like(rm)), (rv, torch.zeros_like(rv))
    return out


def bn_backward_bounds(dy, x, gamma, eps, rm, rv, training, old_dg=None, old_db=None):
    """Bounds for dx, dgamma, dbeta of lafs_bn1d_bwd fed with the forward kernel's own save_mean / save_rstd (hence the statistics'
    bounds enter), next to the closed-form fp64 values (the test compares with fp64 autograd of nn.BatchNorm1d; these agree with it)."""
    n = x.shape[0]
    if training:
        mean, e_mean, _, _, rs, e_rs = bn_stats(x, eps)
    else:
        mean, e_mean, rs = rm, torch.zeros_like(rm), _rs(rv, eps)
        e_rs = 4 * U * rs
    xh, e_xh = bn_xhat(x, mean, e_mean, rs, e_rs)
    db = dy.sum(0)
    e_db = n * U * dy.abs().sum(0)
    dg = (dy * xh).sum(0)
    e_dg = (dy.abs() * e_xh).sum(0) + (n + 1) * U * (dy.abs() * (xh.abs() + e_xh)).sum(0)
    gr = gamma * rs
    e_gr = gamma.abs() * e_rs + U * gr.abs()
    if training:
        mb, mg = db / n, dg / n
        e_mb, e_mg = e_db / n + U * mb.abs(), e_dg / n + U * mg.abs()
        t2 = xh * mg
        e_t2 = e_xh * mg.abs() + xh.abs() * e_mg + e_xh * e_mg + U * t2.abs()
        inner = dy - mb - t2
        e_in = e_mb + e_t2 + 2 * U * (dy.abs() + mb.abs() + t2.abs())
    else:
        inner, e_in = dy, torch.zeros_like(dy)
    dx = gr * inner
    e_dx = SLACK * (e_gr * inner.abs() + gr.abs() * e_in + e_gr * e_in + U * dx.abs())
    if old_dg is not None:                               # the accumulate form: one more addition
        dg, e_dg = old_dg + dg, e_dg + U * (old_dg + dg).abs()
        db, e_db = old_db + db, e_db + U * (old_db + db).abs()
    return {"dx": (dx, e_dx), "dgamma": (dg, SLACK * e_dg), "dbeta": (db, SLACK * e_db)}
