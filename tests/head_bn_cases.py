"""Shared by the BatchNorm DINO head tests (test_head_bn_host.py, test_gpu_head_bn.py, test_gpu_head_bn_module.py,
test_gpu_step_head_bn.py): the case grid and inputs of lafs_bn1d_gelu_fwd / _bwd, their fp64 reference with per-element bounds, an fp32
emulation of the kernels' formulas (with seedable faults) and the F29 / F30 fixture loaders.

The bounds count the roundings of the kernels' formulas and never look at a kernel's output.  They are composed of
  fvit_cases.bn_forward_reference   y = xhat gamma + beta with the statistics' bounds (the arithmetic of lafs_bn1d_fwd, shared through
                                    csrc/bn_rows.hpp), save_mean / save_rstd and the running buffers
  fp64_bounds.gelu                  gelu(y) and gelu'(y) of a y known to within its bound (erf by Abramowitz-Stegun 7.1.26)
  fp64_bounds.flip                  the bf16 store: 0 where no rounding boundary lies within reach
  fvit_cases.bn_backward_bounds     dgamma, dbeta and dx of the BatchNorm backward for an EXACT incoming gradient
The BatchNorm backward is linear in its incoming gradient g = da gelu'(y), which the kernel holds to within e_g: what e_g adds to each
output is propagated with absolute values (`_perturb`) on top of bn_backward_bounds at the fp64 g."""
import glob
import os

import torch

import fp64_bounds as fb
from conftest import GOLDEN, load_golden
from fvit_cases import SLACK, U, _rs, bn_backward_bounds, bn_forward_reference, bn_stats, bn_xhat

f32, f64 = torch.float32, torch.float64
EPS, MOM = 1e-5, 0.1
# (n, D, ld): one row pair; ld > D; nothing a multiple of 64; rows beyond one pass of the 8 waves; the two shapes of the C2 step
SHAPES = [(2, 64, 64), (5, 128, 160), (37, 200, 208), (130, 256, 256), (128, 2048, 2048), (640, 2048, 2048)]
_CACHE = {}


def f32val(v):
    return float(torch.tensor(v, dtype=f32))


def inputs(n, D):
    """fp32 inputs on the CPU, made once per case and left unchanged.  Column 0 is constant over the rows (batch variance 0: rstd =
    eps^-1/2), column 1 has mean 1000 and spread 1e-2 (a one-pass variance cancels there)."""
    key = (n, D)
    if key not in _CACHE:
        g = torch.Generator().manual_seed(n * 1000 + D)
        r = lambda *s: torch.randn(*s, generator=g)
        u = r(n, D) * (0.5 + torch.rand(D, generator=g)) + r(D)
        u[:, 0] = 0.37
        u[:, 1] = 1000.0 + 1e-2 * r(n)
        _CACHE[key] = dict(u=u, gamma=1 + 0.1 * r(D), beta=0.1 * r(D), rm=0.1 * r(D), rv=1 + 0.2 * torch.rand(D, generator=g),
                           da=r(n, D), old_dg=r(D), old_db=r(D))
    return _CACHE[key]


# ------------------------------------------------------------------------------------------------ fp64 reference + bounds
def forward_reference(c, training):
    """{name: (fp64 value, bound)} of everything lafs_bn1d_gelu_fwd writes ("a": the bf16 store), plus "y" (never stored)."""
    d = lambda k: c[k].double()
    out = bn_forward_reference(d("u"), d("gamma"), d("beta"), f32val(EPS), f32val(MOM), d("rm"), d("rv"), training)
    y, ye = out["y"]
    g, ge, _, _ = fb.gelu(y, ye)
    out["a_f32"] = (g, ge)
    out["a"] = fb.flip(g, ge)
    return out


def _perturb(eg, x, gamma, eps, rm, rv, training):
    """What an elementwise error <= eg of the incoming gradient adds to (dx, dgamma, dbeta) of the BatchNorm backward."""
    n = x.shape[0]
    if training:
        mean, e_mean, _, _, rs, e_rs = bn_stats(x, eps)
    else:
        mean, e_mean, rs = rm, torch.zeros_like(rm), _rs(rv, eps)
        e_rs = 4 * U * rs
    xh, e_xh = bn_xhat(x, mean, e_mean, rs, e_rs)
    xa = xh.abs() + e_xh
    db, dg = eg.sum(0), (eg * xa).sum(0)
    gr = (gamma * rs).abs() + gamma.abs() * e_rs
    dx = gr * (eg + db / n + xa * dg / n) if training else gr * eg
    return SLACK * dx, SLACK * dg, SLACK * db


def backward_reference(c, training, accumulate):
    """{name: (fp64 value, bound)} of what lafs_bn1d_gelu_bwd writes when it is fed the forward kernel's save_mean / save_rstd:
    "du" (the bf16 store), "dgamma", "dbeta"; plus "g" = da gelu'(y) (never stored)."""
    d = lambda k: c[k].double()
    eps = f32val(EPS)
    y, ye = bn_forward_reference(d("u"), d("gamma"), d("beta"), eps, f32val(MOM), d("rm"), d("rv"), training)["y"]
    _, _, dg_, dge = fb.gelu(y, ye)
    g = d("da") * dg_
    eg = d("da").abs() * dge + U * g.abs()
    old = dict(old_dg=d("old_dg"), old_db=d("old_db")) if accumulate else {}
    b = bn_backward_bounds(g, d("u"), d("gamma"), eps, d("rm"), d("rv"), training, **old)
    pdx, pdg, pdb = _perturb(eg, d("u"), d("gamma"), eps, d("rm"), d("rv"), training)
    dx, e_dx = b["dx"][0], b["dx"][1] + pdx
    return {"g": (g, eg), "du_f32": (dx, e_dx), "du": fb.flip(dx, e_dx), "dgamma": (b["dgamma"][0], b["dgamma"][1] + pdg),
            "dbeta": (b["dbeta"][0], b["dbeta"][1] + pdb)}


# ------------------------------------------------------------------------------------------------ fp32 emulation of the kernels
def _erf_fast(x):
    ax = x.abs()
    t = 1.0 / (1.0 + 0.3275911 * ax)
    poly = ((((1.061405429 * t - 1.453152027) * t + 1.421413741) * t - 0.284496736) * t + 0.254829592) * t
    return torch.copysign(1.0 - poly * torch.exp2(-1.4426950408889634 * ax * ax), x)


def _gelu32(x, tanh=False):
    if tanh:
        return 0.5 * x * (1.0 + torch.tanh(0.7978845608028654 * (x + 0.044715 * x * x * x)))
    return 0.5 * x * (1.0 + _erf_fast(x * 0.70710678118654752))


def _gelu_grad32(x):
    ax = x.abs() * 0.70710678118654752
    t = 1.0 / (1.0 + 0.3275911 * ax)
    poly = ((((1.061405429 * t - 1.453152027) * t + 1.421413741) * t - 0.284496736) * t + 0.254829592) * t
    e = torch.exp2(-1.4426950408889634 * ax * ax)
    cdf = 0.5 + 0.5 * torch.copysign(1.0 - poly * e, x)
    return cdf + x * (0.39894228040143268 * e)


def emulate_forward(c, training, fault=None):
    """The forward kernel's formulas in fp32 on the CPU (torch's own summation order: the bounds are order-free).
    fault: "one_pass_var" | "biased_running_var" | "tanh_gelu"."""
    u, gamma, beta, rm, rv = (c[k].clone() for k in ("u", "gamma", "beta", "rm", "rv"))
    n = u.shape[0]
    eps, mom = torch.tensor(EPS, dtype=f32), torch.tensor(MOM, dtype=f32)
    if training:
        mean = u[0] + (u - u[0]).sum(0) / n
        var = ((u * u).sum(0) / n - mean * mean).clamp_min(0) if fault == "one_pass_var" else ((u - mean) ** 2).sum(0) / n
        rstd = 1.0 / torch.sqrt(var + eps)
        unb = var if fault == "biased_running_var" else var * (n / (n - 1.0))
        rm = (1.0 - mom) * rm + mom * mean
        rv = (1.0 - mom) * rv + mom * unb
    else:
        mean, rstd = rm, 1.0 / torch.sqrt(rv + eps)
    y = (u - mean) * rstd * gamma + beta
    a = _gelu32(y, tanh=fault == "tanh_gelu").to(torch.bfloat16)
    return dict(a=a, save_mean=mean, save_rstd=rstd, running_mean=rm, running_var=rv)


def emulate_backward(c, training, accumulate, fault=None):
    """The backward kernel's formulas in fp32 from the (fault-free) emulated forward's statistics.
    fault: "gelu_grad_at_u" | "no_xhat_term" | "n_minus_1" | "dgamma_without_xhat" | "eval_with_batch_terms"."""
    fw = emulate_forward(c, training)
    u, gamma, beta, da = c["u"], c["gamma"], c["beta"], c["da"]
    n = u.shape[0]
    mean, rstd = fw["save_mean"], fw["save_rstd"]
    xh = (u - mean) * rstd
    y = xh * gamma + beta
    g = da * _gelu_grad32(u if fault == "gelu_grad_at_u" else y)
    sb, sg = g.sum(0), (g if fault == "dgamma_without_xhat" else g * xh).sum(0)
    dgamma = c["old_dg"] + sg if accumulate else sg
    dbeta = c["old_db"] + sb if accumulate else sb
    nf = float(n - 1) if fault == "n_minus_1" else float(n)
    batch = training or fault == "eval_with_batch_terms"
    mb, mg = (sb / nf, sg / nf) if batch else (torch.zeros_like(sb), torch.zeros_like(sg))
    if fault == "no_xhat_term":
        mg = torch.zeros_like(mg)
    du = ((gamma * rstd) * (g - mb - xh * mg)).to(torch.bfloat16)
    return dict(du=du, dgamma=dgamma, dbeta=dbeta)


# ------------------------------------------------------------------------------------------------ fixtures
ZERO_SUM = ("mlp.0.bias", "mlp.3.bias")         # Linear biases directly in front of a training-mode BatchNorm: their gradient vanishes
# F30 (the whole step): the same column sum reaches the backbone's final LayerNorm bias through W0^T (tools/make_golden_head_bn.py)
ZERO_SUM_STEP = {"head.mlp.0.bias": "head.mlp.0.weight", "head.mlp.3.bias": "head.mlp.3.weight", "backbone.norm.bias": "backbone.norm.weight"}
BN_BUFFERS = ("running_mean", "running_var", "num_batches_tracked")
HEAD_BN_KEYS = tuple(f"mlp.{i}.{k}" for i in (1, 4) for k in BN_BUFFERS)
F29_HEAD = dict(in_dim=128, out_dim=1000, use_bn=True, hidden_dim=256, bottleneck_dim=64)
F30_K, F30_B, F30_NLOCAL = 512, 4, 2
F30_VIT = dict(img_size=[112], patch_size=8, embed_dim=64, depth=2, num_heads=1, qkv_bias=True)
F30_HEAD = dict(use_bn=True, hidden_dim=128, bottleneck_dim=64)


def _load_parts(stem):
    out = {}
    paths = sorted(p for p in glob.glob(os.path.join(GOLDEN, stem + "*.npz"))
                   if os.path.basename(p)[len(stem):-4].lstrip("_").isdigit() or os.path.basename(p)[:-4] == stem)
    assert paths, f"fixture {stem} is missing (tools/make_golden_head_bn.py)"
    for path in paths:
        part = load_golden(os.path.basename(path)[:-4])
        assert not set(part) & set(out), path
        out.update(part)
    return out


def load_f29():
    if "f29" not in _CACHE:
        _CACHE["f29"] = _load_parts("f29_head_bn")
    return _CACHE["f29"]


def load_f30():
    if "f30" not in _CACHE:
        _CACHE["f30"] = _load_parts("f30_lafs_step_head_bn")
    return _CACHE["f30"]
