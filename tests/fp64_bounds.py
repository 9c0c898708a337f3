"""The fp64 oracle of the kernel tests: plain fp64 restatements of the GEMM family's operations that carry, next to every value, a
bound on how far the kernel's value may lie from it, element by element (never normalised by a tensor's maximum).

The reference rounds to 16 bits exactly where include/lafs_hip.h says the kernel stores 16 bits, and nowhere else.  Where the kernel
stores a 16-bit value the bound is the distance to the neighbouring 16-bit values its unrounded value can reach (`flip`): 0 where no
rounding boundary lies within reach, so most 16-bit outputs must match the reference exactly.

Shared by tests/test_gpu_mlp_fused.py, tests/test_gpu_gemm.py, tests/test_gpu_wgrad.py and tests/test_oracle_gemm_host.py (which shows
on the CPU that the bounds are tight enough to mean something and that seeded faults fail them).  Everything here runs on whatever
device its arguments live on.  The case grids, input distributions and guarded buffers of the GEMM modules are in tests/gemm_cases.py."""
import math

import torch

bf16, f16, f32, f64 = torch.bfloat16, torch.float16, torch.float32, torch.float64
U = 2.0 ** -24          # fp32 unit roundoff
# |Phi(u) - kernel's (1 + erf(u / sqrt 2)) / 2|: Abramowitz-Stegun 7.1.26 (common.hpp erf_fast, |err| <= 1.5e-7) plus the fp32
# rounding of its ~15 operations on values <= 1.5
EPS_PHI = 1e-6

EPI_BF16, EPI_BF16_GELU, EPI_RESID_F32, EPI_F32, EPI_DGELU_BF16, EPI_ATOMIC_F32, EPI_EMBED_F32, EPI_BF16_ACT = range(8)   # LAFS_EPI_*
ACT_NONE, ACT_RELU, ACT_HSWISH, ACT_HSIGMOID = range(4)                                                                   # LAFS_ACT_*
F32_EPIS = (EPI_RESID_F32, EPI_F32, EPI_ATOMIC_F32, EPI_EMBED_F32)


# ------------------------------------------------------------------------------------------------ 16-bit rounding
def rbf(v):
    return v.to(f32).to(bf16).to(f64)


def rh(v):
    """fp16 counterpart of rbf (operand_f16 outputs)."""
    return v.to(f32).to(f16).to(f64)


def flip(v, e, r16=rbf):
    """16-bit rounding of a value the kernel holds to within +-e before it rounds: the reference r16(v) and the most the kernel's
    16-bit value can differ from it (rounding is monotone: the kernel's result lies between r16(v - e) and r16(v + e))."""
    r = r16(v)
    return r, torch.maximum(r16(v + e) - r, r - r16(v - e))


def step16(r, half=False):
    """One 16-bit step (the spacing of the format's values) at the reference value r: bf16 has 8 significant bits, fp16 11."""
    bits, emin = (11, -14) if half else (8, -126)
    ex = torch.floor(torch.log2(r.abs().clamp_min(2.0 ** emin)))
    return torch.exp2(ex - (bits - 1))


# ------------------------------------------------------------------------------------------------ contractions
def acc_factor(K, worst=False):
    """fp32 accumulation over K exact 16-bit products.  Of random sign: the partial sums walk like sqrt(k), so even rounding errors
    of one sign add up to < 1.4 sqrt(K) u sum|terms| (rounding toward zero); 3x margin: 4 sqrt(K).  worst: for operands that are NOT
    zero-mean (all-positive inputs) the random-walk argument does not hold -- every partial sum is as large as the sum of the terms
    before it -- and the worst case K u sum|terms| is used instead."""
    return float(K) if worst else 4 * math.sqrt(K)


def gemm(x, xe, w, bias=None, worst=False):
    """x w^T (+ bias) and a bound on the kernel's fp32 value, whose operand x is known to within xe."""
    K = w.shape[1]
    wa = w.abs()
    v, s = x @ w.t(), x.abs() @ wa.t()
    if bias is not None:
        v, s = v + bias, s + bias.abs()
    pe = None if xe is None else xe @ wa.t()
    if pe is not None:
        s = s + pe
    e = acc_factor(K, worst) * U * s
    # The bias, where the sums start, may collect K same-sign roundings (the worst-case form counts it among its terms already:
    # K additions of K + 1 terms).
    if bias is not None and not worst:
        e = e + K * U * bias.abs()
    return v, (e if pe is None else e + pe)


def gemm_tn(a, b, c_old=None, worst=False):
    """C = (C_old +) a^T b, the reduction running over the M rows (token axis): the two bounds of `gemm` with M in place of K.  The
    order of the sum is free (slices, workspaces and atomics are all allowed).  The accumulate / += forms add u |C_old + C_new|."""
    M = a.shape[0]
    v, s = a.t() @ b, a.abs().t() @ b.abs()
    e = acc_factor(M, worst) * U * s
    if c_old is not None:
        v = c_old + v
        # (worst case: C_old is one more term of the same sum -- M additions of M + 1 terms)
        e = e + (M * U * c_old.abs() if worst else U * v.abs() + U * c_old.abs())
    return v, e


def colsum(a, old=None, worst=False):
    """Column sums of a (bias gradient), added to `old` where given."""
    M = a.shape[0]
    v, e = a.sum(0), acc_factor(M, worst) * U * a.abs().sum(0)
    if old is not None:
        v = old + v
        e = e + (M * U * old.abs() if worst else U * v.abs() + U * old.abs())
    return v, e


# ------------------------------------------------------------------------------------------------ epilogues
def gelu(u, ue):
    cdf = 0.5 * (1 + torch.erf(u / math.sqrt(2)))
    pdf = torch.exp(-0.5 * u * u) / math.sqrt(2 * math.pi)
    g, dg = u * cdf, cdf + u * pdf
    # |gelu(u + d) - gelu(u)| <= |gelu'(u)| |d| + 0.4 d^2 (|gelu''| < 0.8); Phi off by EPS_PHI; 4 fp32 roundings
    ge = (dg.abs() + 0.4 * ue) * ue + u.abs() * EPS_PHI + 4 * U * (g.abs() + u.abs())
    # gelu'(u): |gelu''| < 0.8; Phi off by EPS_PHI; exp(-u^2 / 2) in fp32 good to (u^2 + 4) u relative
    dge = 0.8 * ue + EPS_PHI + 4 * U * (u.abs() * pdf * (u * u + 4) + dg.abs())
    return g, ge, dg, dge


def act(v, ve, kind):
    """act_f of common.hpp on a value known to within ve: relu max(v, 0); h-swish v relu6(v + 3) / 6; h-sigmoid relu6(v + 3) / 6.
    Bound = ve x the Lipschitz constant (1, 1.5 -- the slope of h-swish at its kink +3 --, 1/6) + a few u for the fp32 operations;
    where the whole interval [v - ve, v + ve] lies on a flat piece (below the kink 0 / -3, for h-sigmoid also above +3) the kernel's
    value is the constant itself and the bound is 0."""
    z = torch.zeros_like(v)
    if kind == ACT_NONE:
        return v, ve
    if kind == ACT_RELU:
        return v.clamp_min(0), torch.where(v + ve <= 0, z, ve)
    r6 = (v + 3).clamp(0, 6) / 6
    if kind == ACT_HSWISH:
        y = v * r6
        # v + 3 rounds (u |v + 3|, carried through |v| / 6), the two products round
        e = 1.5 * ve + U * (v.abs() * (v + 3).abs() / 6 + 3 * y.abs())
        return y, torch.where(v + ve <= -3, z, e)
    if kind == ACT_HSIGMOID:
        e = ve / 6 + U * ((v + 3).abs() / 6 + 2 * r6.abs())
        return r6, torch.where((v + ve <= -3) | (v - ve >= 3), z, e)
    raise ValueError(kind)


def resid(z, ze, r, s=None, drop=None):
    """The residual / DropPath epilogue resid + s (acc + bias) dropfactor: the product with the dropout factor rounds once (its
    1 / (1 - p) is no power of two), the scaled add twice."""
    t, te = z, ze
    if drop is not None:
        t, te = z * drop, ze * drop.abs() + U * (z * drop).abs()
    if s is not None:
        t, te = s * t, s.abs() * te
    y = r + t
    return y, te + 2 * U * (r.abs() + t.abs())


def embed(z, ze, pos_rows):
    """The embed epilogue acc + bias + pos[1 + m % npatch]: one more fp32 rounding."""
    y = z + pos_rows
    return y, ze + U * (y.abs() + pos_rows.abs())


def dgelu(z, ze, aux, save_grad, drop=None):
    """The GELU' epilogue acc * gelu'(aux) (aux = the bf16 pre-activation u) or, with LAFS_GELU_SAVE_GRAD, acc * aux as it is stored;
    then the dropout factor.  One fp32 rounding per product."""
    if save_grad:
        d, de = aux, torch.zeros_like(aux)
    else:
        _, _, d, de = gelu(aux, torch.zeros_like(aux))
    y = z * d
    ye = ze * d.abs() + z.abs() * de + ze * de + U * y.abs()
    if drop is not None:
        y, ye = y * drop, ye * drop.abs() + U * (y * drop).abs()
    return y, ye


def nt_reference(epi, A, B, bias=None, res=None, s=None, drop=None, aux=None, pos_rows=None, act_kind=0, save_grad=False,
                 half=False, worst=False, n_atomic=0):
    """Every tensor lafs_gemm_nt stores for one request, as {name: (reference, bound, 16-bit output?)}; fp64 arguments (the 16-bit
    operands widened exactly).  n_atomic: K slices an ATOMIC_F32 request adds into C (one fp32 rounding of the running sum each)."""
    r16 = rh if half else rbf
    z, ze = gemm(A, None, B, None if epi in (EPI_DGELU_BF16, EPI_ATOMIC_F32) else bias, worst=worst)
    if epi == EPI_BF16:
        return {"C": flip(z, ze, r16) + (True,)}
    if epi == EPI_F32:
        return {"C": (z, ze, False)}
    if epi == EPI_ATOMIC_F32:
        return {"C": (z, ze + n_atomic * U * (A.abs() @ B.abs().t()), False)}
    if epi == EPI_BF16_GELU:
        g, ge, dg, dge = gelu(z, ze)
        if drop is not None:
            g, ge = g * drop, ge * drop.abs() + U * (g * drop).abs()
        return {"C": (flip(dg, dge) if save_grad else flip(z, ze)) + (True,), "C2": flip(g, ge) + (True,)}
    if epi == EPI_RESID_F32:
        return {"C": resid(z, ze, res, s, drop) + (False,)}
    if epi == EPI_EMBED_F32:
        return {"C": embed(z, ze, pos_rows) + (False,)}
    if epi == EPI_DGELU_BF16:
        return {"C": flip(*dgelu(z, ze, aux, save_grad, drop)) + (True,)}
    if epi == EPI_BF16_ACT:
        if aux is not None:
            z, ze = z + aux, ze + U * (z + aux).abs()
        return {"C": flip(*act(z, ze, act_kind), r16) + (True,)}
    raise ValueError(epi)


# ------------------------------------------------------------------------------------------------ checks
def check(name, got, ref, bound, is16=None):
    """|got - ref| <= bound for every element, or an AssertionError naming the first offender.  Prints the two
    figures of a case: the worst |err| / bound over the elements with a non-zero bound, and -- for a 16-bit output -- the share of
    elements whose bound is 0 (they must match the reference bit for bit)."""
    got, ref, bound = got.double(), ref.double(), bound.double()
    if got.dim() == 1:
        got, ref, bound = got[None], ref[None], bound[None]
    got, ref, bound = got.reshape(-1, got.shape[-1]), ref.reshape(-1, ref.shape[-1]), bound.reshape(-1, bound.shape[-1])
    fin = torch.isfinite(got)
    if not bool(fin.all()):
        rows = (~fin).any(1).nonzero().flatten()
        raise AssertionError(f"{name}: {int((~fin).sum())} non-finite values in {rows.numel()} rows, first rows {rows[:8].tolist()}")
    err = (got - ref).abs()
    nz = bound > 0
    ratio = float((err[nz] / bound[nz]).max()) if bool(nz.any()) else 0.0
    exact = 1.0 - float(nz.double().mean()) if nz.numel() else 1.0
    line = f"{name}: worst |err|/bound {ratio:.3f}" + (f", bound 0 on {100 * exact:.1f} % of the 16-bit outputs" if is16 else "")
    print(line)
    bad = err > bound
    if bool(bad.any()):
        rows = bad.any(1).nonzero().flatten()
        r = int(rows[0])
        c = int(bad[r].nonzero()[0])
        raise AssertionError(f"{name}: {int(bad.sum())} values in {rows.numel()} rows out of bounds (first rows {rows[:8].tolist()}); "
                             f"[{r}, {c}]: kernel {float(got[r, c]):.9g}, fp64 reference {float(ref[r, c]):.9g}, bound {float(bound[r, c]):.3g}")
    return ratio, exact
