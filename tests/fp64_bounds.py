"""The fp64 oracle of the kernel tests: plain fp64 restatements of the GEMM family's, the LayerNorm family's, the arena step's and the
DINO head's and loss's operations that carry, next to every value, a
bound on how far the kernel's value may lie from it, element by element (never normalised by a tensor's maximum).

The reference rounds to 16 bits exactly where include/lafs_hip.h says the kernel stores 16 bits, and nowhere else.  Where the kernel
stores a 16-bit value the bound is the distance to the neighbouring 16-bit values its unrounded value can reach (`flip`): 0 where no
rounding boundary lies within reach, so most 16-bit outputs must match the reference exactly.

(The landmark CNN's kernels use the building blocks of the last section from tests/cnn_cases.py, judged on the CPU by
tests/test_oracle_cnn_host.py.)
Shared by tests/test_gpu_mlp_fused.py, tests/test_gpu_gemm.py, tests/test_gpu_wgrad.py, tests/test_gpu_layernorm.py, tests/test_gpu_optim.py,
tests/test_gpu_dino_head.py and the three CPU modules tests/test_oracle_gemm_host.py, tests/test_oracle_rowops_host.py and
tests/test_oracle_dino_host.py (which show that the bounds are tight
enough to mean something and that seeded faults fail them).  Everything here runs on whatever
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


# ------------------------------------------------------------------------------------------------ row operations (LayerNorm)
# rsqrtf: no accuracy table of the device library ships with the toolchain, so the allowance is a measurement --
# tests/test_gpu_layernorm.py::test_rsqrtf_allowance feeds lafs_layernorm_fwd rows (-a, -a, a, a) with 11-bit a (mean 0, variance a^2
# and the fp32 sum a^2 + eps all exact up to the one rounding the reference repeats) and compares rstd with the fp64 value: the worst
# of 40 000 arguments over [1e-6, 1e6] was 0.82 ulp on the MI355X.  Allowed here: 2 ulp = 4 u relative.
RSQ_REL = 4 * U
# powf: 1 ulp (the figure of HIP's published math-API table) = 2 u relative; cannot be measured apart from the kernel
POW_REL = 2 * U


def f32c(v):
    """The fp32 value of a Python constant, widened: the operand a kernel holds for a literal or a float argument."""
    return float(torch.tensor(v, dtype=f32))


def sum_depth(D):
    """Most fp32 additions a term of a LayerNorm row sum passes through: a lane adds its <= 32 values (4 per 256-column chunk, or per
    128-column chunk in the two-rows-per-wave kernels) in sequence, a butterfly over <= 64 lanes follows.  A sum of D terms of any
    sign is then off by at most depth u sum|terms|."""
    return min(32, 4 * -(-D // 128)) + 6


def rsqrt_iv(v, ve):
    """rsqrtf of a positive value known to within ve: the fp64 value and the widest distance to what the interval's ends give
    (exact, not first order: infinite where the interval reaches 0), plus the RSQ_REL allowance of the instruction."""
    r = v.rsqrt()
    re = torch.maximum((v - ve).clamp_min(0).rsqrt() - r, r - (v + ve).rsqrt())
    return r, re + RSQ_REL * (r + re)


def ln_fwd(x, gamma, beta, eps):
    """lafs_layernorm_fwd on exact fp32 rows x [R, D] (eps: the fp32 value): {"y": fp32 output, "y16": its bf16 store, "mean",
    "rstd"}, each (reference, bound).
    mean:  a sum of D terms of depth sum_depth(D), one division
    var:   two-pass -- sum (x - mean')^2 = sum (x - mean)^2 + D dm^2 for the kernel's mean' = mean + dm, so the mean's error enters
           squared; every term rounds three times (difference, square, product / fma) before the sum of depth sum_depth; / D; + eps
    rstd:  rsqrt_iv
    y:     (x - mean') rstd' gamma + beta: the difference and the product round, the last product and sum round once each (or once
           together as an fma)"""
    D = x.shape[1]
    dep = sum_depth(D)
    m = x.mean(1, keepdim=True)
    me = dep * U * x.abs().mean(1, keepdim=True) + U * m.abs()
    c = x - m
    var = (c * c).mean(1, keepdim=True)
    ve = me * me + (dep + 4) * U * (var + me * me) + U * (var + eps)
    r, re = rsqrt_iv(var + eps, ve)
    xh = c * r
    he = (r + re) * me + c.abs() * re + 2 * U * (c.abs() + me) * (r + re)
    y = xh * gamma + beta
    ye = gamma.abs() * he + U * (xh * gamma).abs() + U * y.abs()
    return {"y": (y, ye), "y16": flip(y, ye), "mean": (m, me), "rstd": (r, re)}


def ln_bwd(dy, x, mean, rstd, gamma, g_old=None, s=None, drop=None, dgamma_old=None, dbeta_old=None):
    """lafs_layernorm_bwd on exact operands (dy: the bf16 or fp32 gradient widened; mean, rstd [R, 1]: the fp32 statistics the kernel
    is handed): {"g": the gradient stream (g_old + dx, or dx), "gb": its scaled / dropped-out bf16 copy, "dgamma", "dbeta"}.
    xhat = (x - mean) rstd rounds twice; d = dy gamma once; the row means m1 = mean(d), m2 = mean(d xhat) are sums of depth
    sum_depth(D) over terms that carry those errors, then a division; dx = rstd (d - m1 - xhat m2): three roundings inside, one
    outside; the accumulate add rounds once; gb: the scale and the dropout factor round once each before the 16-bit store.
    dgamma / dbeta: `colsum` over the rows with the old value as one more term (any order: slots or atomics), plus the three
    roundings each term dy xhat carries."""
    D = x.shape[1]
    dep = sum_depth(D)
    xh = (x - mean) * rstd
    xhe = 2 * U * xh.abs()
    d = dy * gamma
    de = U * d.abs()
    m1 = d.mean(1, keepdim=True)
    m1e = (de.sum(1, keepdim=True) + dep * U * d.abs().sum(1, keepdim=True)) / D + U * m1.abs()
    p = d * xh
    pe = de * xh.abs() + d.abs() * xhe + U * p.abs()
    m2 = p.mean(1, keepdim=True)
    m2e = (pe.sum(1, keepdim=True) + dep * U * p.abs().sum(1, keepdim=True)) / D + U * m2.abs()
    dx = rstd * (d - m1 - xh * m2)
    dxe = rstd * (de + m1e + xh.abs() * m2e + xhe * (m2.abs() + m2e) + 3 * U * (d.abs() + m1.abs() + (xh * m2).abs())) + U * dx.abs()
    g, ge = (dx, dxe) if g_old is None else (g_old + dx, dxe + U * (g_old + dx).abs())
    f = torch.ones_like(g) if s is None else s.expand_as(g)
    if drop is not None:
        f = f * drop
    out = {"g": (g, ge), "gb": flip(f * g, f.abs() * ge + 2 * U * (f * g).abs())}
    a = dy * xh
    z = torch.zeros(1, D, dtype=f64, device=x.device)
    v, e = colsum(torch.cat([a, z if dgamma_old is None else dgamma_old[None]]))
    out["dgamma"] = (v, e + 3 * U * a.abs().sum(0))
    out["dbeta"] = colsum(torch.cat([dy, z if dbeta_old is None else dbeta_old[None]]))
    return out


# ------------------------------------------------------------------------------------------------ the arena step (optim.hip)
CHUNK = 1024
SEG_DECAY, SEG_LAST_LAYER, SEG_TRAINABLE, SEG_LOW_DECAY = 1, 2, 4, 8                                                        # LAFS_SEG_*
HP_LR, HP_WD, HP_BETA1, HP_BETA2, HP_EPS, HP_CLIP, HP_EMA_M, HP_FREEZE_LAST, HP_GRAD_SCALE, HP_WD_LOW = range(10)            # LAFS_HP_*


def sumsq(grad, chunk_seg, n_seg, gs):
    """lafs_grad_sumsq: per tensor sum (gs g)^2 over its chunks (grad [n_chunks, 1024] fp64).  Same-sign terms, so the worst-case form
    of `colsum` -- but over the depth of the kernel's fixed summation tree instead of the element count: a square rounds (1), a lane
    adds 16 of them, a 64-lane butterfly (6); then a thread adds ceil(chunks / 256) chunk sums, a butterfly (6), four wave sums (3),
    and gs multiplies twice (2)."""
    cs = (grad * grad).sum(1)
    ss = torch.zeros(n_seg, dtype=f64, device=grad.device).index_add_(0, chunk_seg.long(), cs)
    nc = torch.bincount(chunk_seg.long(), minlength=n_seg).double()
    depth = 1 + 16 + 6 + torch.ceil(nc / 256) + 6 + 3 + 2
    v = ss * gs * gs
    return v, depth * U * v


def clip_scale(ss, sse, clip, gs):
    """The gradient factor of clip_adamw_ema_kernel per tensor: gs, times coef = clip / (sqrtf(ss) + 1e-6f) where coef < 1.  Returns
    (factor, bound, knife): sqrtf, the add and the division round once each on top of what ss carries.  Where the fp64 coefficient
    lies within its bound of 1 (`knife`) the kernel may take either branch, and the bound covers both."""
    if not clip > 0:
        return torch.full_like(ss, gs), torch.zeros_like(ss), torch.zeros_like(ss, dtype=torch.bool)
    n = ss.sqrt()
    ne = torch.maximum((ss + sse).sqrt() - n, n - (ss - sse).clamp_min(0).sqrt()) + U * n
    den = n + f32c(1e-6)
    dene = ne + U * den
    coef = clip / den
    ce = clip / (den - dene) - coef + U * coef
    knife = (coef - 1).abs() <= ce
    ref = gs * coef.clamp_max(1.0)
    e = gs * ce + U * ref
    e = torch.where(coef - ce >= 1, torch.zeros_like(e), e)
    e = torch.where(knife, gs * (ce + (coef - 1).abs()) + U * gs, e)
    return ref, e, knife


def adamw_ema(p, g, m, v, t, chunk_seg, flags, step, ss, sse, hp):
    """One lafs_clip_adamw_ema launch on fp64 copies of its fp32 state ([n_chunks, 1024] each; t: the teacher, or None), restated
    after torch.optim.AdamW (decoupled decay, bias corrections, eps outside the root) with utils.clip_gradients per tensor and the
    teacher EMA.  hp: the fp32 hyper-parameter vector widened -- the operands the kernel has.  step: seg_step before the launch.
    Returns {"param", "m", "v", "teacher", "param16", "teacher16"} as (reference, bound), "seg_step" (exact) and "knife" (how many
    tensors' clip branch is undecided).  Every fp32 operation of the kernel rounds once (u times its result), errors are carried
    forward by the first-order terms written out below and by exact intervals through the divisions and roots; powf is allowed
    POW_REL, so bc = 1 - beta^t is off by POW_REL beta^t -- at t = 1 and beta2 = 0.999 that is 1000 x POW_REL of bc2 itself, which
    the bound then carries into the update.  Where sqrt(v) / sqrt(bc2) is comparable to eps the denominator's interval is wide
    relative to itself and the bound widens through the quotient."""
    lr, wd, b1, b2, eps, clip, em, frz, gs, wdl = (float(hp[i]) for i in range(10))
    fl = flags.long()
    upd_s = ((fl & SEG_TRAINABLE) != 0) & ~(((fl & SEG_LAST_LAYER) != 0) & (frz != 0))
    new_step = step.long() + upd_s.long()
    cs = chunk_seg.long()
    col = lambda x: x[cs][:, None]
    upd = col(upd_s)
    wd_s = ((fl & SEG_DECAY) != 0).double() * wd
    wd_s[(fl & SEG_LOW_DECAY) != 0] = wdl
    gsc_s, gsce_s, knife = clip_scale(ss, sse, clip, gs)
    tt = new_step.double().clamp_min(1)
    o1, o2, oem = f32c(1.0) - b1, f32c(1.0) - b2, f32c(1.0) - em          # (1 - beta: exact in fp32 for beta in [0.5, 1])
    pw1, pw2 = b1 ** tt, b2 ** tt
    bc1, bc2 = 1 - pw1, 1 - pw2
    bc1e, bc2e = POW_REL * pw1 + U * bc1, POW_REL * pw2 + U * bc2
    ssz = lr / bc1
    ssze = lr / (bc1 - bc1e) - ssz + U * ssz
    isb, isbe = rsqrt_iv(bc2, bc2e)
    dec = 1 - lr * wd_s
    dece = U * lr * wd_s + U * dec
    gsc, gsce, ssz, ssze, isb, isbe, dec, dece = (col(x) for x in (gsc_s, gsce_s, ssz, ssze, isb, isbe, dec, dece))
    gg = g * gsc
    gge = g.abs() * gsce + U * gg.abs()
    p1 = p * dec
    p1e = p.abs() * dece + U * p1.abs()
    mn = m * b1 + gg * o1
    mne = o1 * gge + 2 * U * ((m * b1).abs() + (gg * o1).abs()) + U * mn.abs()
    vn = v * b2 + gg * gg * o2
    vne = o2 * (2 * gg.abs() * gge + gge * gge) + 3 * U * (v * b2 + gg * gg * o2) + U * vn
    sv = vn.sqrt()
    sve = torch.maximum((vn + vne).sqrt() - sv, sv - (vn - vne).clamp_min(0).sqrt()) + U * sv
    den = sv * isb + eps
    dene = sve * (isb + isbe) + sv * isbe + U * sv * isb + U * den
    num = ssz * mn
    nume = ssze * mn.abs() + (ssz + ssze) * mne + U * num.abs()
    q = num / den
    qe = (num.abs() + nume) / (den - dene) - q.abs() + U * q.abs()
    pn = p1 - q
    pne = p1e + qe + U * pn.abs()
    z = torch.zeros_like(p)
    out = {"seg_step": new_step, "knife": int(knife[upd_s].sum())}
    P, Pe = torch.where(upd, pn, p), torch.where(upd, pne, z)
    out["param"] = (P, Pe)
    out["m"] = (torch.where(upd, mn, m), torch.where(upd, mne, z))
    out["v"] = (torch.where(upd, vn, v), torch.where(upd, vne, z))
    out["param16"] = flip(P, Pe)
    if t is not None:
        tn = t * em + oem * P
        tne = oem * Pe + 2 * U * ((t * em).abs() + (oem * P).abs()) + U * tn.abs()
        out["teacher"] = (tn, tne)
        out["teacher16"] = flip(tn, tne)
    return out


# ------------------------------------------------------------------------------------------------ the DINO head and loss (head.hip,
# dino_loss.hip, dino_head_loss.hip)
# v_exp_f32 / v_log_f32: 1 ulp, 2x margin (the allowance of tests/test_gpu_attention_cls.py); a flushed denormal result adds TINY
EXP_REL = 4 * U
LOG_REL = 4 * U
ULP1 = 2 * U            # sqrtf and `/` under the project's default flags: 1 ulp
TINY = 2.0 ** -126
LOG2E, LN2 = 1.4426950408889634, 0.6931471805599453
HEAD_DEPTH = 16 + 6     # head.hip row sums: a lane adds its 4 float4 (16 terms) in sequence, a 6-step butterfly follows


def inv32(t):
    """fl(1.0f / t) for the fp32 value of t, widened: the reciprocal temperature a kernel holds."""
    return float(torch.tensor(1.0, dtype=f32) / torch.tensor(t, dtype=f32))


def dino_coef(ncrops, B, student_temp, grad_scale, dev_student_temp=None):
    """coef = grad_scale / ((2 ncrops - 2) B tau_s) as the host forms it in fp32 and, where device temperatures are given, the
    kernels' correction coef / (fl(1 / tau_s) dev_tau_s), which swaps the host's tau_s for the device's.  The correction's division
    runs on the device (1 ulp); the caller allows ULP1 relative for it."""
    t = lambda v: torch.tensor(v, dtype=f32)
    coef = t(grad_scale) / (t(float(2 * ncrops - 2)) * t(float(B)) * t(student_temp))
    if dev_student_temp is not None:
        coef = coef / ((t(1.0) / t(student_temp)) * t(dev_student_temp))
    return float(coef)


def _sumsq_row(x):
    """Row sums of squares as head.hip forms them: same-sign terms, each square rounds (1), then HEAD_DEPTH additions."""
    ss = (x * x).sum(1, keepdim=True)
    return ss, (HEAD_DEPTH + 1) * U * ss


def _row_dot(y, ye, d):
    """s = sum_c y d over a row of head.hip's backward kernels (y known to within ye, d exact): every product rounds, the sum has
    depth HEAD_DEPTH."""
    t = y * d
    s = t.sum(1, keepdim=True)
    return s, (ye * d.abs() + U * t.abs()).sum(1, keepdim=True) + HEAD_DEPTH * U * t.abs().sum(1, keepdim=True)


def _proj(f, fe, d, y, ye, s, se):
    """f (d - y s), the tangent projection both backward kernels end with: y s and the difference round (or once as an fma), the
    product with f rounds."""
    ys = y * s
    inner = d - ys
    ie = ye * s.abs() + (y.abs() + ye) * se + U * ys.abs() + U * (d.abs() + ys.abs())
    o = f * inner
    return o, f.abs() * ie + fe * (inner.abs() + ie) + U * o.abs()


def l2norm_fwd(x):
    """lafs_l2norm_fwd on exact fp32 rows x [R, D]: {"inv": 1 / max(sqrtf(sum x^2), 1e-12f) [R, 1], "y": x inv, "y16": its bf16 store}, each
    (reference, bound).  The sum of squares is carried as an interval through the root (1 ulp), the clamp (both ends clamped: a row
    wholly below it has inv = fl(1 / 1e-12f) up to the division's ulp) and the division (1 ulp); y = x inv rounds once."""
    ss, sse = _sumsq_row(x)
    n = ss.sqrt()
    ne = torch.maximum((ss + sse).sqrt() - n, n - (ss - sse).clamp_min(0).sqrt()) + ULP1 * n
    c = f32c(1e-12)
    d, lo, hi = n.clamp_min(c), (n - ne).clamp_min(c), (n + ne).clamp_min(c)
    inv = 1 / d
    inve = torch.maximum(1 / lo - inv, inv - 1 / hi) + ULP1 * inv
    y = x * inv
    ye = x.abs() * inve + U * y.abs()
    return {"inv": (inv, inve), "y": (y, ye), "y16": flip(y, ye)}


def l2norm_bwd(x, dy, inv):
    """lafs_l2norm_bwd: dx = inv (dy - y <y, dy>) with y = x inv recomputed in fp32 (one rounding), on the inv_norm [R, 1] the kernel is
    handed."""
    y = x * inv
    ye = U * y.abs()
    s, se = _row_dot(y, ye, dy)
    return _proj(inv, torch.zeros_like(inv), dy, y, ye, s, se)


def weightnorm_fwd(v, g):
    """lafs_weightnorm_fwd on the K live rows: {"inv": rsqrtf(sum v^2) [K, 1], "w": v (g inv), "w16": its bf16 store}; g [K, 1].  (Pad rows are exactly
    0 and w_t is a bitwise transpose: neither needs a bound.)"""
    ss, sse = _sumsq_row(v)
    inv, inve = rsqrt_iv(ss, sse)
    sc = g * inv
    sce = g.abs() * inve + U * sc.abs()
    w = v * sc
    we = v.abs() * sce + U * w.abs()
    return {"inv": (inv, inve), "w": (w, we), "w16": flip(w, we)}


def weightnorm_bwd(dw, v, g, inv, dv_old=None, dg_old=None):
    """lafs_weightnorm_bwd on the inv_norm [K, 1] it is handed: vhat = v inv (one rounding), s = <dw, vhat>, dg = (dg_old +) s,
    dv = (dv_old +) (g inv) (dw - vhat s).  Returns {"dv", "dg"}."""
    vh = v * inv
    vhe = U * vh.abs()
    s, se = _row_dot(vh, vhe, dw)
    f = g * inv
    dv, dve = _proj(f, U * f.abs(), dw, vh, vhe, s, se)
    dg, dge = s, se
    if dg_old is not None:
        dg = dg_old + s
        dge = se + U * dg.abs()
    if dv_old is not None:
        dv = dv_old + dv
        dve = dve + U * dv.abs()
    return {"dv": (dv, dve), "dg": (dg, dge)}


def scaled_logits(z, ze, it, center=None, dev=False):
    """a = (z - center) it, the argument of every exponential of the loss kernels, and the bound on the kernel's fp32 value of it: z
    known to within ze; the subtraction rounds; the product rounds (1) and the constant it runs with is itself rounded (1: the
    fp32 product it log2(e) of the log2-domain kernels, or the log2(e) inside __expf); with device temperatures 1.0f / temp is
    a device division (ULP1)."""
    d = z if center is None else z - center
    a = d * it
    sub = 0 if center is None else U * d.abs()
    return a, it * (ze + sub) + (2 * U + (ULP1 if dev else 0)) * a.abs()


def lse_rows(z, ze, inv_temp, center=None, n_exp=1, n_round=1, dev=False, ln2_product=True, parts=False):
    """Natural log-sum-exp of the rows of (z - center) inv_temp, logits known to within ze: (lse [R, 1], bound, A = the row's largest
    |argument|).  lse is 1-Lipschitz in the maximum norm of its arguments, so the arguments' worst error passes through unscaled.
    parts: also the bound without the logits' own error inv_temp ze (see `dino_loss`: what is left when that error is common to the
    log-sum-exp and to an argument it is subtracted from), which includes the second-order term 2 (inv_temp max ze)^2.
    On top: a term exp(a_k - M) reaches the sum through at most n_exp exponentials (its own and the rescalings exp2(m - m') of the
    running sum), EXP_REL each, whose arguments are differences of running maxima that telescope to M - a_k, each rounded once: u (M -
    a_k) in all, weighted by the term's share of the sum; n_round fp32 roundings of the positive sum; v_log_f32 LOG_REL of max(1,
    |log2 S|); M + log2 S rounds; ln2_product: the product with the fp32 constant ln 2 rounds and the constant is rounded."""
    a, ae = scaled_logits(z, ze, inv_temp, center, dev)
    A = a.abs().max(1, keepdim=True).values
    M = a.max(1, keepdim=True).values
    x = M - a
    ex = torch.exp(-x)
    S = ex.sum(1, keepdim=True)
    L = M + torch.log(S)
    srel = U * (ex * x).sum(1, keepdim=True) / S + n_exp * EXP_REL + n_round * U
    c = (inv_temp * ze).expand_as(a)
    cmax = c.max(1, keepdim=True).values
    Lr = (ae - c).max(1, keepdim=True).values + 1.01 * srel + LOG_REL * torch.log(S).clamp_min(LN2) + U * L.abs()
    if ln2_product:
        Lr = Lr + 2 * U * L.abs()
    return (L, Lr + cmax, A, Lr + 2 * cmax * cmax) if parts else (L, Lr + cmax, A)


def _exp_minus(a, ae, L, Le):
    """exp(a - L) as the kernels form it (v_exp_f32 of a rounded difference, arguments off by ae and Le): (value, bound).  v_exp_f32
    flushes a denormal result: where the kernel's value can fall below TINY it may be 0, off by the value itself (<= TINY)."""
    arg = a - L
    v = torch.exp(arg)
    e = v * (torch.expm1(ae + Le + 2 * U * arg.abs()) + EXP_REL)
    return v, e + torch.where(v - e < TINY, v, torch.zeros_like(v))


def dino_loss(s, se, t, te, center, ncrops, B, temps, coef, grad16, dev=False, fused=False):
    """lafs_dino_loss_fwd_bwd (fused: lafs_dino_head_loss) on student logits s [ncrops B, K] and teacher logits t [2 B, K] known to
    within se, te (0 for the unfused kernel, whose logits are operands; `gemm`'s bound for the fused one), centre [K], temps = the
    fp32 (tau_s, tau_t) in force, coef = `dino_coef`.  Returns {"q" [2 B, K], "p", "grad" [ncrops B, K] (through `flip` where
    grad16), "dots" [ncrops B, 1] = <sum_{i != v} q_i, s / tau_s>, "loss", "lse_s", "lse_t"} as (reference, bound) and "A" [ncrops B, 1],
    the row's largest |logit / tau| over the student row and its two teacher rows.
    p, q: `_exp_minus` -- the argument's error grows with |a| and |lse| and multiplies the value.  A logit's own error (se, te) is
    common to the argument and to the log-sum-exp it is subtracted from, and is carried as such (`centred` below, and `common` for the
    loss); every rounding of the kernels' own arithmetic is counted independently on both sides.
    grad: coef (n_v p - sum q): the errors of both sides add (the cancellation is carried, not divided out); the sum q_0 + q_1, the
    difference and the product with coef round; with device temperatures coef carries a device division.
    dots, loss: sums of any order over terms that carry the errors above; depth = the longest chain of fp32 additions a term can
    pass through in either kernel (written out below)."""
    K = s.shape[1]
    its, itt = inv32(temps[0]), inv32(temps[1])
    if fused:
        nblk = -(-K // 64)
        trips = -(-nblk // 64)
        # row_part: 16 values in sequence + 2 shuffles; row_lse: `trips` in sequence + 6 butterfly steps, one rescaling each
        ne, nr = 1 + trips + 6, 18 + 2 * (trips + 6)
    else:
        trips = -(-K // 4096) + 1
        # row_stats: 16 values per trip, then the butterfly (6) and the four waves (4), one rescaling each
        ne, nr = 1 + trips + 10, 16 + 2 * (trips + 10)
    Ls, Lse, As, Lsr = lse_rows(s, se, its, None, ne, nr, dev, not fused, parts=True)
    Lt, Lte, At, Ltr = lse_rows(t, te, itt, center, ne, nr, dev, not fused, parts=True)
    a_s, ase = scaled_logits(s, se, its, None, dev)
    a_t, ate = scaled_logits(t, te, itt, center, dev)

    def centred(a, ae, ze, it, L):
        """The argument error of exp(a_k - lse) with the logits' own error eta (|eta_j| <= c_j = ze_j / tau) taken as what it is in
        the fused kernel: the same in both passes (they form a logit with the same MFMA sequence, bit for bit), hence common to a_k
        and to the log-sum-exp, which moves by sum_j w_j eta_j (w = the softmax; second order in `lse_rows`).  What is left of it in
        a_k - lse is eta_k - sum_j w_j eta_j, at most (1 - w_k) c_k + sum_{j != k} w_j c_j -- 0 for a single class, ~2 c for a
        flat row.  Every other part of ae (the roundings of the kernel's own arithmetic) stays as it is."""
        c = (it * ze).expand_as(a)
        w = torch.exp(a - L)
        return ae + (w * c).sum(1, keepdim=True) - 2 * w * c

    p, pe = _exp_minus(a_s, centred(a_s, ase, se, its, Ls), Ls, Lsr)
    q, qe = _exp_minus(a_t, centred(a_t, ate, te, itt, Lt), Lt, Ltr)
    q0, q1, q0e, q1e = q[:B], q[B:], qe[:B], qe[B:]
    v = torch.arange(ncrops * B, device=s.device) // B
    sel0, sel1 = (v != 0).double()[:, None], (v != 1).double()[:, None]           # crop v meets q_i for i != v
    rep = lambda x: x.repeat(ncrops, 1)
    qs = sel0 * rep(q0) + sel1 * rep(q1)
    qse = sel0 * rep(q0e) + sel1 * rep(q1e) + U * qs
    nv = sel0 + sel1
    diff = nv * p - qs
    g = coef * diff
    ge = coef * (nv * pe + qse + U * diff.abs()) + (U + (ULP1 if dev else 0)) * g.abs()
    ge = ge + torch.where(g.abs() - ge < TINY, g.abs(), torch.zeros_like(g))       # (a denormal product may be flushed as well)
    out = {"q": (q, qe), "p": (p, pe), "lse_s": (Ls, Lse), "lse_t": (Lt, Lte), "grad": flip(g, ge) if grad16 else (g, ge)}
    At2 = torch.maximum(At[:B], At[B:])
    out["A"] = torch.maximum(As, rep(At2))
    term = qs * a_s
    dots, dabs = term.sum(1, keepdim=True), term.abs().sum(1, keepdim=True)
    terme = (qse * a_s.abs() + qs * ase + U * term.abs()).sum(1, keepdim=True)
    rows_s = ncrops * B
    if fused:
        # a thread's 32 values per 32-row tile over <= ceil(rows_s / 128) tiles, the wave (6) and the four waves (2); the finalize
        # kernel: a thread's rows and blocks in sequence, then 256 partial sums in sequence
        d_dot = 32 * -(-rows_s // 128) + 8
        d_fin = -(-rows_s // 256) + -(-nblk // 256) + min(256, max(rows_s, nblk))          # (the other partial sums are exact zeros)
    else:
        # a thread's 4 values, the wave (6), the four waves (3), the 1024-class chunks in sequence; the finalize kernel: a thread's
        # <= 2 rows, the wave (6), 16 waves in sequence
        d_dot = 4 + 6 + 3 + -(-K // 1024)
        d_fin = 2 + 6 + 16
    out["dots"] = (dots, terme + d_dot * U * dabs)
    N = (2 * ncrops - 2) * B
    loss = (nv * Ls - dots).sum() / N
    lmag = (nv * Ls.abs() + dabs).sum()
    # A student logit's own error eta_j is common to n_v lse (which it moves by n_v p_j eta_j) and to the dot (by sum q_j eta_j): to
    # first order the loss moves by the gradient, (n_v p_j - sum q_j) eta_j; the second order is in `lse_rows`' part without it.
    c_s = (its * se).expand_as(a_s)
    common = (diff.abs() * c_s).sum()
    terme_r = (qse * a_s.abs() + qs * (ase - c_s) + U * term.abs()).sum()
    le = ((nv * Lsr).sum() + terme_r + common + (d_dot + d_fin + 2) * U * lmag) / N + ULP1 * loss.abs()
    if fused:
        le = le + 2 * U * (nv * Ls.abs()).sum() / N              # the product with the fp32 constant ln 2, here in the finalize kernel
    out["loss"] = (loss.reshape(1), le.reshape(1))
    return out


def center_ema(center, colsum, inv_rows, m):
    """lafs_center_ema: center m + colsum inv_rows (1 - m) on the fp32 values of inv_rows and m (1.0f - m is exact for m in [0.5, 1]):
    two products on the right, one on the left, one sum."""
    ir, mm = f32c(inv_rows), f32c(m)
    new = colsum * ir * (f32c(1.0) - mm)
    ref = center * mm + new
    return ref, U * ((center * mm).abs() + 2 * new.abs() + ref.abs())


# ------------------------------------------------------------------------------------------------ the landmark CNN (landmark_cnn.hip,
# landmark_train.hip): activation derivatives, depthwise convolutions, column means
def act_grad(z, ze, kind):
    """act_grad_f of landmark_train.hip on a pre-activation z the kernel holds to within ze: (derivative, bound, knife).  relu': z > 0;
    h-swish': 0 for z <= -3, 1 for z >= 3, (2 z + 3) (1 / 6) between (2 z exact, the sum rounds, the product with the rounded constant
    rounds twice); h-sigmoid': 1 / 6 for -3 < z < 3 (the rounded constant: u / 6), else 0.  The derivatives jump at the kinks -- relu'
    by 1 at 0, h-swish' by 0.5 at -3 (0 -> -0.5) and at 3 (1.5 -> 1), h-sigmoid' by 1 / 6 at +-3: an element whose z lies within ze
    of a kink (`knife`) may take either branch, and its bound admits both.  With ze = 0 nothing is on a knife edge and the side is
    the source's."""
    zero = torch.zeros_like(z)
    if kind == ACT_NONE:
        return torch.ones_like(z), zero, torch.zeros_like(z, dtype=torch.bool)
    if kind == ACT_RELU:
        knife = z.abs() < ze
        return (z > 0).double(), knife.double(), knife
    knife = ((z + 3).abs() < ze) | ((z - 3).abs() < ze)
    if kind == ACT_HSWISH:
        mid = (z > -3) & (z < 3)
        d = torch.where(mid, (2 * z + 3) / 6, (z >= 3).double())
        e = torch.where(mid, ze / 3 + U * ((2 * z + 3).abs() / 6 + 2 * d.abs()), zero)
        return d, e + 0.5 * knife.double(), knife
    if kind == ACT_HSIGMOID:
        mid = (z > -3) & (z < 3)
        return mid.double() / 6, torch.where(mid, zero + U / 6, zero) + knife.double() / 6, knife
    raise ValueError(kind)


def _dw_geom(H, W, k, stride):
    return (H + stride - 1) // stride, (W + stride - 1) // stride, (k - 1) // 2


def dwconv(x, w, k, stride):
    """Depthwise k x k convolution, stride 1 or 2, pad (k - 1) / 2, of NHWC x [N, H, W, C] with tap-major weights w [k k, C]: (value,
    sum |terms|) [N, ceil(H / stride), ceil(W / stride), C] -- nn.Conv2d(C, C, k, stride, (k - 1) // 2, groups=C) without its bias."""
    N, H, W, C = x.shape
    Ho, Wo, P = _dw_geom(H, W, k, stride)
    xp = torch.zeros(N, H + 2 * P, W + 2 * P, C, dtype=x.dtype, device=x.device)
    xp[:, P:P + H, P:P + W] = x
    v = torch.zeros(N, Ho, Wo, C, dtype=x.dtype, device=x.device)
    s = torch.zeros_like(v)
    for ky in range(k):
        for kx in range(k):
            t = xp[:, ky:ky + stride * (Ho - 1) + 1:stride, kx:kx + stride * (Wo - 1) + 1:stride] * w[ky * k + kx]
            v, s = v + t, s + t.abs()
    return v, s


def dwconv_bwd(x, dy, w, k, stride):
    """Both gradients of `dwconv`: (dx, sum |terms of dx|) [N, H, W, C] and (dw, sum |terms of dw|) [k k, C]."""
    N, H, W, C = x.shape
    Ho, Wo, P = _dw_geom(H, W, k, stride)
    xp = torch.zeros(N, H + 2 * P, W + 2 * P, C, dtype=x.dtype, device=x.device)
    xp[:, P:P + H, P:P + W] = x
    dxp, sxp = torch.zeros_like(xp), torch.zeros_like(xp)
    dw, sw = torch.zeros_like(w), torch.zeros_like(w)
    for ky in range(k):
        for kx in range(k):
            sl = (slice(None), slice(ky, ky + stride * (Ho - 1) + 1, stride), slice(kx, kx + stride * (Wo - 1) + 1, stride))
            t = dy * w[ky * k + kx]
            dxp[sl] += t
            sxp[sl] += t.abs()
            u = dy * xp[sl]
            dw[ky * k + kx] = u.sum((0, 1, 2))
            sw[ky * k + kx] = u.abs().sum((0, 1, 2))
    crop = (slice(None), slice(P, P + H), slice(P, P + W))
    return (dxp[crop], sxp[crop]), (dw, sw)


def tree_depth(n, lanes):
    """Most fp32 additions a term passes through when `lanes` threads each add their share of n terms in sequence and a binary tree
    over the lanes follows: a sum of any sign is then off by at most depth u sum|terms|."""
    return -(-n // lanes) + max(1, math.ceil(math.log2(lanes)))


def col_mean(x, depth, r16):
    """mean over dim 1 of x [N, HW, C] as the pooling kernels form it: a sum of the given depth, then the product with the rounded
    fp32 reciprocal 1.0f / HW (2 u), stored to 16 bits."""
    HW = x.shape[1]
    m = x.mean(1)
    return flip(m, depth * U * x.abs().sum(1) / HW + 2 * U * m.abs(), r16)


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
