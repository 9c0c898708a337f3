"""The fp64 oracle of the AdaFace head (lafs_adaface_margins, lafs_margin_softmax_ce_ada_bf16, the AdaFace module and margin_type 2 of
FinetuneEngine), its per-element bounds, the case lists and the guarded buffers.  Shared by tests/test_oracle_adaface_host.py (CPU:
the oracle against an independent restatement, seeded faults, the caps), tests/test_gpu_adaface.py and tests/test_gpu_adaface_dp.py.

Specification (Kim, Jain, Liu, CVPR 2022, restated; include/lafs_hip.h):
  n_b = clip(1 / inv_norm[b], 1e-3, 100);  mean, unbiased two-pass std over the batch;  update: state <- t (mean, std) + (1 - t) state FIRST;
  k_b = clip((n_b - batch_mean) / (batch_std + eps) h, -1, 1);  g_ang = -m k_b;  g_add = m + m k_b     (detached)
  c^ = clamp(c, -1 + eps, 1 - eps);  target classes (weight > 0): z = s (cos(clip(acos c^ + g_ang, eps, pi - eps)) - g_add);  else z = s c^
  loss_b = lse(z) - sum_k y_k z_k;  dL/dc_k = loss_scale / B (softmax_k - y_k) dz_k/dc_k, dz/dc = 0 where clamped or clipped.
Every threshold is the fp32 constant the kernel compares with, widened: both sides take the same branch.

Bounds follow the kernels' fp32 arithmetic (csrc/finetune.hip), one rounding = U = 2^-24 relative:
  `/`, sqrtf 1 ulp (fp64_bounds.ULP1);  acosf, cosf, sinf (the full-precision device library on the <= 2 targets per row) 2 ulp = TRIG_REL,
  twice the 1 ulp of HIP's published math-API table;  __expf = v_exp_f32(fl(log2(e) x)) and __logf: fp64_bounds.EXP_REL / LOG_REL.
  v_exp_f32 returns 0 for a result below 2^-126 (it has no denormal results: fp64_bounds, `_exp_minus`): the oracle flushes where the
  kernel must, so a far-off class has reference 0 and bound 0; only where the argument's error straddles the threshold is either accepted."""
import math

import torch

import fp64_bounds as fb

f32, f64, bf16 = torch.float32, torch.float64, torch.bfloat16
U, ULP1, TINY = fb.U, fb.ULP1, fb.TINY
TRIG_REL = 4 * U
NCH = 16                                            # MCE_NCH of csrc/finetune.hip

_t = lambda v: torch.tensor(v, dtype=f32)
EPS = float(_t(1e-3))
LO, HI = float(_t(-1.0) + _t(1e-3)), float(_t(1.0) - _t(1e-3))
PI_HI = float(_t(math.pi) - _t(1e-3))
NORM_LO, NORM_HI = EPS, 100.0
S, M, H, T_ALPHA = 64.0, fb.f32c(0.4), fb.f32c(0.333), fb.f32c(0.01)
STATE0 = (20.0, 100.0)

MCE_SHAPES = [(8, 50), (8, 1000), (32, 20533)]      # the project's own smallest shapes (tests/test_gpu_finetune.py)


# ------------------------------------------------------------------------------------------------ norm statistics and margins
def _clip_iv(v, e, lo, hi):
    """clip(v, lo, hi) of a value known to within e: the clipped value and the widest distance to what the interval's ends give (0
    where the whole interval lies outside)."""
    c = v.clamp(lo, hi)
    return c, torch.maximum((v + e).clamp(lo, hi) - c, c - (v - e).clamp(lo, hi))


def _sqrt_iv(v, e):
    r = v.clamp_min(0).sqrt()
    return r, torch.maximum((v + e).clamp_min(0).sqrt() - r, r - (v - e).clamp_min(0).sqrt()) + ULP1 * r


def margins_ref(inv_norm, state, t_alpha=T_ALPHA, h=H, m=M, update=True):
    """lafs_adaface_margins on fp32 inv_norm [B] and the fp32 state (mean, std): {"state": (new state [2], bound), "rm": (row_margin
    [B, 2], bound), "k": k_b, "stats": (mean, std) of the batch}.  Sums: a thread adds ceil(B / 256) values in sequence, a 6-step
    butterfly and two additions of wave sums follow (depth d); the mean's error enters the second pass squared plus first order through
    every term."""
    x = inv_norm.double()
    B = x.numel()
    d = -(-B // 256) + 8
    n, ne = _clip_iv(1 / x, ULP1 / x, NORM_LO, NORM_HI)
    mean = n.mean()
    me = ne.mean() + d * U * n.abs().mean() + ULP1 * mean.abs()
    c = n - mean
    ce = ne + me + U * c.abs()
    ss = (c * c).sum()
    sse = (2 * c.abs() * ce + ce * ce).sum() + (d + 1) * U * ((c.abs() + ce) ** 2).sum()
    var, vare = ss / (B - 1), sse / (B - 1) + ULP1 * ss / (B - 1)
    std, stde = _sqrt_iv(var, vare)
    bm, bs = torch.tensor(float(state[0]), dtype=f64), torch.tensor(float(state[1]), dtype=f64)
    bme = bse = torch.zeros((), dtype=f64)
    bm_use, bs_use = bm, bs
    if update:
        one_t = float(_t(1.0) - _t(t_alpha))
        bm_n, bs_n = t_alpha * mean + one_t * bm, t_alpha * std + one_t * bs
        bme = t_alpha * me + U * ((t_alpha * mean).abs() + (one_t * bm).abs() + bm_n.abs())
        bse = t_alpha * stde + U * ((t_alpha * std).abs() + (one_t * bs).abs() + bs_n.abs())
        bm, bs = bm_use, bs_use = bm_n, bs_n
    num, nume = n - bm_use, ne + bme + U * (n - bm_use).abs()
    dn = bs_use + EPS
    dne = bse + U * dn
    q = num / dn * h
    qe = ((num.abs() + nume) / (dn - dne) - num.abs() / dn) * h + (ULP1 + U) * q.abs()
    k, ke = _clip_iv(q, qe, -1.0, 1.0)
    mk = m * k
    g_ang, g_add = -mk, m + mk
    rm = torch.stack([g_ang, g_add], 1)
    rme = torch.stack([m * ke + U * mk.abs(), m * ke + 2 * U * mk.abs() + U * g_add.abs()], 1)
    return {"state": (torch.stack([bm, bs]), torch.stack([bme, bse]) if update else torch.zeros(2, dtype=f64)), "rm": (rm, rme), "k": k,
            "stats": (mean, std)}


def stats_cases():
    """(name, inv_norm f32 [B], state, t_alpha, update) of the statistics kernel: B in {2, 8, 64, 200, 1024} x norms N(20, 5) / all equal
    (std 0, t_alpha 1) / outside both clips / a spread that drives k to -1 and +1 (from the arbitrary state, whose std is small), from
    the initial state and an arbitrary one."""
    out = []
    for B in (2, 8, 64, 200, 1024):
        g = torch.Generator().manual_seed(1000 + B)
        normal = (20 + 5 * torch.randn(B, generator=g)).clamp_min(0.5)
        equal = torch.full((B,), 17.25)
        outside = torch.where(torch.arange(B) % 2 == 0, torch.tensor(1e-4), torch.tensor(1e3))
        spread = torch.where(torch.arange(B) % 2 == 0, torch.tensor(2.0), torch.tensor(60.0)) + torch.rand(B, generator=g)
        for name, norms, t in (("normal", normal, T_ALPHA), ("equal", equal, 1.0), ("outside", outside, T_ALPHA), ("spread", spread, T_ALPHA)):
            for state in (STATE0, (fb.f32c(23.7), fb.f32c(4.1))):
                for update in (True, False):
                    out.append((f"{name} B={B} state={state[0]:.1f},{state[1]:.1f} update={int(update)}", (1 / norms).to(f32), state, t, update))
    return out


# ------------------------------------------------------------------------------------------------ the loss
def sparse_target(y1, y2, lam, B, C):
    """(columns [B, 2], weights [B, 2]) of y = lam e_y1 + (1 - lam) e_y2; equal classes: the summed weight on the first, 0 on the second."""
    y1, y2, lam = y1.long(), y2.long(), lam.double()
    same = y1 == y2
    w1 = torch.where(same, torch.ones_like(lam), lam)
    w2 = torch.where(same, torch.zeros_like(lam), 1 - lam)
    return torch.stack([y1, y2], 1), torch.stack([w1, w2], 1)


def lse_terms(C):
    """(n_exp, n_round) of fp64_bounds.lse_rows for the (row, chunk) kernels: a thread folds t = ceil(chunk / 256) logits online (a
    rescaling exponential each), the butterfly (6), the four waves (1) and the NCH chunk partials (1) follow; additions: t + 2 per
    merge level."""
    t = -(-((-(-C // NCH) + 3) // 4 * 4) // 256)
    return t + 9, t + 2 * 6 + 4 + NCH


def loss_ref(cos, y1, y2, lam, rm, s=S, loss_scale=1.0):
    """lafs_margin_softmax_ce_ada_bf16 on fp32 operands (cos [B, C], lam [B], rm [B, 2] = (g_ang, g_add)), in the sparse (y1, y2, lam)
    form: {"rows": (row losses, bound), "loss": (mean, bound), "grad": (fp64 gradient, its pre-rounding fp32 error bound),
    "grad16": fp64_bounds.flip of the two (the bf16 store), "zero": elements that must be exactly 0 (clamped or clipped),
    "clip_dist": per target its distance to the nearer clip bound (rad), "clamp_dist": every cosine's distance to the nearer clamp
    threshold}."""
    c = cos.double()
    B, C = c.shape
    cols, w = sparse_target(y1, y2, lam, B, C)
    g_ang, g_add = rm[:, :1].double(), rm[:, 1:].double()
    cc = c.clamp(LO, HI)
    clamped = (c < LO) | (c > HI)
    z = s * cc
    ze = U * z.abs()
    dz = torch.where(clamped, torch.zeros_like(c), torch.full_like(c, s))
    dze = torch.zeros_like(c)
    y = torch.zeros_like(c)
    rows_idx = torch.arange(B)
    clip_dist = torch.full((B, 2), float("inf"), dtype=f64)
    for j in (1, 0):                                         # (column 0 last: on equal classes its summed weight wins)
        k, wj = cols[:, j], w[:, j]
        on = wj > 0
        cj = cc[rows_idx, k]
        th = torch.acos(cj)
        the = TRIG_REL * th
        tm = th + g_ang[:, 0]
        tme = the + U * tm.abs()
        clipped = (tm < EPS) | (tm > PI_HI)
        tmc = tm.clamp(EPS, PI_HI)
        tmce = torch.where(clipped, torch.zeros_like(tme), tme)
        co = torch.cos(tmc)
        coe = torch.sin(tmc).abs() * tmce + TRIG_REL * co.abs()
        df = co - g_add[:, 0]
        zj = s * df
        zje = s * (coe + U * df.abs()) + U * zj.abs()
        sn, sd = torch.sin(tm), torch.sin(th)
        sne, sde = torch.cos(tm).abs() * tme + TRIG_REL * sn.abs(), torch.cos(th).abs() * the + TRIG_REL * sd.abs()
        dj = s * sn / sd
        dje = s * ((sn.abs() + sne) / (sd - sde) - sn.abs() / sd) + (ULP1 + U) * dj.abs()
        dead = clipped | clamped[rows_idx, k]
        dj, dje = torch.where(dead, torch.zeros_like(dj), dj), torch.where(dead, torch.zeros_like(dje), dje)
        r = rows_idx[on]
        z[r, k[on]], ze[r, k[on]], dz[r, k[on]], dze[r, k[on]], y[r, k[on]] = zj[on], zje[on], dj[on], dje[on], wj[on]
        clip_dist[on, j] = torch.minimum((tm - EPS).abs(), (tm - PI_HI).abs())[on]
    n_exp, n_round = lse_terms(C)
    L, Le, _ = fb.lse_rows(z, ze, 1.0, None, n_exp, n_round, False, True)
    # row loss: lse - the spikes (one product and one addition each), one subtraction
    dot = (y * z).sum(1, keepdim=True)
    dote = (y * ze + 2 * U * (y * z).abs()).sum(1, keepdim=True)
    rows = L - dot
    rowse = Le + dote + U * rows.abs()
    loss = rows.mean()
    losse = rowse.mean() + (-(-B // 256) + 8) * U * rows.abs().mean() + U * loss.abs()
    # gradient: exp(z - lse) with the kernel's flush below 2^-126; (p - y) rounds; gs * (.) * dz: two products
    arg = z - L
    arge = ze + Le + 2 * U * arg.abs()
    p = torch.exp(arg)
    pe = p * (torch.expm1(arge) + fb.EXP_REL)
    y2e = arg * fb.LOG2E                                     # the argument of v_exp_f32
    slack = arge * fb.LOG2E + 2 * U * y2e.abs()
    gone, knife = y2e + slack < -126, ((y2e - slack) < -126) & ~(y2e + slack < -126)
    p, pe = torch.where(gone, torch.zeros_like(p), p), torch.where(gone, torch.zeros_like(pe), torch.where(knife, pe + p, pe))
    diff = p - y
    diffe = pe + U * diff.abs() + U * y                      # (the kernel's weights lam, fl(1 - lam) and their fp32 sum on equal classes)
    gs = float(_t(loss_scale) / _t(float(B)))
    g = gs * diff * dz
    ge = gs * (diffe * dz.abs() + (diff.abs() + diffe) * dze) + 2 * U * g.abs()
    ge = ge + torch.where((g != 0) & (g.abs() - ge < TINY), g.abs(), torch.zeros_like(g))      # (a denormal product may be flushed)
    zero = dz == 0
    ge = torch.where(zero, torch.zeros_like(ge), ge)
    return {"rows": (rows[:, 0], rowse[:, 0]), "loss": (loss.reshape(1), losse.reshape(1)), "grad": (g, ge), "grad16": fb.flip(g, ge),
            "zero": zero, "clip_dist": clip_dist, "clamp_dist": torch.minimum((c - LO).abs(), (c - HI).abs()), "z": z, "lse": L}


def dense_restatement(cos, y1, y2, lam, rm, s=S, loss_scale=1.0):
    """The published forward in its dense one-hot, scatter formulation, by float64 autograd: independent of `loss_ref`'s sparse
    bookkeeping and of its hand-written derivative.  Returns (row losses, mean loss, gradient of loss_scale x mean loss)."""
    c = cos.double().clone().requires_grad_(True)
    B, C = c.shape
    t = torch.zeros(B, C, dtype=f64)
    t.scatter_add_(1, y1.long().view(-1, 1), lam.double().view(-1, 1))
    t.scatter_add_(1, y2.long().view(-1, 1), (1 - lam.double()).view(-1, 1))
    cc = c.clamp(LO, HI)
    theta_m = (torch.acos(cc) + rm[:, :1].double()).clamp(EPS, PI_HI)
    z = s * torch.where(t > 0, torch.cos(theta_m) - rm[:, 1:].double(), cc)
    rows = torch.logsumexp(z, -1) - (t * z).sum(-1)
    (loss_scale * rows.mean()).backward()
    return rows.detach(), rows.mean().detach(), c.grad


def loss_case(B, C, lam_value, explicit_y2=False, seed=0):
    """One case of the loss kernel at an MCE shape: uniform cosines with the planted values the specification's branches need, one row
    with y1 == y2, rows with k = -1, 0, +1, and the fp32 operands the kernel gets.  Rows (partner of row b: B-1-b, or a permutation
    when explicit_y2):
      row 0: k = +1 (g_ang = -m, g_add = 2m), target cosine 0.9985: theta_m clipped at eps
      row 1: k = -1 (g_ang = +m, g_add = 0), target cosine -0.9985: theta_m clipped at pi - eps
      row 2: y1 == y2;  rows 3, 4: k = 0 and k = +1 with ordinary targets;  the rest: k uniform in [-1, 1]
      non-target cosines +-0.9995 and +-1.0 planted in rows 0..3 (clamped: z = s (+-(1 - eps)), gradient exactly 0)."""
    g = torch.Generator().manual_seed(7919 * C + 31 * B + seed)
    Cpad = (C + 127) // 128 * 128
    cos = torch.rand(B, Cpad, generator=g) * 2 - 1
    cos[:, C:] = 0
    y1 = torch.randint(0, C, (B,), generator=g)
    y1[2] = y1[B - 3]
    y2 = y1.flip(0)
    if explicit_y2:
        y2 = y1[torch.randperm(B, generator=g)]
        y2[2] = y1[2]
    k = torch.rand(B, generator=g) * 2 - 1
    k[0], k[1], k[3], k[4] = 1.0, -1.0, 0.0, 1.0
    mk = (_t(M) * k.to(f32))
    rm = torch.stack([-mk, _t(M) + mk], 1).to(f32)
    lam = torch.full((B,), lam_value, dtype=f32)
    taken = lambda b: {int(y1[b]), int(y2[b])}
    for b, vals in ((0, (0.9995, -1.0)), (1, (-0.9995, 1.0)), (2, (0.9995, -0.9995)), (3, (1.0, -1.0))):
        free = [j for j in range(C) if j not in taken(b)]
        for i, v in enumerate(vals):
            cos[b, free[3 + 5 * i]] = v
    # ordinary targets stay away from the clamp and, with their row's margin, from the clip bounds
    for b in range(B):
        for col in taken(b):
            cos[b, col] = cos[b, col].clamp(-0.95, 0.95)
    cos[0, y1[0]] = 0.9985
    cos[1, y1[1]] = -0.9985
    if lam_value < 1.0:                                      # the partner spikes of the two clipped rows: ordinary values
        for b in (0, 1):
            if int(y2[b]) != int(y1[b]):
                cos[b, y2[b]] = 0.3 if b == 0 else -0.3
    return {"cos": cos, "Cpad": Cpad, "y1": y1, "y2": y2, "lam": lam, "rm": rm, "k": k}


def check_conditions(case, ref, C):
    """The conditions the gates are stated under, asserted on the CPU inputs: apart from the two planted clipped targets no target
    lies within 1e-4 rad of a clip bound, and no cosine within 1e-6 of a clamp threshold."""
    assert float(ref["clip_dist"].min()) > 1e-4, float(ref["clip_dist"].min())      # (the two planted targets lie 0.3 rad BEYOND their bound)
    assert float(ref["clamp_dist"][:, :C].min()) > 1e-6, float(ref["clamp_dist"][:, :C].min())
    assert bool(ref["zero"][0, case["y1"][0]]) and bool(ref["zero"][1, case["y1"][1]]), "the planted targets must be clipped"


def judge_margins(tag, state, rm, ref):
    """lafs_adaface_margins' outputs inside their bounds, element by element; returns the worst error / bound."""
    r1, _ = fb.check(f"{tag} state", state.double().cpu(), *ref["state"])
    r2, _ = fb.check(f"{tag} row_margin", rm.double().cpu(), *ref["rm"])
    assert bool(torch.isfinite(rm).all())
    return max(r1, r2)


def judge_loss(tag, loss, rows, grad16, ref, C):
    """The gates of the loss kernel: mean loss and every row loss within 1e-5 relative (the project's own for the bf16 entries); the
    bf16 gradient element by element inside fp64_bounds.flip of the fp32 error bound; exactly 0 at every clamped or clipped element and
    in the pad columns; cap: the bound is 0 (an exact bf16 match) at no fewer than 95 % of the elements.  Returns (worst error / bound,
    share of elements with bound 0)."""
    ref_loss, ref_rows = ref["loss"][0], ref["rows"][0]
    e_loss = abs(float(loss) - float(ref_loss)) / abs(float(ref_loss))
    e_rows = float(((rows.double().cpu() - ref_rows).abs() / ref_rows.abs()).max())
    print(f"{tag}: loss {float(loss):.6f} vs {float(ref_loss):.6f}: rel {e_loss:.2e}; worst row {e_rows:.2e}")
    assert e_loss < 1e-5, e_loss
    assert e_rows < 1e-5, e_rows
    g = grad16.float().double().cpu()
    ratio, exact = fb.check(f"{tag} gradient", g[:, :C], *ref["grad16"], is16=True)
    assert bool((g[:, :C][ref["zero"]] == 0).all()), "a clamped or clipped element has a non-zero gradient"
    assert float(g[:, C:].abs().max() if g.shape[1] > C else 0.0) == 0.0, "pad columns must be zero"
    assert exact >= 0.95, f"bound 0 at only {100 * exact:.1f} % of the elements"
    return ratio, exact


# ------------------------------------------------------------------------------------------------ fp32 emulation with seeded faults
def emulate_margins(inv_norm, state, t_alpha, h, m, update, fault=None):
    """lafs_adaface_margins in fp32 torch arithmetic (any summation order).  fault: None, 'biased_std', 'stale_state', 'g_ang_sign'."""
    n = (1 / inv_norm.to(f32)).clamp(NORM_LO, NORM_HI)
    mean = n.mean()
    std = ((n - mean) ** 2).sum().div(n.numel() if fault == "biased_std" else n.numel() - 1).sqrt()
    bm, bs = _t(state[0]), _t(state[1])
    bm_new, bs_new = (_t(t_alpha) * mean + (1 - _t(t_alpha)) * bm, _t(t_alpha) * std + (1 - _t(t_alpha)) * bs) if update else (bm, bs)
    um, us = (bm, bs) if fault == "stale_state" else (bm_new, bs_new)
    k = ((n - um) / (us + _t(1e-3)) * _t(h)).clamp(-1, 1)
    mk = _t(m) * k
    return torch.stack([bm_new, bs_new]), torch.stack([mk if fault == "g_ang_sign" else -mk, _t(m) + mk], 1)


def emulate_loss(cos, y1, y2, lam, rm, s=S, loss_scale=1.0, fault=None):
    """The loss kernel in fp32 torch arithmetic, bf16 gradient out.  fault: None, 'no_clamp', 'grad_at_clamp', 'margin_times_y',
    'no_theta_clip'."""
    c = cos.to(f32)
    B, C = c.shape
    t = torch.zeros(B, C, dtype=f32)
    t.scatter_add_(1, y1.long().view(-1, 1), lam.to(f32).view(-1, 1))
    t.scatter_add_(1, y2.long().view(-1, 1), (1 - lam.to(f32)).view(-1, 1))
    tgt = t > 0
    lo, hi = (-1.0, 1.0) if fault == "no_clamp" else (LO, HI)
    cc = c.clamp(lo, hi)
    live = torch.ones_like(tgt) if fault == "grad_at_clamp" else (c >= lo) & (c <= hi)
    g_ang, g_add = rm[:, :1].to(f32), rm[:, 1:].to(f32)
    if fault == "margin_times_y":
        g_ang, g_add = g_ang * t, g_add * t
    th = torch.acos(cc)
    tm = th + g_ang
    e, ph = (-1e30, 1e30) if fault == "no_theta_clip" else (EPS, PI_HI)
    z = _t(s) * torch.where(tgt, torch.cos(tm.clamp(e, ph)) - g_add, cc)
    dz = _t(s) * torch.where(tgt, torch.where((tm >= e) & (tm <= ph), torch.sin(tm) / torch.sin(th).clamp_min(1e-30), torch.zeros_like(c)),
                             torch.ones_like(c)) * live
    L = torch.logsumexp(z, -1, keepdim=True)
    rows = (L - (t * z).sum(-1, keepdim=True))[:, 0]
    p = torch.exp(z - L)
    p = torch.where(p < TINY, torch.zeros_like(p), p)        # v_exp_f32 has no denormal results
    grad = (_t(loss_scale) / _t(float(B))) * (p - t) * dz
    return rows.mean(), rows, grad.to(bf16)


# ------------------------------------------------------------------------------------------------ the whole head, for module and engine
def head_ref(x, weight, y1, y2, lam, state, t_alpha, h=H, m=M, s=S, update=True, attach_k=False):
    """The head on fp64 embeddings x [B, D] (requires_grad for gradients): L2 normalisations, statistics -> state -> margins (detached;
    attach_k: the 'gradient through k_b' fault), logits, row losses.  Returns (logits, mean loss, new state (mean, std))."""
    n = x.norm(dim=1).clamp_min(1e-12)
    nc = n.clamp(NORM_LO, NORM_HI)
    if not attach_k:
        nc = nc.detach()
    mean, std = nc.mean(), nc.std(unbiased=True)
    bm, bs = float(state[0]), float(state[1])
    if update:
        bm, bs = t_alpha * mean + (1 - t_alpha) * bm, t_alpha * std + (1 - t_alpha) * bs
    k = ((nc - bm) / (bs + EPS) * h).clamp(-1, 1)
    cos = (x / n[:, None]) @ torch.nn.functional.normalize(weight, dim=1).t()
    B, C = cos.shape
    t = torch.zeros(B, C, dtype=x.dtype)
    t.scatter_add_(1, y1.long().view(-1, 1), lam.to(x.dtype).view(-1, 1))
    t.scatter_add_(1, y2.long().view(-1, 1), (1 - lam.to(x.dtype)).view(-1, 1))
    cc = cos.clamp(LO, HI)
    tm = (torch.acos(cc) + (-m * k)[:, None]).clamp(EPS, PI_HI)
    z = s * torch.where(t > 0, torch.cos(tm) - (m + m * k)[:, None], cc)
    rows = torch.logsumexp(z, -1) - (t * z).sum(-1)
    return z, rows.mean(), (float(torch.as_tensor(bm).detach()), float(torch.as_tensor(bs).detach()))


# ------------------------------------------------------------------------------------------------ guarded buffers
GUARD = 64


class Guarded:
    """A flat device buffer of `n` elements between two runs of GUARD sentinel words; intact() demands both runs bit-identical."""

    def __init__(self, n, dtype, device, fill=0.0):
        self.buf = torch.full((n + 2 * GUARD,), 7.0, dtype=dtype, device=device)
        self.v = self.buf[GUARD:GUARD + n]
        self.v.fill_(fill)
        self.n = n

    def intact(self, name):
        g = torch.cat([self.buf[:GUARD], self.buf[GUARD + self.n:]]).float()
        assert bool((g == 7.0).all()), f"{name}: guard words were overwritten"
