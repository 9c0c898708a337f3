"""The fp64 restatement, the arena and the case grid of the SGD / LARS arena step (lafs_grad_sumsq_trust_range and
lafs_clip_momentum_ema_range), shared by tests/test_sgd_lars_host.py and tests/test_gpu_sgd_lars.py as optim_cases.py is for AdamW.

The arena is optim_cases' ragged one (the 24-element tensor, the 4100-chunk tensor that takes two trips of the segment loop and a tail,
a non-trainable tensor, a last-layer tensor, 1-D tensors, the knife-edge clip tensor) plus two decayed tensors: one whose parameters
are all zero (||p|| = 0: q = 1) and one whose gradient is all zero (q = eta / wd; with wd = 0, ||d|| = 0 and q = 1).

Rules (g^ = gsc g, gsc = grad_scale min(1, clip coefficient), as in fb.adamw_ema):
  sgd   d = g^ + wd_t p                       wd_t: WD_LOW for a SEG_LOW_DECAY tensor, WD for a SEG_DECAY one, else 0
  lars  SEG_DECAY set:   d = q (g^ + wd_t p), q = eta ||p|| / ||g^ + wd_t p|| where both norms are > 0, else 1
        SEG_DECAY clear: d = g^
  both  mu = momentum mu + d;  p -= lr mu;  then the teacher EMA and the two bf16 shadows from the new p
Bounds follow the kernels' operation order, one u per fp32 operation (a fused multiply-add rounds less, never more)."""
import torch

import fp64_bounds as fb
import optim_cases as oc
from fp64_bounds import CHUNK, SEG_DECAY, SEG_LAST_LAYER, SEG_LOW_DECAY, SEG_TRAINABLE, U, f32, f64
from gemm_cases import seed_of

HP_MOMENTUM, HP_LARS_ETA = 13, 14                       # LAFS_HP_MOMENTUM, LAFS_HP_LARS_ETA
UPDATE = {"sgd": 1, "lars": 2}                          # LAFS_UPDATE_*
ZERO_P, ZERO_G = 8, 9                                   # the two added tensors
CHUNKS = oc.CHUNKS + [2, 1]
SHORT = oc.SHORT + [100, 7]
FLAGS = oc.FLAGS + [SEG_DECAY | SEG_TRAINABLE, SEG_DECAY | SEG_TRAINABLE]
NORMS = oc.NORMS + [2.0, 0.0]
CLIP, GRAD_SCALE, KNIFE, GUARD = oc.CLIP, oc.GRAD_SCALE, oc.KNIFE, oc.GUARD
N_SEG, N_CHUNKS = len(CHUNKS), sum(CHUNKS)
HYPER = dict(oc.HYPER, momentum=0.9, eta=1e-3)


def case(rule, cid, step0, freeze, clip=CLIP, teacher=True, shadow=True, wd=None):
    return dict(id=f"{rule}-{cid}", rule=rule, step0=step0, freeze=freeze, clip=clip, teacher=teacher, shadow=shadow,
                wd=HYPER["wd"] if wd is None else wd)


def _grid(rule):
    return [case(rule, "t1-frozen-last", 0, 1), case(rule, "later", 3, 0), case(rule, "clip-disabled", 1, 0, clip=0.0),
            case(rule, "wd0", 1, 0, wd=0.0), case(rule, "no-teacher", 1, 1, teacher=False), case(rule, "no-shadow", 1, 0, shadow=False)]


CASES = _grid("sgd") + _grid("lars")


def seg_starts():
    s = [0]
    for n in CHUNKS:
        s.append(s[-1] + n)
    return s


def hyper_vec(c):
    h = torch.zeros(16, dtype=f32)
    h[fb.HP_LR], h[fb.HP_WD], h[fb.HP_WD_LOW], h[fb.HP_EMA_M] = HYPER["lr"], c["wd"], HYPER["wd_low"], HYPER["ema"]
    h[fb.HP_BETA1], h[fb.HP_BETA2], h[fb.HP_EPS] = HYPER["beta1"], HYPER["beta2"], HYPER["eps"]         # (unread by both rules)
    h[fb.HP_CLIP], h[fb.HP_FREEZE_LAST], h[fb.HP_GRAD_SCALE] = c["clip"], c["freeze"], GRAD_SCALE
    h[HP_MOMENTUM], h[HP_LARS_ETA] = HYPER["momentum"], HYPER["eta"]
    return h


def arena_inputs(c):
    """The state of case c as fp64 CPU tensors of exactly representable fp32 values, [N_CHUNKS, 1024] each, padding zero: p, g, m
    (the momentum buffer), t (teacher); chunk_seg, flags, step (int32); hyper (fp32 [16]); mask (the logical elements)."""
    gen = torch.Generator()
    gen.manual_seed(seed_of("sgd-lars-arena", c["id"]))
    rn = lambda: torch.randn(N_CHUNKS, CHUNK, generator=gen, dtype=f64)
    rf = lambda v: v.to(f32).double()
    st = seg_starts()
    chunk_seg = torch.cat([torch.full((n,), i, dtype=torch.int32) for i, n in enumerate(CHUNKS)])
    mask = torch.ones(N_CHUNKS, CHUNK, dtype=torch.bool)
    for i in range(N_SEG):
        mask[st[i + 1] - 1, CHUNK - SHORT[i]:] = False
    g = rn() * mask
    for i in range(N_SEG):
        seg = g[st[i]:st[i + 1]]
        target = (CLIP - 1e-6 if NORMS[i] is None else NORMS[i]) / GRAD_SCALE            # (None: the knife edge, as in optim_cases)
        seg *= target / seg.norm()
    p, t = 0.05 * rn(), 0.01 * rn()
    p[st[ZERO_P]:st[ZERO_P + 1]] = 0
    t = p + t
    m = 0.02 * rn() if c["step0"] else torch.zeros_like(p)
    d = {k: rf(x * mask) for k, x in (("p", p), ("g", g), ("m", m), ("t", t))}
    d.update(chunk_seg=chunk_seg, flags=torch.tensor(FLAGS, dtype=torch.int32), step=torch.full((N_SEG,), c["step0"], dtype=torch.int32),
             hyper=hyper_vec(c), mask=mask)
    return d


def trust(rule, p, g, chunk_seg, flags, n_seg, ss, sse, hp):
    """seg_trust of lafs_grad_sumsq_trust_range per tensor, (q, bound): G = sum g^2, P = sum p^2, X = sum g p through the summation tree
    of fb.sumsq (its depth without the two grad_scale products), each off by depth u times the sum of its terms' absolute values;
    ||d||^2 = gsc^2 G + 2 gsc wd X + wd^2 P: every product and sum rounds once, gsc carries the clip factor's bound; two square roots (u
    each, exact intervals), one product with eta, one division.  1 with bound 0 where SEG_DECAY is clear, where P = 0 (a sum of
    zeros is exact) and where ||d||^2 = 0 (g = 0 and wd = 0: every term is an exact zero)."""
    cs, fl = chunk_seg.long(), flags.long()
    eta, clip, gs = float(hp[HP_LARS_ETA]), float(hp[fb.HP_CLIP]), float(hp[fb.HP_GRAD_SCALE])
    fold = lambda x: torch.zeros(n_seg, dtype=f64, device=p.device).index_add_(0, cs, x.sum(1))
    G, P, X, Xa = fold(g * g), fold(p * p), fold(g * p), fold((g * p).abs())
    nc = torch.bincount(cs, minlength=n_seg).double()
    depth = 1 + 16 + 6 + torch.ceil(nc / 256) + 6 + 3
    Ge, Pe, Xe = depth * U * G, depth * U * P, depth * U * Xa
    wd = torch.full((n_seg,), float(hp[fb.HP_WD]), dtype=f64, device=p.device)
    wd[(fl & SEG_LOW_DECAY) != 0] = float(hp[fb.HP_WD_LOW])
    gsc, gsce, _ = fb.clip_scale(ss, sse, clip, gs)
    A, B, C = gsc * gsc * G, 2 * gsc * wd * X, wd * wd * P
    Ae = (2 * gsc * gsce + gsce * gsce) * (G + Ge) + gsc * gsc * Ge + 2 * U * A
    Be = 2 * wd * (gsce * (X.abs() + Xe) + gsc * Xe) + 2 * U * B.abs()
    Ce = wd * wd * Pe + 2 * U * C
    dd = A + B + C
    dde = Ae + Be + Ce + 2 * U * (A + B.abs() + C)
    sp, sd = P.sqrt(), dd.sqrt()
    spe = torch.maximum((P + Pe).sqrt() - sp, sp - (P - Pe).clamp_min(0).sqrt()) + U * sp
    sde = torch.maximum((dd + dde).sqrt() - sd, sd - (dd - dde).clamp_min(0).sqrt()) + U * sd
    num = eta * sp
    nume = eta * spe + U * num
    live = ((fl & SEG_DECAY) != 0) & (P > 0) & (dd > 0) & (rule == "lars")
    one = torch.ones_like(P)
    q = torch.where(live, num / torch.where(live, sd, one), one)
    den = torch.where(live, sd - sde, one)
    qe = torch.where(live, torch.where(den > 0, (num + nume) / den.clamp_min(1e-300) - q + U * q, torch.full_like(q, float("inf"))), torch.zeros_like(q))
    return q, qe


def step64(rule, p, g, m, t, chunk_seg, flags, step, hp, n_seg):
    """One launch pair on fp64 copies of the state ([n_chunks, 1024] each; t: the teacher, or None); hp: the hyper vector as fp64 -- the
    operands the kernel has.  Returns {"param", "mom", "teacher", "param16", "teacher16", "seg_sumsq", "seg_trust"} as (reference,
    bound), "seg_step" (exact) and "knife"."""
    lr, clip, em, frz, gs = (float(hp[i]) for i in (fb.HP_LR, fb.HP_CLIP, fb.HP_EMA_M, fb.HP_FREEZE_LAST, fb.HP_GRAD_SCALE))
    mu = float(hp[HP_MOMENTUM])
    fl, cs = flags.long(), chunk_seg.long()
    upd_s = ((fl & SEG_TRAINABLE) != 0) & ~(((fl & SEG_LAST_LAYER) != 0) & (frz != 0))
    new_step = step.long() + upd_s.long()
    col = lambda x: x[cs][:, None]
    upd = col(upd_s)
    ss, sse = fb.sumsq(g, chunk_seg, n_seg, gs)
    wd_s = ((fl & SEG_DECAY) != 0).double() * float(hp[fb.HP_WD])
    wd_s[(fl & SEG_LOW_DECAY) != 0] = float(hp[fb.HP_WD_LOW])
    if rule == "lars":
        wd_s = wd_s * ((fl & SEG_DECAY) != 0)
    gsc_s, gsce_s, knife = fb.clip_scale(ss, sse, clip, gs)
    q_s, qe_s = trust(rule, p, g, chunk_seg, flags, n_seg, ss, sse, hp)
    gsc, gsce, wd, q, qe = (col(x) for x in (gsc_s, gsce_s, wd_s, q_s, qe_s))
    gg = g * gsc
    gge = g.abs() * gsce + U * gg.abs()
    w = wd * p
    d = gg + w
    de = gge + U * w.abs() + U * d.abs()
    if rule == "lars":                                   # (q = 1, bound 0 on the others: the product is exact)
        dq = q * d
        de = torch.where(qe > 0, d.abs() * qe + (q + qe) * de + U * dq.abs(), de)
        d = dq
    mn = m * mu + d
    mne = de + U * (m * mu).abs() + U * mn.abs()
    pn = p - lr * mn
    pne = lr * mne + U * (lr * mn).abs() + U * pn.abs()
    z = torch.zeros_like(p)
    out = {"seg_step": new_step, "knife": int(knife[upd_s].sum()), "seg_sumsq": (ss, sse)}
    if rule == "lars":
        out["seg_trust"] = (q_s, qe_s)
    P, Pe = torch.where(upd, pn, p), torch.where(upd, pne, z)
    out["param"] = (P, Pe)
    out["mom"] = (torch.where(upd, mn, m), torch.where(upd, mne, z))
    out["param16"] = fb.flip(P, Pe)
    if t is not None:
        oem = fb.f32c(1.0) - em
        tn = t * em + oem * P
        tne = oem * Pe + 2 * U * ((t * em).abs() + (oem * P).abs()) + U * tn.abs()
        out["teacher"] = (tn, tne)
        out["teacher16"] = fb.flip(tn, tne)
    return out


def expected(c, d, state=None):
    """{name: (reference, bound)} of one launch pair on d -- or on `state` (p, m, t, step of a previous launch) with d's gradients."""
    s = d if state is None else state
    return step64(c["rule"], s["p"], d["g"], s["m"], s["t"] if c["teacher"] else None, d["chunk_seg"], d["flags"], s["step"], d["hyper"].double(),
                  d["flags"].numel())
