"""What makes tests/test_gpu_layernorm.py and tests/test_gpu_optim.py trustworthy without a GPU (tests/fp64_bounds.py is their oracle).

(a) Non-vacuity caps, as conditions on the oracle itself, for every case of both grids (LayerNorm cases on their first 512 rows where
    larger): no fp32 output's bound may exceed 1e-4 times the magnitude the operation forms at that element --
        y:       |gamma| rstd (|x| + mean|x|) + |beta|
        dx:      rstd (|dy gamma| + mean|dy gamma| + |xhat| mean|dy gamma xhat|) + |g_old|
        dgamma:  sum |dy xhat| (+ |old|);  dbeta: sum |dy| (+ |old|)
        param:   |p| + lr |m^| / (sqrt(v^) + eps)
    -- and at most 2 % of a case's 16-bit outputs may carry a bound wider than one 16-bit step.  The distributions of
    ln_cases.ln_inputs and optim_cases.arena_inputs meet the caps; none of the three had to be changed -- only the exactly constant
    rows hold small values (2^-10, -2^-9) instead of values near 1: at variance 0 rstd = eps^-1/2 multiplies the mean's allowance by
    up to 1000, which for values near 1 exceeds a bf16 step of the outputs.  (The worst case
    is the `offset` distribution: the mean of same-sign values carries sum_depth(D) u mean|x| <= 38 u mean|x|, which rstd |gamma|
    turns into ~38 u of the cap's own magnitude, against the cap's 1e-4 = 1680 u.)  At most one tensor of an arena case may have
    its clip coefficient on the knife edge.
(b) Semantics tie: the fp64 AdamW reference equals torch.optim.AdamW on float64 parameters with utils.clip_gradients per tensor and a
    frozen (grad = None) last layer, over three steps, to 1e-12, step counters included.
(c) Mutation self-test: a CPU fp32 emulation of the kernels passes the oracle, and each seeded fault fails it."""
import pytest
import torch

import fp64_bounds as fb
import ln_cases as lc
import optim_cases as oc
from fp64_bounds import bf16, f32, f64

ROWS = 512
TINY = 1 + 1e-12


def _cap16(name, ref, bound):
    wide = (bound > fb.step16(ref) * (1 + 1e-9)).double().mean().item()
    assert wide <= 0.02, f"{name}: {100 * wide:.2f} % of the 16-bit outputs carry a bound wider than one step"


def _cap32(name, bound, mag):
    assert bool(torch.isfinite(bound).all()) and bool((bound >= 0).all()), name
    over = bound > 1e-4 * mag * TINY
    assert not bool(over.any()), f"{name}: {int(over.sum())} fp32 bounds above the cap, worst ratio {float((bound / (1e-4 * mag))[over].max()):.3g}"


# ------------------------------------------------------------------------------------------------ the emulated LayerNorm kernels
def emulate_ln_fwd(c, d, fault=None):
    """fp32, in the kernels' order of operations: mean, then the sum of squares around it, rsqrt, the scaled output.  Returns y (fp32),
    y16, mean, rstd; a skipped region keeps the 0 the buffers are created with."""
    x, g, b = d["x"].float(), d["gamma"].float(), d["beta"].float()
    R, D = x.shape
    eps = torch.tensor(c["eps"], dtype=f32)
    mean = x.sum(1, keepdim=True) / D
    cc = x - mean
    if fault == "one-pass variance":
        var = (x * x).sum(1, keepdim=True) / D - mean * mean
    else:
        var = (cc * cc).sum(1, keepdim=True) / (D - 1 if fault == "D - 1 in the variance" else D)
    rstd = 1 / (var.clamp_min(0).sqrt() + eps) if fault == "eps added after the square root" else torch.rsqrt(var + eps)
    y = cc * rstd * g + b
    if fault == "last row skipped":
        y[-1], mean[-1], rstd[-1] = 0, 0, 0
    if fault == "last column chunk skipped":
        y[:, (D - 1) // 256 * 256:] = 0
    return y, y.to(bf16), mean, rstd


def emulate_ln_bwd(c, d, mean, rstd, fault=None):
    dy, x, gam = d["dy"].float(), d["x"].float(), d["gamma"].float()
    D = x.shape[1]
    xh = (x - mean) * rstd
    dd = dy * gam
    src = dy if fault == "gamma missing from the row means" else dd
    m1 = src.sum(1, keepdim=True) / D
    m2 = (src * xh).sum(1, keepdim=True) / D
    if fault == "m2 term dropped from dx":
        m2 = torch.zeros_like(m2)
    dx = rstd * (dd - m1 - xh * m2)
    s = d["seq_scale"].float()[d["row2seq"].long()][:, None] if c["scale"] else torch.ones(x.shape[0], 1)
    old = d["g_old"].float() if c["acc"] else torch.zeros_like(dx)
    g = old + s * dx if fault == "scale applied to dx before the accumulate" else old + dx
    if fault == "last row skipped":
        g[-1] = 0
    if fault == "last column chunk skipped":
        g[:, (D - 1) // 256 * 256:] = 0
    return {"g": g, "gb": (s * g).to(bf16), "dgamma": d["dgamma_old"].float() + (dy * xh).sum(0), "dbeta": d["dbeta_old"].float() + dy.sum(0)}


def judge_ln(c, d, fault=None):
    y, y16, mean, rstd = emulate_ln_fwd(c, d, fault)
    exp = lc.fwd_expected(c, d)
    for name, got in (("y", y), ("y16", y16), ("mean", mean), ("rstd", rstd)):
        fb.check(f"{c['id']}: {name}", got, *exp[name], name == "y16")
    # the backward is judged on the statistics it is handed: those of a correct forward
    _, _, mean, rstd = emulate_ln_fwd(c, d)
    got = emulate_ln_bwd(c, d, mean, rstd, fault)
    exp = lc.bwd_expected(c, d, mean.double(), rstd.double())
    for name in ("g", "gb", "dgamma", "dbeta"):
        fb.check(f"{c['id']}: {name}", got[name], *exp[name], name == "gb")


# ------------------------------------------------------------------------------------------------ (a) LayerNorm caps
@pytest.mark.parametrize("c", lc.LN_CASES, ids=[c["id"] for c in lc.LN_CASES])
def test_ln_bounds_are_not_vacuous(c):
    d = lc.ln_inputs(c, rows=ROWS)
    x, gam, bet = d["x"], d["gamma"], d["beta"]
    exp = lc.fwd_expected(c, d)
    r = exp["rstd"][0]
    _cap32(f"{c['id']} y", exp["y"][1], gam.abs() * r * (x.abs() + x.abs().mean(1, keepdim=True)) + bet.abs())
    _cap16(f"{c['id']} y16", *exp["y16"])
    for k in ("mean", "rstd"):
        assert bool(torch.isfinite(exp[k][1]).all()), k
    _cap32(f"{c['id']} rstd", exp["rstd"][1], r)
    # the backward on the fp32 statistics of the emulated forward
    _, _, mean, rstd = emulate_ln_fwd(c, d)
    mean, rstd = mean.double(), rstd.double()
    drop = None
    if c["drop"]:
        gen = torch.Generator()
        gen.manual_seed(lc.seed_of("drop", c["id"]))
        drop = (torch.rand(x.shape, generator=gen) >= lc.DROP_P).double() * fb.f32c(1 / (1 - lc.DROP_P))
    exp = lc.bwd_expected(c, d, mean, rstd, drop)
    xh = (x - mean) * rstd
    dg = (d["dy"] * gam).abs()
    mag = rstd * (dg + dg.mean(1, keepdim=True) + xh.abs() * (dg * xh.abs()).mean(1, keepdim=True))
    if c["acc"]:
        mag = mag + d["g_old"].abs()
    _cap32(f"{c['id']} g", exp["g"][1], mag)
    _cap16(f"{c['id']} gb", *exp["gb"])
    _cap32(f"{c['id']} dgamma", exp["dgamma"][1], (d["dy"] * xh).abs().sum(0) + d["dgamma_old"].abs())
    _cap32(f"{c['id']} dbeta", exp["dbeta"][1], d["dy"].abs().sum(0) + d["dbeta_old"].abs())


# ------------------------------------------------------------------------------------------------ (c) LayerNorm mutations
LN_FAULTS = ["one-pass variance", "eps added after the square root", "D - 1 in the variance", "m2 term dropped from dx",
             "gamma missing from the row means", "scale applied to dx before the accumulate", "last row skipped", "last column chunk skipped"]


def _ln_mut_case(fault):
    # (the one-pass variance shows on same-sign rows; everything else on rows of every scale, where eps matters for the small ones)
    return lc.ln_case("mut-ln-offset", 130, 260, "offset") if fault == "one-pass variance" else lc.ln_case("mut-ln-spread", 130, 260, "spread", eps=1e-5)


@pytest.mark.parametrize("dist", lc.DISTS)
def test_the_emulated_layernorm_passes(dist):
    c = lc.ln_case(f"mut-ln-{dist}", 130, 260, dist, eps=1e-5 if dist == "spread" else 1e-6)
    judge_ln(c, lc.ln_inputs(c))


@pytest.mark.parametrize("fault", LN_FAULTS)
def test_a_seeded_layernorm_fault_fails(fault):
    c = _ln_mut_case(fault)
    d = lc.ln_inputs(c)
    with pytest.raises(AssertionError):
        judge_ln(c, d, fault)
    print(f"rejected: {fault}")


# ------------------------------------------------------------------------------------------------ the emulated arena step
def emulate_step(c, d, fault=None):
    """fp32 clip + AdamW + EMA in the kernel's order of operations over the whole arena; returns its new state."""
    h = d["hyper"]
    lr, wd, b1, b2, eps, clip, em, frz, gs, wdl = (h[i] for i in range(10))
    p, g, m, v, t = (d[k].float() for k in ("p", "g", "m", "v", "t"))
    fl, cs = d["flags"].long(), d["chunk_seg"].long()
    frozen = ((fl & fb.SEG_LAST_LAYER) != 0) & bool(frz != 0)
    upd_s = ((fl & fb.SEG_TRAINABLE) != 0) & ~frozen
    step = d["step"].clone()
    step += ((fl & fb.SEG_TRAINABLE) != 0).int() if fault == "step advanced on a frozen tensor" else upd_s.int()
    ss = torch.zeros(oc.N_SEG, dtype=f32).index_add_(0, cs, (g * g).sum(1)) * gs * gs
    if fault == "global instead of per-tensor clip":
        ss = torch.full_like(ss, float(ss.sum()))
    if fault == "neighbour segment's clip":
        ss = torch.roll(ss, 1)
    gsc = torch.full((oc.N_SEG,), float(gs), dtype=f32)
    if clip > 0:
        coef = clip / (ss.sqrt() + 1e-6)
        gsc = torch.where(coef < 1, gsc * coef, gsc)
    wd_s = torch.where((fl & fb.SEG_DECAY) != 0, wd, torch.zeros((), dtype=f32))
    wd_s = torch.where((fl & fb.SEG_LOW_DECAY) != 0, wd if fault == "LOW_DECAY using wd" else wdl, wd_s)
    tt = step.float()
    bc1, bc2 = 1 - torch.pow(b1, tt), 1 - torch.pow(b2, tt)
    if fault == "bias correction omitted":
        bc1, bc2 = torch.ones_like(bc1), torch.ones_like(bc2)
    col = lambda x: x[cs][:, None]
    gg = g * col(gsc)
    if fault == "coupled instead of decoupled decay":
        gg = gg + col(wd_s) * p
        p1 = p
    else:
        p1 = p * (1 - lr * col(wd_s))
    mn = m * b1 + gg * (1 - b1)
    vn = v * b2 + gg * gg * (1 - b2)
    if fault == "eps inside the square root":
        den = (vn / col(bc2) + eps).sqrt()
    else:
        den = vn.sqrt() * col(torch.rsqrt(bc2)) + eps
    pn = p1 - col(lr / bc1) * mn / den
    u = col(upd_s)
    P = torch.where(u, pn, p)
    tn = t * (1 - em) + em * P if fault == "EMA weights swapped" else t * em + (1 - em) * P
    return {"param": P, "m": torch.where(u, mn, m), "v": torch.where(u, vn, v), "teacher": tn, "param16": P.to(bf16), "teacher16": tn.to(bf16),
            "seg_step": step, "sumsq": ss}


_EXPECTED = {}


def judge_step(c, d, got):
    if c["id"] not in _EXPECTED:                       # (the seeded faults share one case: its reference is computed once)
        _EXPECTED[c["id"]] = oc.expected(c, d)
    (ss, sse), exp = _EXPECTED[c["id"]]
    fb.check(f"{c['id']}: sumsq", got["sumsq"], ss, sse)
    assert torch.equal(got["seg_step"].long(), exp["seg_step"]), f"{c['id']}: seg_step {got['seg_step'].tolist()}, expected {exp['seg_step'].tolist()}"
    for name in ("param", "m", "v", "teacher", "param16", "teacher16"):
        if name in exp:
            fb.check(f"{c['id']}: {name}", got[name], *exp[name], name.endswith("16"))


def test_the_oracle_uses_the_flags_and_hyper_parameter_slots_of_the_abi():
    from lafs_cvpr2024_amd import _lib
    assert (fb.SEG_DECAY, fb.SEG_LAST_LAYER, fb.SEG_TRAINABLE, fb.SEG_LOW_DECAY) == (_lib.SEG_DECAY, _lib.SEG_LAST_LAYER, _lib.SEG_TRAINABLE, _lib.SEG_LOW_DECAY)
    assert fb.CHUNK == _lib.CHUNK
    for n in ("LR", "WD", "BETA1", "BETA2", "EPS", "CLIP", "EMA_M", "FREEZE_LAST", "GRAD_SCALE", "WD_LOW"):
        assert getattr(fb, "HP_" + n) == getattr(_lib, "HP_" + n), n


# ------------------------------------------------------------------------------------------------ (a) arena caps
@pytest.mark.parametrize("c", oc.OPT_CASES, ids=[c["id"] for c in oc.OPT_CASES])
def test_arena_bounds_are_not_vacuous(c):
    d = oc.arena_inputs(c)
    (ss, sse), exp = oc.expected(c, d)
    _cap32(f"{c['id']} sumsq", sse, ss)
    assert exp["knife"] <= 1, f"{c['id']}: {exp['knife']} tensors on the clip knife edge"
    if c["clip"] > 0:
        assert exp["knife"] == 1, "the knife-edge tensor is meant to be undecided"
    hp = d["hyper"].double()
    lr, b1, b2, eps = (float(hp[i]) for i in (fb.HP_LR, fb.HP_BETA1, fb.HP_BETA2, fb.HP_EPS))
    tt = exp["seg_step"].double().clamp_min(1)[d["chunk_seg"].long()][:, None]
    mh, vh = exp["m"][0] / (1 - b1 ** tt), exp["v"][0] / (1 - b2 ** tt)
    _cap32(f"{c['id']} param", exp["param"][1], d["p"].abs() + lr * mh.abs() / (vh.sqrt() + eps))
    # (not asked for by the caps above, but as cheap: the moments and the teacher against the terms they are formed from)
    for k, mag in (("m", d["m"].abs() + d["g"].abs()), ("v", d["v"] + d["g"] ** 2), ("teacher", d["t"].abs() + exp["param"][0].abs())):
        if k in exp:
            _cap32(f"{c['id']} {k}", exp[k][1], mag)
    for k in ("param16", "teacher16"):
        if k in exp:
            _cap16(f"{c['id']} {k}", *exp[k])
    # padding: reference and bound are zero
    for k in ("param", "m", "v", "teacher"):
        if k in exp:
            assert bool((exp[k][0][~d["mask"]] == 0).all()) and bool((exp[k][1][~d["mask"]] == 0).all()), k


# ------------------------------------------------------------------------------------------------ (b) the semantics tie
def test_the_adamw_reference_is_torch_adamw_with_per_tensor_clipping():
    from lafs_cvpr2024_amd.utils import clip_gradients
    c = oc.opt_case("tie", 0, 1)
    d = oc.arena_inputs(c)
    # (semantics do not depend on a tensor's length: the 4100-chunk tensor keeps its first three chunks and its ragged last one)
    full = oc.seg_starts()
    keep = torch.tensor([i for s in range(oc.N_SEG) for i in range(full[s], full[s + 1]) if s != 6 or i < full[s] + 3 or i == full[s + 1] - 1])
    d = {k: (v[keep] if v.shape[:1] == (oc.N_CHUNKS,) else v) for k, v in d.items()}
    st = [0] + torch.cumsum(torch.bincount(d["chunk_seg"].long()), 0).tolist()
    hp = d["hyper"].double()
    lr, wd, b1, b2, eps, clip, em, _, gs, wdl = (float(hp[i]) for i in range(10))
    mask = d["mask"]
    cut = lambda a, i: a[st[i]:st[i + 1]][mask[st[i]:st[i + 1]]].clone()
    params = [torch.nn.Parameter(cut(d["p"], i)) for i in range(oc.N_SEG)]
    model = torch.nn.ParameterList(params)
    trainable = [bool(f & fb.SEG_TRAINABLE) for f in oc.FLAGS]
    frozen = [bool(f & fb.SEG_LAST_LAYER) for f in oc.FLAGS]
    groups = [dict(params=[params[i]], weight_decay=wdl if oc.FLAGS[i] & fb.SEG_LOW_DECAY else wd if oc.FLAGS[i] & fb.SEG_DECAY else 0.0)
              for i in range(oc.N_SEG) if trainable[i]]
    opt = torch.optim.AdamW(groups, lr=lr, betas=(b1, b2), eps=eps)
    teacher = [cut(d["t"], i) for i in range(oc.N_SEG)]
    state = dict(p=d["p"], m=d["m"], v=d["v"], t=d["t"], step=d["step"])
    for it in range(3):
        gen = torch.Generator()
        gen.manual_seed(it)
        d["g"] = (d["g"] * (1 + 0.3 * torch.randn(d["g"].shape, generator=gen, dtype=f64))).to(f32).double()
        for i in range(oc.N_SEG):
            params[i].grad = cut(d["g"], i) * gs if trainable[i] and not frozen[i] else None
        clip_gradients(model, clip)
        opt.step()
        with torch.no_grad():
            for i in range(oc.N_SEG):
                teacher[i] = teacher[i] * em + (1 - em) * params[i]
        _, exp = oc.expected(c, d, state)
        state = dict(p=exp["param"][0], m=exp["m"][0], v=exp["v"][0], t=exp["teacher"][0], step=exp["seg_step"].int())
        for i in range(oc.N_SEG):
            live = trainable[i] and not frozen[i]
            assert int(state["step"][i]) == (it + 1 if live else 0)
            assert (cut(state["p"], i) - params[i].detach()).abs().max() <= 1e-12
            assert (cut(state["t"], i) - teacher[i]).abs().max() <= 1e-12
            if live:
                s = opt.state[params[i]]
                assert int(s["step"]) == it + 1
                assert (cut(state["m"], i) - s["exp_avg"]).abs().max() <= 1e-12 and (cut(state["v"], i) - s["exp_avg_sq"]).abs().max() <= 1e-12
            else:
                assert params[i] not in opt.state or not opt.state[params[i]]
                assert torch.equal(cut(state["p"], i), cut(d["p"], i)) and torch.equal(cut(state["m"], i), cut(d["m"], i))


# ------------------------------------------------------------------------------------------------ (c) arena mutations
OPT_FAULTS = ["bias correction omitted", "coupled instead of decoupled decay", "eps inside the square root", "global instead of per-tensor clip",
              "neighbour segment's clip", "step advanced on a frozen tensor", "EMA weights swapped", "LOW_DECAY using wd"]


@pytest.mark.parametrize("c", oc.OPT_CASES[:3], ids=[c["id"] for c in oc.OPT_CASES[:3]])
def test_the_emulated_step_passes(c):
    d = oc.arena_inputs(c)
    judge_step(c, d, emulate_step(c, d))


_MUT = {}


@pytest.mark.parametrize("fault", OPT_FAULTS)
def test_a_seeded_step_fault_fails(fault):
    c = oc.opt_case("mut-step", 1, 1)            # t = 2, the last layer frozen
    if not _MUT:
        _MUT["d"] = oc.arena_inputs(c)
    d = _MUT["d"]
    with pytest.raises(AssertionError):
        judge_step(c, d, emulate_step(c, d, fault))
    print(f"rejected: {fault}")
