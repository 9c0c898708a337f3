"""What makes tests/test_gpu_cnn_kernels.py trustworthy without a GPU (tests/cnn_cases.py holds its cases and fp64 references).

(a) Non-vacuity caps, as conditions on the oracle itself, for every case: no fp32 / fp64 output's bound may exceed 1e-4 times the
    magnitude the operation forms at that element (sums: sum |terms| + |old|; theta: the value's own terms), at most 2 % of a case's
    16-bit outputs may carry a bound wider than one 16-bit step, and at most 0.1 % of a case's elements may sit on a knife edge of
    an activation derivative (none does: the only kinked backward among these kernels recomputes its pre-activation exactly).  One
    distribution was adjusted to meet the caps: the pooling cases shift their `normal` inputs by 0.5 (cnn_cases._dist says why); the
    same-sign cases use the worst-case accumulation factor and still meet them.
(b) Semantics tie: each fp64 reference with its 16-bit roundings switched off equals the torch statement in float64 to 1e-12 --
    F.conv2d (grouped, stride 2, pad (k - 1) / 2) and its autograd gradients, F.relu / F.hardswish / F.hardsigmoid and their autograd
    derivatives away from the kinks, F.batch_norm in training and eval mode with its running-statistics update and its three autograd
    gradients, mean, the min-max scaling and its autograd gradient with duplicate extrema.
(c) Mutation self-test: a CPU fp32 emulation of each kernel in the kernel's order of operations passes every case, and each seeded
    fault fails at least one."""
import pytest
import torch
import torch.nn.functional as F

import cnn_cases as cc
import fp64_bounds as fb
from fp64_bounds import bf16, f16, f32, f64

TINY = 1 + 1e-12
SIXTH = torch.tensor(1.0, dtype=f32) / 6


def _cap16(name, ref, bound, half):
    wide = (bound > fb.step16(ref, half) * (1 + 1e-9)).double().mean().item()
    assert wide <= 0.02, f"{name}: {100 * wide:.2f} % of the 16-bit outputs carry a bound wider than one step"


def _cap32(name, bound, mag):
    assert bool(torch.isfinite(bound).all()) and bool((bound >= 0).all()), name
    over = bound > 1e-4 * mag * TINY
    assert not bool(over.any()), f"{name}: {int(over.sum())} bounds above the cap, worst ratio {float((bound / (1e-4 * mag))[over].max()):.3g}"


def judge(cid, exp, got):
    for name, out in got.items():
        ref, bound, is16 = exp[name]
        fb.check(f"{cid}: {name}", out.reshape(ref.shape), ref, bound, is16)


# ------------------------------------------------------------------------------------------------ fp32 building blocks
def fma(acc, a, b):
    return (acc.double() + a.double() * b.double()).float()


def act32(v, act):
    if act == 1:
        return v.clamp_min(0)
    if act == 2:
        return v * (v + 3).clamp(0, 6) * SIXTH
    if act == 3:
        return (v + 3).clamp(0, 6) * SIXTH
    return v


def act_grad32(z, act, fault=None):
    one, zero = torch.ones_like(z), torch.zeros_like(z)
    if act == 1:
        return torch.where(z > 0, one, zero)
    if act == 2:
        hi = z > 3 if fault == "hswish' with the z = 3 side swapped" else z >= 3
        return torch.where(z <= -3, zero, torch.where(hi, one, (2 * z + 3) * SIXTH))
    return one


def tree(s):
    """Binary tree over dim 0 (a power of two), upper half added onto the lower."""
    n = s.shape[0]
    while n > 1:
        n //= 2
        s = s[:n] + s[n:2 * n]
    return s[0]


def emu_dw(x, w, b, k, stride, fault=None, floor_ok=True):
    """A chain of fmas over the taps in (ky, kx) order from the bias, NHWC fp32."""
    N, H, W, C = x.shape
    P = (k - 1) // 2
    Ho, Wo = -(-H // stride), -(-W // stride)
    ho, wo = (H // stride, W // stride) if fault == "stride-2 Ho floored instead of ceiled" else (Ho, Wo)
    xp = torch.zeros(N, H + 2 * P + 1, W + 2 * P + 1, C)
    xp[:, P:P + H, P:P + W] = x
    out = torch.zeros(N, Ho, Wo, C)
    if ho == 0 or wo == 0:
        return out

    def chain(sh):
        acc = torch.zeros(N, ho, wo, C) + (0 if b is None else b)
        for ky in range(k):
            for kx in range(k):
                acc = fma(acc, xp[:, ky + sh:ky + sh + stride * (ho - 1) + 1:stride, kx + sh:kx + sh + stride * (wo - 1) + 1:stride], w[ky * k + kx])
        return acc
    acc = chain(0)
    if fault == "depthwise: tap shifted by one at the bottom/right border only":
        sh = chain(1)
        acc[:, -1], acc[:, :, -1] = sh[:, -1], sh[:, :, -1]
    out[:, :ho, :wo] = acc
    return out


# ------------------------------------------------------------------------------------------------ emulated kernels
def emu_stem(c, d, fault=None):
    x, w, b = d["x"].float(), d["w"].float(), d["b"].float()
    N, _, S, _ = x.shape
    So = S // 2
    xp = torch.zeros(N, 3, S + 2, S + 2)
    xp[:, :, 1:S + 1, 1:S + 1] = x
    acc = torch.zeros(N, So, So, 16) + b
    for ch in range(3):
        for ky in range(3):
            for kx in range(3):
                acc = fma(acc, xp[:, ch, ky:ky + 2 * (So - 1) + 1:2, kx:kx + 2 * (So - 1) + 1:2][..., None], w[ch * 9 + ky * 3 + kx])
    y = torch.zeros(N, So, So, c["ldy"], dtype=bf16)
    y[..., :16] = act32(acc, c["act"]).to(bf16)
    if fault == "pad channel written non-zero" and c["ldy"] > 16:
        y[..., -1] = 2.0 ** -20
    return {"y": y}


def emu_dwconv(c, d, fault=None):
    return {"y": act32(emu_dw(d["x"].float(), d["w"].float(), d["b"].float(), c["k"], c["stride"], fault), max(c["act"], 0)).to(bf16)}


def emu_pool(c, d, fault=None):
    x = d["x"].float()
    N, HW, C = x.shape
    inv = torch.tensor(1.0, dtype=f32) / HW
    if cc.pool_route(c) == "thread":
        s = torch.zeros(N, C)
        for p in range(HW):
            s = s + x[:, p]
    else:
        parts = 256 // (C // 8)
        s = torch.zeros(N, C)
        for q in range(parts - 1 if fault == "pooling: last pixel lane dropped" else parts):
            a = torch.zeros(N, C)
            for p in range(q, HW, parts):
                a = a + x[:, p]
            s = s + a
        if fault == "pooling: 1 / HW replaced by 1 / (HW + 1) only on the workgroup route":
            inv = torch.tensor(1.0, dtype=f32) / (HW + 1)
    return {"out": (s * inv).to(bf16)}


def emu_scale_act(c, d, fault=None, dt=bf16):
    return {"y": act32(d["x"].float() * d["s"].float()[:, None], c["act"]).to(dt)}


def emu_im2col(c, d, fault=None):
    P = cc.im2col_expected(c, d)["P"][0].clone()           # (values are moved: the restatement is the emulation)
    if fault == "pad channel written non-zero":
        P[:, 31] = 2.0 ** -14
    return {"P": P.to(f16)}


def emu_stats(c, d, fault=None):
    R, C = c["R"], c["C"]
    x = d["x"][:, :C].float()
    rpb, RL = cc.rows_per_block(R), 256 // cc.group_block(c["ld"])
    nblk, T = -(-R // rpb), rpb // RL
    xb = torch.zeros(nblk * rpb, C)
    xb[:R] = x
    xb = xb.view(nblk, T, RL, C)
    live = (torch.arange(nblk * rpb) < R).view(nblk, T, RL)
    n_l = live.sum(1, keepdim=True)
    if fault == "BN stats: the <4-row tail skipped":
        live = live & (torch.arange(T).view(1, T, 1) < n_l // 4 * 4)
    s1, s2 = torch.zeros(nblk, RL, C), torch.zeros(nblk, RL, C)
    for t in range(T):
        v = xb[:, t] * live[:, t, :, None]
        s1, s2 = s1 + v, fma(s2, v, v)
    p1, p2 = tree(s1.transpose(0, 1)), tree(s2.transpose(0, 1))
    return {"sums": d["old"] + torch.cat([p1.double().sum(0), p2.double().sum(0)])}


def col_reduce(c_ld, v1, a2, b2, live=None):
    """col_reduce2 of landmark_train.hip: per workgroup of rows_per_block rows, 256 / GB row lanes each adding its rows in sequence
    (s1 += v1, s2 = fma(a2, b2, s2)), a tree over the lanes, the workgroups' partials added in fp64."""
    R, C = v1.shape
    rpb, RL = cc.rows_per_block(R), 256 // cc.group_block(c_ld)
    nblk, T = -(-R // rpb), rpb // RL
    blk = lambda v: torch.cat([v, torch.zeros(nblk * rpb - R, C)]).view(nblk, T, RL, C)
    v1, a2, b2 = blk(v1), blk(a2), blk(b2)
    s1, s2 = torch.zeros(nblk, RL, C), torch.zeros(nblk, RL, C)
    for t in range(T):
        s1, s2 = s1 + v1[:, t], fma(s2, a2[:, t], b2[:, t])
    return tree(s1.transpose(0, 1)).double().sum(0), tree(s2.transpose(0, 1)).double().sum(0)


def emu_bn_apply(c, d, fault=None):
    R, C, ld = c["R"], c["C"], c["ld"]
    s1, s2 = d["sums"][:C], d["sums"][C:]
    eps = torch.tensor(cc.BN_EPS, dtype=f32)
    md = s1 * (1.0 / R)
    vd = (s2 * (1.0 / R) - md * md).clamp_min(0)
    m, var = md.float(), vd.float()
    if fault == "unbiased factor used for the normalising variance":
        vd = vd * R / max(R - 1, 1)
    rs = (1.0 / (vd + eps.double()).sqrt()).float()
    if fault == "E[x^2] - mean^2 formed in fp32":
        var = ((s2 / R).float() - m * m).clamp_min(0)
        rs = 1.0 / (var + eps).sqrt()
    g, b, x = d["gamma"].float(), d["beta"].float(), d["x"][:, :C].float()
    scale = rs * g
    shift = b - m * scale
    a = act32(fma(shift, x, scale), c["act"])
    if c["resid"]:
        a = a + d["resid"][:, :C].float()
    y = torch.zeros(R, ld, dtype=f16)
    y[:, :C] = a.to(f16)
    if fault == "pad channel written non-zero" and ld > C:
        y[:, C] = 2.0 ** -14
    out = {"y": y, "stat": torch.cat([m, rs])}
    if c["run"]:
        mom = torch.tensor(c["mom"], dtype=f32)
        out["rm"] = (1 - mom) * d["rm"].float() + mom * m
        out["rv"] = (1 - mom) * d["rv"].float() + mom * var * (torch.tensor(float(R)) / torch.tensor(float(max(R - 1, 1))))
    return out


def emu_bn_bwd(c, d, stat, fault=None, frozen=False, dsums_old=None):
    R, C, ld = c["R"], c["C"], c["ld"]
    x, dy, g, b = d["x"][:, :C].float(), d["dy"][:, :C].float(), d["gamma"].float(), d["beta"].float()
    m, rs = stat[:C].float(), stat[C:].float()
    dd = dy
    if c["HW"]:
        a = d["add"][:, :C].float().repeat_interleave(c["HW"], 0)
        dd = dy + a if fault == "add_nc not divided by HW" else fma(dy, a, torch.tensor(1.0, dtype=f32) / c["HW"])
    xh = (x - m) * rs
    dz = dd * act_grad32(fma(b, xh, g), c["act"], fault)
    p1, p2 = col_reduce(ld, dz, dz, xh)
    old = torch.zeros(2 * C, dtype=f64) if dsums_old is None else dsums_old
    s = torch.cat([p1, p2]) + old
    c4, c5 = (torch.zeros(C), torch.zeros(C)) if frozen else ((s[:C] / R).float(), (s[C:] / R).float())
    if fault == "BN backward: xhat term dropped":
        c5 = torch.zeros(C)
    dx = torch.zeros(R, ld, dtype=f16)
    dx[:, :C] = (g * rs * (dz - c4 - xh * c5)).to(f16)
    out = {"dsums": s, "dx": dx}
    if c["affine"]:
        inv = 1.0 if c["gs"] is None else 1.0 / c["gs"]
        out["dgamma"] = d["dgamma_old"].float() + (s[C:] * inv).float()
        out["dbeta"] = d["dbeta_old"].float() + (s[:C] * inv).float()
    return out


def emu_tables(spec, d, inv=1.0, fault=None):
    T, m = spec["T"], d["master"].float()
    cast = torch.full((T.cast_size,), cc.SENT16, dtype=f16)
    for src, rows, cols, doff, ld, tr, prow, _ in T.cast:
        i = torch.arange(prow * ld)
        dr, dc = i // ld, i % ld
        sr, sc = (dc, dr) if tr else (dr, dc)
        ok = (sr < rows) & (sc < cols)
        cast[doff + i] = torch.where(ok, m[(src + sr * cols + sc).clamp_max(m.numel() - 1)], torch.zeros(())).to(f16)
    dwl = torch.full((T.dw_size,), cc.SENT16)
    for src, C, kk, doff, ld, *_ in T.dwl:
        i = torch.arange(kk * ld)
        t, ch = i // ld, i % ld
        dwl[doff + i] = torch.where(ch < C, m[(src + ch * kk + t).clamp_max(m.numel() - 1)], torch.zeros(()))
    grad, pad = d["grad_old"].float().clone(), d["padded"].float()
    for src, rows, cols, ld, goff, tr, *_ in T.fold:
        i = torch.arange(rows * cols)
        r, cl = i // cols, i % cols
        at = src + cl * ld + r if tr and fault != "fold: transpose ignored for depthwise entries" else src + r * ld + cl
        grad[goff + i] += torch.tensor(inv, dtype=f32) * pad[at]
    return {"cast": cast, "dwl": dwl, "grad": grad}


def _lane_tree(terms, PL, fault=None, prod=None):
    """terms [N, HW, C] dealt to PL lanes (p = lane, lane + PL, ...), each lane in sequence (fma with `prod` where given), then the tree."""
    N, HW, C = terms.shape
    T = -(-HW // PL)
    pad = lambda v: torch.cat([v, torch.zeros(N, T * PL - HW, C)], 1).view(N, T, PL, C)
    a, b = pad(terms), None if prod is None else pad(prod)
    acc = torch.zeros(N, PL, C)
    for t in range(T):
        acc = acc + a[:, t] if b is None else fma(acc, a[:, t], b[:, t])
    if fault == "pooling: last pixel lane dropped":
        acc[:, PL - 1] = 0
    return tree(acc.transpose(0, 1))


def emu_pool_train(c, d, fault=None):
    x = d["x"].float()
    HW = c["HW"]
    inv = torch.tensor(1.0, dtype=f32) / HW
    out = (_lane_tree(x, 256 // cc.group_block(c["ld"]), fault) * inv).to(f16)
    dx = (d["dfeat"].float() * inv).to(f16)[:, None].expand(-1, HW, -1)
    return {"out": out, "dx": dx}


def emu_se(c, d, fault=None):
    z, g, do = d["z"].float(), d["gate"].float()[:, None], d["dout"].float()
    p = z * g
    ds = do * act_grad32(p, c["act"], fault)
    return {"out": act32(p, c["act"]).to(f16), "dz": (ds * g).to(f16), "dgate": _lane_tree(ds, 256 // cc.group_block(c["ld"]), prod=z)}


def emu_act_post(c, d, fault=None):
    y, dy = d["y"].float(), d["dy"].float()
    g = torch.ones_like(y)
    if c["act"] == 1:
        g = (y > 0).float()
    if c["act"] == 3:
        g = ((y > 0) & (y < 1)).float() * SIXTH
    return {"out": (dy * g).to(f16)}


def emu_cast(c, d, fault=None):
    dst = torch.zeros(c["rows"], c["ld"], dtype=f16)
    dst[:, :c["cols"]] = (d["src"].float() * torch.tensor(1.0 if c["scale"] is None else c["scale"], dtype=f32)).to(f16)
    return {"dst": dst}


def emu_dwt(c, d, fault=None):
    k, st, C, K = c["k"], c["stride"], c["C"], c["k"] ** 2
    x, dy, w = d["x"].float(), d["dy"].float(), d["w"].float()
    N, H, W, ld = x.shape
    P = (k - 1) // 2
    Ho, Wo = dy.shape[1:3]
    y = emu_dw(x, w, None, k, st, fault)
    xp = torch.zeros(N, H + 2 * P, W + 2 * P, ld)
    xp[:, P:P + H, P:P + W] = x
    dxp = torch.zeros_like(xp)
    taps = []
    for ky in range(k):
        for kx in range(k):
            sl = (slice(None), slice(ky, ky + st * (Ho - 1) + 1, st), slice(kx, kx + st * (Wo - 1) + 1, st))
            dxp[sl] = fma(dxp[sl], dy, w[ky * k + kx])
            taps.append(xp[sl])
    dx = dxp[:, P:P + H, P:P + W].clone()
    # dw: slabs of pix_per_block pixels, 256 threads each walking its pixels in sequence, a tree, one atomic per slab
    npix = N * Ho * Wo
    ppb = max(1024, -(-npix // 256))
    xt = torch.stack(taps, 3).view(npix, K, ld)
    g = dy.reshape(npix, 1, ld).expand(-1, K, -1)
    dw = d["dw_old"].float().clone()
    for p0 in range(0, npix, ppb):
        n = min(ppb, npix - p0)
        J = -(-n // 256)
        pad = lambda v: torch.cat([v[p0:p0 + n], torch.zeros(J * 256 - n, K, ld)]).view(J, 256, K, ld)
        a, b = pad(g), pad(xt)
        acc = torch.zeros(256, K, ld)
        for j in range(J):
            acc = fma(acc, a[j], b[j])
        dw[:, :C] = dw[:, :C] + tree(acc)[:, :C]
    if fault == "pad channel written non-zero" and ld > C:
        y[..., C] = 2.0 ** -14
    return {"y": y.to(f16), "dx": dx.to(f16), "dw": dw}


def emu_theta(c, d, fault=None):
    t = d["t"].float()
    mn, mx = t.min(1, keepdim=True).values, t.max(1, keepdim=True).values
    v = (t - mn) / (mx - mn) * 111.0
    if c["noise"]:
        v = v + torch.tensor(cc.NOISE_SCALE, dtype=f32) * d["noise"].float()
    if c["sel"]:
        v = v.gather(1, (2 * d["sel"].long()[:, :, None] + torch.arange(2)).view(t.shape[0], -1))
    return {"theta": v[:, :2 * c["n_out"]]}


def emu_theta_bwd(c, d, fault=None):
    t, g = d["t"].float(), d["dtheta"].float()
    n = t.shape[1]
    mn, mx = t.min(1, keepdim=True).values, t.max(1, keepdim=True).values
    if fault == "theta_bwd: last occurrence instead of first":
        imn, imx = n - 1 - (t.flip(1) == mn).float().argmax(1, keepdim=True), n - 1 - (t.flip(1) == mx).float().argmax(1, keepdim=True)
    else:
        imn, imx = (t == mn).float().argmax(1, keepdim=True), (t == mx).float().argmax(1, keepdim=True)
    r = mx - mn
    k, k2 = 111.0 / r, 111.0 / (r * r)
    dt = g * k
    T = -(-n // 256)
    lanes = lambda v: torch.cat([v, torch.zeros(v.shape[0], T * 256 - n)], 1).view(-1, T, 256)
    ta, tb = lanes(g * k2 * (t - mx)), lanes(g * k2 * (t - mn))
    a, b = torch.zeros(t.shape[0], 256), torch.zeros(t.shape[0], 256)
    for j in range(T):
        a, b = a + ta[:, j], b - tb[:, j]
    a, b = tree(a.t())[:, None], tree(b.t())[:, None]
    if fault == "theta_bwd: d/dmin and d/dmax exchanged":
        a, b = b, a
    dt.scatter_add_(1, imn, a)
    dt.scatter_add_(1, imx, b)
    return {"dt": dt}


def emu_grad_scale(c, d, fault=None):
    g = d["g"].float()
    a = g.abs()
    ok = a < 3.0e38
    m = a[ok].max() if bool(ok.any()) else torch.tensor(0.0)
    target = torch.tensor(c["state_target"] if c["state_target"] > 0 else c["target"], dtype=f32)
    s = target / m if m > 0 else torch.tensor(1.0)
    s = s.clamp(2.0 ** -24, 2.0 ** 24)
    lg = torch.log2(s)
    s = torch.exp2(torch.ceil(lg) if fault == "grad_scale: ceil instead of floor" else torch.floor(lg))
    return float(s), float(1.0 / s), 0.0 if bool(ok.all()) else 1.0


FAMILIES = {
    "stem": (cc.STEM_CASES, cc.stem_inputs, cc.stem_expected, emu_stem),
    "dwconv": (cc.DW_CASES, cc.dw_inputs, cc.dw_expected, emu_dwconv),
    "pool": (cc.POOL_CASES, cc.pool_inputs, cc.pool_expected, emu_pool),
    "scale_act": (cc.SCALE_ACT_CASES, cc.scale_inputs, cc.scale_expected, emu_scale_act),
    "im2col": (cc.IM2COL_CASES, cc.im2col_inputs, cc.im2col_expected, emu_im2col),
    "stats": (cc.STATS_CASES, cc.stats_inputs, cc.stats_expected, emu_stats),
    "pool_train": (cc.POOL_TRAIN_CASES, cc.pool_train_inputs, cc.pool_train_expected, emu_pool_train),
    "se": (cc.SE_CASES, cc.se_inputs, cc.se_expected, emu_se),
    "act_post": (cc.ACT_POST_CASES, cc.act_post_inputs, cc.act_post_expected, emu_act_post),
    "cast": (cc.CAST_CASES, cc.cast_inputs, cc.cast_expected, emu_cast),
    "dwt": (cc.DWT_CASES, cc.dwt_inputs, cc.dwt_expected, emu_dwt),
    "theta": (cc.THETA_CASES, cc.theta_inputs, cc.theta_expected, emu_theta),
}
HALF = {"im2col", "pool_train", "se", "act_post", "cast", "dwt"}           # fp16 families (the others store bf16)
MAGS = {"sums": "mag", "dgate": "mag", "dw": "mag_dw"}
ALL = [(f, c) for f, (cases, *_) in FAMILIES.items() for c in cases]
_CACHE = {}


def _case(fam, c):
    """(inputs, expected) of a case, computed once and left unchanged."""
    if c["id"] not in _CACHE:
        _, inputs, expected, _ = FAMILIES[fam]
        d = inputs(c)
        _CACHE[c["id"]] = (d, expected(c, d))
    return _CACHE[c["id"]]


# ------------------------------------------------------------------------------------------------ (a) caps
@pytest.mark.parametrize("fam,c", ALL, ids=[c["id"] for _, c in ALL])
def test_bounds_are_not_vacuous(fam, c):
    d, exp = _case(fam, c)
    for name, val in exp.items():
        if not isinstance(val, tuple):
            continue
        ref, bound, is16 = val
        assert ref.shape == bound.shape
        if is16:
            _cap16(f"{c['id']} {name}", ref, bound, fam in HALF)
        elif name == "theta":
            _cap32(f"{c['id']} {name}", bound, ref.abs() + 1e-30)
        else:
            _cap32(f"{c['id']} {name}", bound, exp[MAGS[name]][..., :ref.shape[-1]] if name == "dw" else exp[MAGS[name]])
    n_el = sum(v[0].numel() for v in exp.values() if isinstance(v, tuple))
    assert exp.get("knife", 0) <= 1e-3 * n_el


@pytest.mark.parametrize("kind", cc.THETA_BWD_KINDS)
def test_theta_bwd_bounds_are_not_vacuous(kind):
    for c in cc.THETA_CASES[::2]:
        d = cc.theta_structured(c, kind)
        exp = cc.theta_bwd_expected(c, d)
        _cap32(f"{c['id']}-{kind}", exp["dt"][1], exp["mag"])


# ------------------------------------------------------------------------------------------------ (b) semantics
def _close(a, b, name):
    assert a.shape == b.shape and float((a - b).abs().max()) <= 1e-12 * max(1.0, float(b.abs().max())), name


@pytest.mark.parametrize("k,stride,H,W", [(k, s, H, W) for k in (3, 5) for s in (1, 2) for H, W in cc.DW_PLANES])
def test_depthwise_reference_is_conv2d_and_its_autograd(k, stride, H, W):
    gen = torch.Generator()
    gen.manual_seed(cc.seed_of("tie", k, stride, H, W))
    N, C = 2, 5
    x = torch.randn(N, H, W, C, generator=gen, dtype=f64)
    w = torch.randn(k * k, C, generator=gen, dtype=f64)
    xt = x.permute(0, 3, 1, 2).clone().requires_grad_()
    wt = w.t().reshape(C, 1, k, k).clone().requires_grad_()
    y = F.conv2d(xt, wt, None, stride, (k - 1) // 2, 1, C)
    v, s = fb.dwconv(x, w, k, stride)
    _close(v, y.detach().permute(0, 2, 3, 1), "value")
    _close(s, F.conv2d(xt.abs(), wt.abs(), None, stride, (k - 1) // 2, 1, C).detach().permute(0, 2, 3, 1), "sum |terms|")
    dy = torch.randn(y.shape, generator=gen, dtype=f64)
    y.backward(dy)
    (dx, _), (dw, _) = fb.dwconv_bwd(x, dy.permute(0, 2, 3, 1), w, k, stride)
    _close(dx, xt.grad.permute(0, 2, 3, 1), "dx")
    _close(dw, wt.grad.reshape(C, k * k).t(), "dw")


@pytest.mark.parametrize("N,S", cc.STEM_PLANES)
def test_stem_reference_is_conv2d_stride_2_pad_1(N, S):
    c = dict(id=f"tie-stem-{N}-{S}", N=N, S=S, ldy=16, act=2, coded=False)
    d = cc.stem_inputs(c)
    y = F.hardswish(F.conv2d(d["x"], d["w"].t().reshape(16, 3, 3, 3), d["b"], 2, 1))
    ref = cc.stem_expected(c, d, r16=lambda v: v)["y"][0]
    _close(ref, y.permute(0, 2, 3, 1), "stem")


def test_activation_references_are_torch_and_its_autograd():
    z = torch.linspace(-7, 7, 2801, dtype=f64) + 1e-3                       # (away from the kinks)
    zero = torch.zeros_like(z)
    for kind, fn in ((fb.ACT_RELU, F.relu), (fb.ACT_HSWISH, F.hardswish), (fb.ACT_HSIGMOID, F.hardsigmoid)):
        zz = z.clone().requires_grad_()
        y = fn(zz)
        y.sum().backward()
        _close(fb.act(z, zero, kind)[0], y.detach(), f"act {kind}")
        d, e, knife = fb.act_grad(z, zero, kind)
        if kind == fb.ACT_HSIGMOID:
            # (torch's own hardsigmoid backward multiplies by the fp32 constant 1 / 6 even on float64 tensors, 5e-9 off: the derivative
            # is tied to the autograd of the clamp form, whose value is tied to F.hardsigmoid just above)
            zz = z.clone().requires_grad_()
            ((zz + 3).clamp(0, 6) / 6).sum().backward()
        _close(d, zz.grad, f"act' {kind}")
        assert not bool(knife.any()) and float(e.max()) < 1e-6
    # the knife edges: within ze of a kink the bound admits both branches
    z = torch.tensor([-3.0, 0.0, 3.0], dtype=f64)
    for kind, jump in ((fb.ACT_RELU, (0, 1, 0)), (fb.ACT_HSWISH, (0.5, 0, 0.5)), (fb.ACT_HSIGMOID, (1 / 6, 0, 1 / 6))):
        _, e, knife = fb.act_grad(z, torch.full_like(z, 1e-6), kind)
        assert knife.tolist() == [j > 0 for j in jump] and all(float(e[i]) >= jump[i] for i in range(3))


def test_pool_reference_is_the_mean():
    x = torch.randn(2, 49, 24, dtype=f64)
    _close(fb.col_mean(x, 1, lambda v: v)[0], x.mean(1), "mean")


@pytest.mark.parametrize("kind", cc.THETA_BWD_KINDS)
def test_theta_references_are_the_min_max_scaling_and_its_autograd(kind):
    for c in cc.THETA_CASES:
        d = cc.theta_structured(c, kind)
        t = d["t"].clone().requires_grad_()
        mn, mx = t.min(1, keepdim=True).values, t.max(1, keepdim=True).values          # (torch.min(dim): gradient to the first occurrence)
        th = (t - mn) / (mx - mn) * 111
        full = th + (cc.NOISE_SCALE * d["noise"] if c["noise"] else 0)
        if c["sel"]:
            full = full.gather(1, (2 * d["sel"].long()[:, :, None] + torch.arange(2)).view(t.shape[0], -1))
        _close(cc.theta_expected(c, d)["theta"][0], full.detach()[:, :2 * c["n_out"]], "theta")
        th.backward(d["dtheta"])
        first = lambda m: (d["t"] == m).double().argmax(1)
        sel = torch.zeros_like(d["t"])
        # (torch spreads the gradient of min / max over ties in some versions: compare on the row sums and off the extrema, and pin
        # the first-occurrence rule itself with index_select below)
        ref = cc.theta_bwd_expected(c, d)["dt"][0]
        ext = (d["t"] == mn.detach()) | (d["t"] == mx.detach())
        _close(torch.where(ext, sel, ref), torch.where(ext, sel, t.grad), "dt off the extrema")
        _close(ref.sum(1), t.grad.sum(1), "row sums")
        # first occurrence: an explicit index_select formulation
        t2 = d["t"].clone().requires_grad_()
        rows = torch.arange(t2.shape[0])
        mn2, mx2 = t2[rows, first(mn.detach())][:, None], t2[rows, first(mx.detach())][:, None]
        ((t2 - mn2) / (mx2 - mn2) * 111).backward(d["dtheta"])
        _close(ref, t2.grad, "dt")


# ------------------------------------------------------------------------------------------------ (c) emulation and faults
@pytest.mark.parametrize("fam,c", ALL, ids=[c["id"] for _, c in ALL])
def test_the_emulated_kernel_passes(fam, c):
    d, exp = _case(fam, c)
    judge(c["id"], exp, FAMILIES[fam][3](c, d))


@pytest.mark.parametrize("kind", cc.THETA_BWD_KINDS)
def test_the_emulated_theta_bwd_passes(kind):
    for c in cc.THETA_CASES[::2]:
        d = cc.theta_structured(c, kind)
        judge(f"{c['id']}-{kind}", cc.theta_bwd_expected(c, d), emu_theta_bwd(c, d))


def test_squeeze_excite_on_the_kinks_emulated():
    for act in (1, 2):
        c = dict(id=f"se-kink-act{act}", HW=49, ld=24, N=2, act=act, wide=8, dist="normal")
        d = cc.se_inputs(c, kink=True)
        judge(c["id"], cc.se_expected(c, d), emu_se(c, d))


@pytest.mark.parametrize("c", cc.GS_CASES, ids=[c["id"] for c in cc.GS_CASES])
def test_the_emulated_grad_scale_meets_its_contract(c):
    cc.gs_contract(c, *emu_grad_scale(c, cc.gs_inputs(c)))


def test_guard_state_machine():
    s, z = cc.guard_ref([8.0, 0.125, 1024.0, 1.0, 3.0, 17.0, 0.0, 0.0], 4096.0)
    assert z and s == [8.0, 0.125, 512.0, 1.0, 4.0, 0.0, 0.0, 0.0]
    s, z = cc.guard_ref([8.0, 0.125, 1024.0, 0.0, 3.0, 1999.0, 0.0, 0.0], 4096.0)
    assert not z and s == [8.0, 0.125, 2048.0, 0.0, 3.0, 0.0, 0.0, 0.0]


def _fails(fam, fault, pick=lambda c: True):
    """The ids of the cases of a family that the fault fails."""
    cases, _, _, emu = FAMILIES[fam]
    bad = []
    for c in cases:
        if not pick(c):
            continue
        d, exp = _case(fam, c)
        try:
            judge(c["id"], exp, emu(c, d, fault))
        except AssertionError:
            bad.append(c["id"])
    return bad


FAULTS = {
    "depthwise: tap shifted by one at the bottom/right border only": ("dwconv", "dwt"),
    "stride-2 Ho floored instead of ceiled": ("dwconv", "dwt"),
    "pooling: last pixel lane dropped": ("pool", "pool_train"),
    "pooling: 1 / HW replaced by 1 / (HW + 1) only on the workgroup route": ("pool",),
    "BN stats: the <4-row tail skipped": ("stats",),
    "pad channel written non-zero": ("stem", "im2col", "dwt"),
}


@pytest.mark.parametrize("fault", list(FAULTS))
def test_a_seeded_fault_fails(fault):
    for fam in FAULTS[fault]:
        bad = _fails(fam, fault)
        assert bad, f"{fault}: passes every case of {fam}"
        print(f"rejected: {fault} ({fam}): {len(bad)} cases, first {bad[0]}")


def test_the_pooling_factor_fault_shows_on_the_workgroup_route_only():
    bad = _fails("pool", "pooling: 1 / HW replaced by 1 / (HW + 1) only on the workgroup route")
    wg = [c["id"] for c in cc.POOL_CASES if cc.pool_route(c) == "wg"]
    assert bad and set(bad) <= set(wg)


def test_the_hswish_side_at_3_fails_on_the_kink_case():
    c = dict(id="se-kink-act2", HW=49, ld=24, N=2, act=2, wide=8, dist="normal")
    d = cc.se_inputs(c, kink=True)
    with pytest.raises(AssertionError):
        judge(c["id"], cc.se_expected(c, d), emu_se(c, d, "hswish' with the z = 3 side swapped"))


@pytest.mark.parametrize("fault", ["theta_bwd: last occurrence instead of first", "theta_bwd: d/dmin and d/dmax exchanged"])
def test_a_seeded_theta_bwd_fault_fails(fault):
    bad = 0
    for kind in cc.THETA_BWD_KINDS:
        for c in cc.THETA_CASES[::2]:
            d = cc.theta_structured(c, kind)
            try:
                judge(c["id"], cc.theta_bwd_expected(c, d), emu_theta_bwd(c, d, fault))
            except AssertionError:
                bad += 1
    assert bad, fault


def test_grad_scale_ceil_instead_of_floor_fails():
    bad = 0
    for c in cc.GS_CASES:
        try:
            cc.gs_contract(c, *emu_grad_scale(c, cc.gs_inputs(c), "grad_scale: ceil instead of floor"))
        except AssertionError:
            bad += 1
    assert bad


# ------------------------------------------------------------------------------------------------ BatchNorm and the tables
def host_case(c):
    """The 16.8 M-element case of the GPU module is judged here on 4099 rows of the same distribution (its id says so)."""
    return c if c["R"] < 100000 else dict(c, R=4099, id=c["id"] + "-on-4099-rows")


BN_HOST = [host_case(c) for c in cc.BN_CASES]
BN_IDS = [c["id"] for c in BN_HOST]
_BN = {}


def _bn(c):
    """(inputs, apply reference, the emulated apply's fp32 statistics, backward reference on them)."""
    if c["id"] not in _BN:
        d = cc.bn_inputs(c)
        stat = emu_bn_apply(c, d)["stat"].double()
        old = d["dgamma_old"].repeat(2)[:2 * c["C"]] if "dsums-old" in c["id"] else None
        _BN[c["id"]] = (d, cc.bn_apply_expected(c, d), stat, old, {f: cc.bn_bwd_expected(c, d, stat, f, old) for _, f in cc.bn_bwd_modes(c)})
    return _BN[c["id"]]


@pytest.mark.parametrize("c", BN_HOST, ids=BN_IDS)
def test_batchnorm_bounds_are_not_vacuous(c):
    d, fwd, stat, old, bwd = _bn(c)
    _cap16(f"{c['id']} y", fwd["y"][0], fwd["y"][1], True)
    for k in ("stat", "rm", "rv"):
        if k in fwd:
            _cap32(f"{c['id']} {k}", fwd[k][1], fwd["mag_" + k])
    for frozen, exp in bwd.items():
        _cap16(f"{c['id']} dx", exp["dx"][0], exp["dx"][1], True)
        for k in ("dsums", "dgamma", "dbeta"):
            if k in exp:
                _cap32(f"{c['id']} {k}", exp[k][1], exp["mag_" + k] + 1e-300)
        assert exp["knife"] <= 1e-3 * c["R"] * c["C"], f"{c['id']}: {exp['knife']} elements on a knife edge"
        assert bool((exp["knife_share"] <= 0.5 * exp["dsums"][1]).all()), f"{c['id']}: a sum owes more than half its bound to knife edges"


@pytest.mark.parametrize("c", BN_HOST, ids=BN_IDS)
def test_the_emulated_batchnorm_passes(c):
    d, fwd, stat, old, bwd = _bn(c)
    judge(c["id"], fwd, emu_bn_apply(c, d))
    for frozen, exp in bwd.items():
        judge(f"{c['id']} frozen={frozen}", exp, emu_bn_bwd(c, d, stat, None, frozen, old))


def _bn_fails(fault, which):
    bad = []
    for c in BN_HOST:
        d, fwd, stat, old, bwd = _bn(c)
        try:
            if which == "apply":
                judge(c["id"], fwd, emu_bn_apply(c, d, fault))
            elif which == "y":
                judge(c["id"], {"y": fwd["y"]}, {"y": emu_bn_apply(c, d, fault)["y"]})
            else:
                if False in bwd:
                    judge(c["id"], bwd[False], emu_bn_bwd(c, d, stat, fault, False, old))
        except AssertionError:
            bad.append(c["id"])
    return bad


@pytest.mark.parametrize("fault,which", [("unbiased factor used for the normalising variance", "apply"), ("pad channel written non-zero", "apply"),
                                         ("BN backward: xhat term dropped", "bwd"), ("add_nc not divided by HW", "bwd")])
def test_a_seeded_batchnorm_fault_fails(fault, which):
    bad = _bn_fails(fault, which)
    assert bad, fault
    print(f"rejected: {fault}: {len(bad)} cases, first {bad[0]}")


def test_the_fp32_variance_fails_the_offset_cases_only():
    """E[x^2] - mean^2 formed in fp32, judged on y (the output the fp64 sums exist for).  At |mean| = 30 std the difference loses
    log2(900) ~ 10 of its 24 bits: the variance is off by up to 900 u = 5e-5, rstd by half of that, y by ~5 % of an fp16 step -- a few
    per cent of the elements flip, nearly all of them where the bound is 0.  On the zero-mean and all-positive cases the same arithmetic
    moves rstd by at most one fp32 ulp, 1e-4 of an fp16 step: `only` is asserted as a share of elements (none of a case of < 100 000
    elements; a 264 000-element case loses two), because a bit-exact check cannot let a whole case pass a one-ulp change of rstd."""
    hit = []
    for c in BN_HOST:
        d, fwd, *_ = _bn(c)
        y = emu_bn_apply(c, d, "E[x^2] - mean^2 formed in fp32")["y"].double()
        ref, bound, _ = fwd["y"]
        share = float(((y - ref).abs() > bound).double().mean())
        if c["dist"] == "offset" and c["R"] > 1 and c["R"] * c["C"] >= 1000:
            assert share >= 5e-3, f"{c['id']}: only {share:.2e} of y out of bounds"
            hit.append(c["id"])
        elif c["dist"] != "offset":
            assert share <= 1e-4 and (share == 0 or c["R"] * c["C"] >= 100000), f"{c['id']}: {share:.2e} of y out of bounds"
    assert len(hit) >= 3
    print(f"rejected on: {hit}")


def test_batchnorm_on_the_kinks_emulated_and_the_swapped_side_fails():
    for act in (1, 2):
        c = dict(id=f"bn-kink-act{act}", R=60, C=8, ld=8, act=act, dist="normal", resid=False, mom=0.1, run=False, HW=None, gs=None, affine=True,
                 const=False)
        d = cc.bn_inputs(c, exact_z=True)
        stat = torch.cat([torch.zeros(8), torch.ones(8)]).double()
        exp = cc.bn_bwd_expected(c, d, stat, exact_z=True)
        assert exp["knife"] == 0
        judge(c["id"], exp, emu_bn_bwd(c, d, stat))
        if act == 2:
            with pytest.raises(AssertionError):
                judge(c["id"], exp, emu_bn_bwd(c, d, stat, "hswish' with the z = 3 side swapped"))


@pytest.mark.parametrize("training", [True, False])
@pytest.mark.parametrize("act,HW", [(0, None), (1, 4), (2, None)])
def test_batchnorm_references_are_torch_batch_norm_and_its_autograd(training, act, HW):
    """With both roundings switched off: F.batch_norm in training mode (batch statistics, biased variance, running statistics updated
    with the unbiased one) and in eval mode (through the sums lafs_cnn_bn_eval_sums states), then the activation and the residual; the
    three gradients by autograd, the squeeze-excite pooling gradient add / HW entering at the block's output."""
    ident = lambda v: v
    fn = {0: ident, 1: F.relu, 2: F.hardswish}[act]
    c = dict(id=f"tie-bn-{training}-{act}-{HW}", R=24, C=20, ld=32, act=act, dist="normal", resid=True, mom=0.1, run=training, HW=HW, gs=None,
             affine=True, const=False)
    d = cc.bn_inputs(c)
    C = c["C"]
    if not training:
        d["sums"] = cc.bn_eval_sums_expected(d["rm"], d["rv"], c["R"])["sums"][0]
    fwd = cc.bn_apply_expected(c, d, r32=ident, rh=ident)
    x = d["x"][:, :C].clone().requires_grad_()
    g, b = d["gamma"].clone().requires_grad_(), d["beta"].clone().requires_grad_()
    rm, rv = d["rm"].clone(), d["rv"].clone()
    z = F.batch_norm(x, rm, rv, g, b, training, fb.f32c(0.1), fb.f32c(cc.BN_EPS))
    y = fn(z) + d["resid"][:, :C]
    _close(fwd["y"][0][:, :C], y.detach(), "y")
    if training:
        _close(fwd["rm"][0], rm, "running_mean")
        _close(fwd["rv"][0], rv, "running_var")
        _close(fwd["stat"][0][:C], x.detach().mean(0), "mean")
        _close(fwd["stat"][0][C:], 1 / (x.detach().var(0, unbiased=False) + fb.f32c(cc.BN_EPS)).sqrt(), "rstd")
    # the backward differentiates act(z) alone (the residual branch takes dy as it is)
    dz_in = d["dy"][:, :C] + (d["add"][:, :C].repeat_interleave(HW, 0) / HW if HW else 0)
    fn(z).backward(dz_in)
    bwd = cc.bn_bwd_expected(c, d, fwd["stat"][0], frozen=not training, rh=ident)
    _close(bwd["dx"][0][:, :C], x.grad, "dx")
    _close(bwd["dgamma"][0] - d["dgamma_old"], g.grad, "dgamma")
    _close(bwd["dbeta"][0] - d["dbeta_old"], b.grad, "dbeta")


def test_the_emulated_tables_pass_and_the_ignored_transpose_fails():
    spec = cc.table_entries()
    d = cc.table_inputs(spec)
    for inv in (1.0, 1 / 64.0):
        exp = cc.tables_expected(spec, d, inv)
        judge("tables", exp, emu_tables(spec, d, inv))
        with pytest.raises(AssertionError):
            judge("tables", exp, emu_tables(spec, d, inv, "fold: transpose ignored for depthwise entries"))
    # what no entry covers keeps what it held
    exp = cc.tables_expected(spec, d)
    a = spec["arena"]
    for gap in ("gap0", "gap1"):
        sl = slice(a[gap][0], a[gap][0] + a[gap][1])
        assert torch.equal(exp["grad"][0][sl], d["grad_old"][sl]) and bool((exp["grad"][1][sl] == 0).all())
    assert int((exp["cast"][0] == cc.SENT16).sum()) >= 63          # the 1025-element image leaves 63 gap elements
