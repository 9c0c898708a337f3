"""What makes tests/test_gpu_sgd_lars.py trustworthy without a GPU, and the host side of --optimizer sgd / lars.

(a) The entry point's parser takes the reference's three optimizers; the two hyper slots sit where the header says.
(b) Semantics ties of the fp64 restatement (tests/sgd_lars_cases.py): SGD equals torch.optim.SGD(momentum=0.9) on float64 parameters
    with utils.clip_gradients per tensor and a frozen (grad = None) last layer, over three steps with changing lr and wd; LARS equals
    the reference's own class on fixture F31 (tests/golden/f31_lars.npz, tools/make_golden_lars.py), every step, every tensor,
    parameters and mu.  Both to 1e-12, the tolerance of test_the_adamw_reference_is_torch_adamw_with_per_tensor_clipping.
(c) Non-vacuity caps (_cap32 / _cap16 of tests/test_oracle_rowops_host.py) for every case: no fp32 bound above 1e-4 of the magnitude
    of the terms that form the value --
        mom:  |momentum mu| + q (|g^| + |wd p|)        param:  |p| + lr x (the terms of mom)        teacher: |t| + |p'|
        seg_sumsq: the sum itself         seg_trust: q
    -- at most one tensor per case on the clip knife edge.
(d) Mutation self-test: an fp32 CPU emulation of the kernels in their operation order passes every case; each seeded fault fails.
(e) The two entry points refuse bad arguments before any launch."""
import ctypes as C
import os
import re

import pytest
import torch

import fp64_bounds as fb
import sgd_lars_cases as sc
from conftest import load_golden
from fp64_bounds import CHUNK, bf16, f32, f64
from test_oracle_rowops_host import _cap16, _cap32

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
_CACHE = {}


def case_data(c):
    """(inputs, expected) of a case, computed once per module run (the arena has 4.2 M elements)."""
    if c["id"] not in _CACHE:
        d = sc.arena_inputs(c)
        _CACHE[c["id"]] = (d, sc.expected(c, d))
    return _CACHE[c["id"]]


# ------------------------------------------------------------------------------------------------ (a) parser and slots
@pytest.mark.parametrize("opt", ["adamw", "sgd", "lars"])
def test_the_parser_accepts_the_reference_optimizers(opt):
    from lafs_cvpr2024_amd.lafs_train import get_args_parser
    assert get_args_parser().parse_args(["--optimizer", opt]).optimizer == opt


def test_the_hyper_slots_are_those_of_the_header():
    from lafs_cvpr2024_amd import _lib
    assert (_lib.HP_MOMENTUM, _lib.HP_LARS_ETA) == (13, 14) == (sc.HP_MOMENTUM, sc.HP_LARS_ETA)
    assert _lib.HP_MOMENTUM < _lib.HP_COUNT and _lib.HP_LARS_ETA < _lib.HP_COUNT and _lib.HP_COUNT == 16
    txt = open(os.path.join(ROOT, "include", "lafs_hip.h")).read()
    assert re.search(r"\bLAFS_HP_MOMENTUM\s*=\s*13\b", txt) and re.search(r"\bLAFS_HP_LARS_ETA\s*=\s*14\b", txt)
    assert re.search(r"\bLAFS_HP_COUNT\s*=\s*16\b", txt)
    assert re.search(r"\bLAFS_UPDATE_SGD\s*=\s*1\b", txt) and re.search(r"\bLAFS_UPDATE_LARS\s*=\s*2\b", txt)
    assert (_lib.UPDATE_SGD, _lib.UPDATE_LARS) == (sc.UPDATE["sgd"], sc.UPDATE["lars"]) == (1, 2)
    # the slots below them are still the ones the fine-tune step uses
    assert (_lib.HP_STEP, _lib.HP_MIX_LAM, _lib.HP_LAND_W) == (10, 11, 12)


# ------------------------------------------------------------------------------------------------ (b) semantics ties
def test_the_sgd_reference_is_torch_sgd_with_per_tensor_clipping():
    from lafs_cvpr2024_amd.utils import clip_gradients
    c = sc.case("sgd", "tie", 0, 1)
    d = sc.arena_inputs(c)
    full = sc.seg_starts()                              # (the 4100-chunk tensor keeps its first three chunks and its ragged last one)
    keep = torch.tensor([i for s in range(sc.N_SEG) for i in range(full[s], full[s + 1]) if s != 6 or i < full[s] + 3 or i == full[s + 1] - 1])
    d = {k: (v[keep] if v.shape[:1] == (sc.N_CHUNKS,) else v) for k, v in d.items()}
    st = [0] + torch.cumsum(torch.bincount(d["chunk_seg"].long()), 0).tolist()
    mask = d["mask"]
    cut = lambda a, i: a[st[i]:st[i + 1]][mask[st[i]:st[i + 1]]].clone()
    params = [torch.nn.Parameter(cut(d["p"], i)) for i in range(sc.N_SEG)]
    model = torch.nn.ParameterList(params)
    trainable = [bool(f & fb.SEG_TRAINABLE) for f in sc.FLAGS]
    last = [bool(f & fb.SEG_LAST_LAYER) for f in sc.FLAGS]
    kind = ["low" if f & fb.SEG_LOW_DECAY else "wd" if f & fb.SEG_DECAY else "none" for f in sc.FLAGS]
    hp = d["hyper"].double()
    gs, em, clip, mom = (float(hp[i]) for i in (fb.HP_GRAD_SCALE, fb.HP_EMA_M, fb.HP_CLIP, sc.HP_MOMENTUM))
    groups = [dict(params=[params[i]], kind=kind[i]) for i in range(sc.N_SEG) if trainable[i]]
    opt = torch.optim.SGD(groups, lr=0, momentum=mom)
    teacher = [cut(d["t"], i) for i in range(sc.N_SEG)]
    state = dict(p=d["p"], m=d["m"], t=d["t"], step=d["step"])
    # (lr, wd, wd_low, last layer frozen) per step: frozen for two steps, then released with an empty momentum buffer
    for it, (lr, wd, wdl, frz) in enumerate([(5e-2, 0.04, 0.02, 1), (3e-2, 0.1, 0.0, 1), (1e-2, 0.0, 0.3, 0)]):
        hp[fb.HP_LR], hp[fb.HP_WD], hp[fb.HP_WD_LOW], hp[fb.HP_FREEZE_LAST] = lr, wd, wdl, frz
        for g in opt.param_groups:
            g["lr"], g["weight_decay"] = lr, {"low": wdl, "wd": wd, "none": 0.0}[g["kind"]]
        gen = torch.Generator()
        gen.manual_seed(it)
        d["g"] = (d["g"] * (1 + 0.3 * torch.randn(d["g"].shape, generator=gen, dtype=f64))).to(f32).double()
        for i in range(sc.N_SEG):
            params[i].grad = cut(d["g"], i) * gs if trainable[i] and not (last[i] and frz) else None
        clip_gradients(model, clip)
        opt.step()
        with torch.no_grad():
            for i in range(sc.N_SEG):
                teacher[i] = teacher[i] * em + (1 - em) * params[i]
        exp = sc.step64("sgd", state["p"], d["g"], state["m"], state["t"], d["chunk_seg"], d["flags"], state["step"], hp, sc.N_SEG)
        state = dict(p=exp["param"][0], m=exp["mom"][0], t=exp["teacher"][0], step=exp["seg_step"].int())
        for i in range(sc.N_SEG):
            steps = 0 if not trainable[i] else it + 1 if not last[i] else max(0, it - 1)       # (the last layer: released at it = 2)
            stepped = steps > 0
            assert int(state["step"][i]) == steps
            assert (cut(state["p"], i) - params[i].detach()).abs().max() <= 1e-12
            assert (cut(state["t"], i) - teacher[i]).abs().max() <= 1e-12
            if stepped:
                assert (cut(state["m"], i) - opt.state[params[i]]["momentum_buffer"]).abs().max() <= 1e-12
            else:
                assert params[i] not in opt.state or opt.state[params[i]].get("momentum_buffer") is None
                assert torch.equal(cut(state["p"], i), cut(d["p"], i)) and torch.equal(cut(state["m"], i), cut(d["m"], i))


def test_the_lars_reference_is_the_reference_class_on_f31():
    z = load_golden("f31_lars")
    names = ["w57", "v11", "w234", "z44"]
    shapes = [z["p0." + n].shape for n in names]
    assert [tuple(s) for s in shapes] == [(5, 7), (11,), (2, 3, 4), (4, 4)] and bool((z["p0.z44"] == 0).all())
    assert bool((z["g1.w57"] == 0).all()) and float(z["wd"][1]) == 0.0, "one step has wd = 0 and a zero gradient on a matrix"
    n_seg = len(names)
    pack = lambda key: torch.stack([torch.cat([z[f"{key}.{n}"].double().flatten(), torch.zeros(CHUNK - z[f"{key}.{n}"].numel(), dtype=f64)]) for n in names])
    chunk_seg = torch.arange(n_seg, dtype=torch.int32)
    flags = torch.tensor([fb.SEG_TRAINABLE | (fb.SEG_DECAY if len(s) != 1 else 0) for s in shapes], dtype=torch.int32)
    p, m, step = pack("p0"), torch.zeros(n_seg, CHUNK, dtype=f64), torch.zeros(n_seg, dtype=torch.int32)
    for it in range(3):
        hp = torch.zeros(16, dtype=f64)
        hp[fb.HP_LR], hp[fb.HP_WD], hp[fb.HP_GRAD_SCALE] = float(z["lr"][it]), float(z["wd"][it]), 1.0           # clip 0: disabled
        hp[sc.HP_MOMENTUM], hp[sc.HP_LARS_ETA] = float(z["momentum"]), float(z["eta"])
        exp = sc.step64("lars", p, pack(f"g{it}"), m, None, chunk_seg, flags, step, hp, n_seg)
        p, m, step = exp["param"][0], exp["mom"][0], exp["seg_step"].int()
        assert (p - pack(f"p{it + 1}")).abs().max() <= 1e-12, f"parameters after step {it + 1}"
        assert (m - pack(f"mu{it + 1}")).abs().max() <= 1e-12, f"mu after step {it + 1}"
        q = exp["seg_trust"][0]
        assert float(q[1]) == 1.0, "the 1-D tensor is not adapted"
        if it == 0:
            assert float(q[3]) == 1.0, "||p|| = 0: q = 1"
        if it == 1:
            assert float(q[0]) == 1.0, "||d|| = 0: q = 1"
    assert step.tolist() == [3, 3, 3, 3]


# ------------------------------------------------------------------------------------------------ (c) caps
@pytest.mark.parametrize("c", sc.CASES, ids=[c["id"] for c in sc.CASES])
def test_bounds_are_not_vacuous(c):
    d, exp = case_data(c)
    hp = d["hyper"].double()
    lr, mu, wd, wdl = (float(hp[i]) for i in (fb.HP_LR, sc.HP_MOMENTUM, fb.HP_WD, fb.HP_WD_LOW))
    ss, sse = exp["seg_sumsq"]
    _cap32(f"{c['id']} seg_sumsq", sse, ss)
    assert exp["knife"] <= 1, f"{c['id']}: {exp['knife']} tensors on the clip knife edge"
    if c["clip"] > 0:
        assert exp["knife"] == 1, "the knife-edge tensor is meant to be undecided"
    cs, fl = d["chunk_seg"].long(), d["flags"].long()
    col = lambda x: x[cs][:, None]
    q = torch.ones(sc.N_SEG, dtype=f64)
    if c["rule"] == "lars":
        q, qe = exp["seg_trust"]
        _cap32(f"{c['id']} seg_trust", qe, q)
        st = sc.seg_starts()
        dec = (fl & fb.SEG_DECAY) != 0
        assert bool((q[~dec] == 1).all()) and float(q[sc.ZERO_P]) == 1.0, "no adaptation without SEG_DECAY, nor at ||p|| = 0"
        eta = float(hp[sc.HP_LARS_ETA])
        if c["wd"] > 0:
            assert abs(float(q[sc.ZERO_G]) - eta / wd) <= 1e-12 * eta / wd, "zero gradient: q = eta / wd"
        else:
            assert float(q[sc.ZERO_G]) == 1.0, "zero gradient and wd = 0: ||d|| = 0, q = 1"
        assert bool(((q[dec] < 0.1) | (q[dec] == 1)).all()), "a trust ratio of the arena is eta-sized"
    wd_s = ((fl & fb.SEG_DECAY) != 0).double() * wd
    wd_s[(fl & fb.SEG_LOW_DECAY) != 0] = wdl
    if c["rule"] == "lars":
        wd_s = wd_s * ((fl & fb.SEG_DECAY) != 0)
    ssq, _, _ = fb.clip_scale(ss, sse, c["clip"], float(hp[fb.HP_GRAD_SCALE]))
    terms = col(q) * ((d["g"] * col(ssq)).abs() + (col(wd_s) * d["p"]).abs())
    _cap32(f"{c['id']} mom", exp["mom"][1], (d["m"] * mu).abs() + terms)
    _cap32(f"{c['id']} param", exp["param"][1], d["p"].abs() + lr * ((d["m"] * mu).abs() + terms))
    if c["teacher"]:
        _cap32(f"{c['id']} teacher", exp["teacher"][1], d["t"].abs() + exp["param"][0].abs())
        _cap16(f"{c['id']} teacher16", *exp["teacher16"])
    else:
        assert "teacher" not in exp
    _cap16(f"{c['id']} param16", *exp["param16"])
    for k in ("param", "mom", "teacher"):                # padding: reference and bound are zero
        if k in exp:
            assert bool((exp[k][0][~d["mask"]] == 0).all()) and bool((exp[k][1][~d["mask"]] == 0).all()), k
    # tensors that take no step: the reference is the input, the bound 0
    skip = col(exp["seg_step"] == d["step"].long()).expand_as(d["p"])
    assert skip.any() and torch.equal(exp["param"][0][skip], d["p"][skip]) and torch.equal(exp["mom"][0][skip], d["m"][skip])
    assert bool((exp["param"][1][skip] == 0).all()) and bool((exp["mom"][1][skip] == 0).all())


# ------------------------------------------------------------------------------------------------ (d) emulation and mutations
FAULTS = ["mu <- mu + momentum d", "decay applied to a non-decay tensor", "decoupled decay", "adaptation applied to the 1-D tensor", "q without eta",
          "q inverted", "q = 0 at ||p|| = 0", "clip coefficient ignored", "frozen last layer updated", "mu not stored", "EMA taken from the old p",
          "update range off by one chunk", "seg_sumsq not scaled by gs^2"]
ONE_D = 1                                                # a trainable tensor without SEG_DECAY


def emulate(c, d, fault=None):
    """fp32 reduction + clip + SGD / LARS + EMA in the kernels' order of operations over the whole arena; returns the new state."""
    h = d["hyper"]
    lr, wd, clip, em, frz, gs, wdl = (h[i] for i in (fb.HP_LR, fb.HP_WD, fb.HP_CLIP, fb.HP_EMA_M, fb.HP_FREEZE_LAST, fb.HP_GRAD_SCALE, fb.HP_WD_LOW))
    mu, eta = h[sc.HP_MOMENTUM], h[sc.HP_LARS_ETA]
    lars = c["rule"] == "lars"
    p, g, m, t = (d[k].float() for k in ("p", "g", "m", "t"))
    fl, cs = d["flags"].long(), d["chunk_seg"].long()
    frozen = ((fl & fb.SEG_LAST_LAYER) != 0) & bool(frz != 0) & (fault != "frozen last layer updated")
    upd_s = ((fl & fb.SEG_TRAINABLE) != 0) & ~frozen
    step = d["step"] + upd_s.int()
    fold = lambda x: torch.zeros(sc.N_SEG, dtype=f32).index_add_(0, cs, x.sum(1))
    G, P, X = fold(g * g), fold(p * p), fold(g * p)
    ss = G if fault == "seg_sumsq not scaled by gs^2" else G * gs * gs
    gsc = torch.full((sc.N_SEG,), float(gs), dtype=f32)
    if clip > 0 and fault != "clip coefficient ignored":
        coef = clip / (ss.sqrt() + 1e-6)
        gsc = torch.where(coef < 1, gsc * coef, gsc)
    dec = (fl & fb.SEG_DECAY) != 0
    zero = torch.zeros((), dtype=f32)
    wd_s = torch.where((fl & fb.SEG_LOW_DECAY) != 0, wdl, torch.where(dec, wd, zero))
    if lars:
        wd_s = torch.where(dec, wd_s, zero)
    if fault == "decay applied to a non-decay tensor":
        wd_s[ONE_D] = wd
    q = torch.ones(sc.N_SEG, dtype=f32)
    if lars:
        adapt = dec.clone()
        if fault == "adaptation applied to the 1-D tensor":
            adapt[ONE_D] = True
        dd = gsc * gsc * G + 2 * gsc * wd_s * X + wd_s * wd_s * P
        ratio = P.sqrt() / dd.sqrt() if fault == "q without eta" else dd.sqrt() / (eta * P.sqrt()) if fault == "q inverted" else eta * P.sqrt() / dd.sqrt()
        q = torch.where(adapt & (P > 0) & (dd > 0), ratio, q)
        if fault == "q = 0 at ||p|| = 0":
            q = torch.where(adapt & (P == 0), zero, q)
    col = lambda x: x[cs][:, None]
    gg = g * col(gsc)
    if fault == "decoupled decay":
        dv, p1 = gg, p * (1 - lr * col(wd_s))
    else:
        dv, p1 = gg + col(wd_s) * p, p
    if lars:
        dv = dv * col(q)
    mn = m + mu * dv if fault == "mu <- mu + momentum d" else m * mu + dv
    pn = p1 - lr * mn
    u = col(upd_s).expand_as(p).clone()
    if fault == "update range off by one chunk":
        u[0] = False
    P_ = torch.where(u, pn, p)
    tn = t * em + (1 - em) * (p if fault == "EMA taken from the old p" else P_)
    out = {"param": P_, "mom": m if fault == "mu not stored" else torch.where(u, mn, m), "teacher": tn, "param16": P_.to(bf16), "teacher16": tn.to(bf16),
           "seg_step": step, "seg_sumsq": ss}
    if lars:
        out["seg_trust"] = q
    return out


def judge(c, exp, got):
    assert torch.equal(got["seg_step"].long(), exp["seg_step"]), f"{c['id']}: seg_step {got['seg_step'].tolist()}, expected {exp['seg_step'].tolist()}"
    for name in ("seg_sumsq", "seg_trust", "param", "mom", "teacher", "param16", "teacher16"):
        if name in exp:
            fb.check(f"{c['id']}: {name}", got[name], *exp[name], name.endswith("16"))


@pytest.mark.parametrize("c", sc.CASES, ids=[c["id"] for c in sc.CASES])
def test_the_emulated_step_passes(c):
    d, exp = case_data(c)
    judge(c, exp, emulate(c, d))


@pytest.mark.parametrize("fault", FAULTS)
def test_a_seeded_fault_fails(fault):
    """Each fault fails at least one case: looked for among the LARS cases (every fault can show there), first hit ends the search."""
    hits = []
    for c in [c for c in sc.CASES if c["rule"] == "lars"]:
        d, exp = case_data(c)
        try:
            judge(c, exp, emulate(c, d, fault))
        except AssertionError:
            hits.append(c["id"])
            break
    assert hits, f"no case notices: {fault}"
    print(f"rejected by {hits[0]}: {fault}")


@pytest.mark.parametrize("fault", [f for f in FAULTS if not f.startswith(("q ", "adaptation"))])
def test_a_seeded_fault_fails_under_sgd(fault):
    hits = []
    for c in [c for c in sc.CASES if c["rule"] == "sgd"]:
        d, exp = case_data(c)
        try:
            judge(c, exp, emulate(c, d, fault))
        except AssertionError:
            hits.append(c["id"])
            break
    assert hits, f"no case notices: {fault}"


# ------------------------------------------------------------------------------------------------ (e) argument rejection
def test_bad_arguments_are_rejected_before_any_launch():
    """A range that leaves the arena, an unknown kind, LARS without seg_trust, null mandatory pointers: rc < 0 and lafs_last_error() is
    set, no GPU needed (host buffers stand in for the pointers: nothing is launched)."""
    from lafs_cvpr2024_amd import _lib
    h = _lib.lib()
    buf = (C.c_float * 16)()
    ptr = C.cast(buf, C.c_void_p)
    none = C.c_void_p(None)
    n_chunks, n_seg = 4, 2
    upd = lambda kind, lo, hi, trust, param=ptr: h.lafs_clip_momentum_ema_range(kind, param, ptr, ptr, none, none, none, ptr, n_chunks, lo, hi, ptr, ptr,
                                                                               n_seg, 0, n_seg, ptr, trust, ptr, None)
    red = lambda lo, hi, s_hi, trust=ptr: h.lafs_grad_sumsq_trust_range(ptr, ptr, ptr, n_chunks, n_seg, lo, hi, 0, s_hi, ptr, ptr, ptr, ptr, trust, None)
    for what, rc in (("update: range past the arena", upd(_lib.UPDATE_LARS, 0, n_chunks + 1, ptr)), ("update: empty range", upd(_lib.UPDATE_SGD, 2, 2, none)),
                     ("update: negative start", upd(_lib.UPDATE_SGD, -1, 2, none)),
                     ("update: unknown kind", upd(3, 0, n_chunks, ptr)), ("update: kind 0", upd(0, 0, n_chunks, ptr)),
                     ("update: LARS without seg_trust", upd(_lib.UPDATE_LARS, 0, n_chunks, none)),
                     ("update: null param", upd(_lib.UPDATE_SGD, 0, n_chunks, none, param=none)),
                     ("reduction: range past the arena", red(0, n_chunks + 1, n_seg)), ("reduction: tensors past the arena", red(0, n_chunks, n_seg + 1)),
                     ("reduction: null seg_trust", red(0, n_chunks, n_seg, trust=none))):
        assert rc < 0 and h.lafs_last_error(), what
