"""What makes tests/test_gpu_dino_head.py trustworthy without a GPU (tests/fp64_bounds.py is its oracle, tests/dino_cases.py its grid).

(a) Non-vacuity caps, as conditions on the oracle itself, for every case of the grids: at most 2 % of a case's 16-bit outputs may
    carry a bound wider than one 16-bit step, and no fp32 bound may exceed 1e-4 max(1, A / 32) times the magnitude formed at that
    element (A: the row's largest |logit / tau|; 1 for the row kernels) --
        gradient:  coef (n_v p + sum q)
        loss:      mean (n_v |lse| + |dot|)
        dx:        inv (|dy| + |y| sum|y dy|);  dv: likewise with g inv, plus |dv_old|
    Two departures from "every case, every element", both stated in `_loss_caps`: gradient elements whose n_v p + sum q lies within
    3e4 of fp32's smallest normal number (a flushed exponential alone is 1e-4 of them) are judged but not capped; and the bf16
    gradient at K = 1, identically 0, takes the fp32 cap in the 16-bit cap's place.  The loss's cap holds for every case as stated.
    The distributions that had to be adjusted to meet the caps are described where they are made (dino_cases.logits: K <= 8).
(b) Semantics tie, to 1e-12: the fp64 references equal torch in float64 on the loss's double loop over teacher views and student
    crops and the centre update restated with autograd, on F.normalize, on nn.utils.weight_norm(dim=0) forward and gradients, and the
    fused form equals the unfused form applied to zn wn^T.
(c) Mutation self-test: an fp32 CPU emulation of each kernel (its formulas, constants and number domains; torch's summation order)
    passes the oracle on every case of the grids, and each seeded fault fails it on a case that the GPU grid contains."""
import pytest
import torch

import dino_cases as dc
import fp64_bounds as fb
from fp64_bounds import bf16, f32, f64
from test_oracle_rowops_host import _cap16, _cap32

F = lambda v: torch.tensor(v, dtype=f32)
BY_ID = {c["id"]: c for g in (dc.ROW_CASES, dc.WN_CASES, dc.LOSS_CASES, dc.HEAD_CASES, dc.COLSUM_CASES, dc.EMA_CASES) for c in g}


# ------------------------------------------------------------------------------------------------ the emulated kernels (fp32)
def emulate_l2(c, d, fault=None):
    x, dy = d["x"].float(), d["dy"].float()
    n = (x * x).sum(1, keepdim=True).sqrt()
    inv = 1 / (n if fault == "l2norm clamp missing" else n.clamp_min(1e-12))
    y = x * inv
    s = (y * dy).sum(1, keepdim=True)
    if fault == "<y, dy> term dropped":
        s = torch.zeros_like(s)
    dx = inv * (dy - y * s)
    y16 = y.to(bf16)
    if fault == "last row of a four-row workgroup skipped":
        y16[3::4], dx[3::4] = 0, 0
    return inv, y16, dx


def emulate_wn_bwd(c, d, inv, fault=None):
    v, dw, g = d["x"].float(), d["dy"].float(), d["g"].float()
    vh = v * inv
    s = (vh * dw).sum(1, keepdim=True)
    dv = (inv if fault == "weight-norm g missing from dv" else g * inv) * (dw - vh * s)
    dg = s
    if c["acc"]:
        dg = d["dg_old"].float() + s
        if fault != "accumulate overwrites":
            dv = dv + d["dv_old"].float()
    if fault == "last row of a four-row workgroup skipped":
        dv[3::4] = 0
    return dv, dg


def emulate_wn_fwd(c, d):
    v, g = d["v"].float(), d["g"].float()
    inv = torch.rsqrt((v * v).sum(1, keepdim=True))
    return inv, (v * (g * inv)).to(bf16)


def emulate_loss(c, s, t, center, fault=None, fused=False):
    """Both loss kernels from their logits on, with the kernels' constants and domains (not their summation order): log2-domain
    statistics with the rounded constant fl(1 / tau) fl(log2 e); unfused: the fp32 ln 2 product on the statistics, p and q as exp of
    natural-domain arguments; fused: p and q as exp2 of log2-domain arguments minus the log2-domain statistic, ln 2 in the loss
    only; coef as the host forms it and as the device corrects it."""
    nc, B, K = c["ncrops"], c["B"], c["K"]
    hs, ht = dc.host_temps(c)
    coef = F(1.0 if fault == "grad_scale ignored" else c["scale"]) / (F(float(2 * nc - 2)) * F(float(B)) * F(hs))
    its, itt = 1 / F(hs), 1 / F(ht)
    if c["dev"]:
        if fault != "coef not corrected for the device temperatures":
            coef = coef / (its * F(c["ts"]))
        its, itt = 1 / F(c["ts"]), 1 / F(c["tt"])
    if fault == "teacher temperature used for the student":
        its = itt
    s, t, center = s.float(), t.float(), center.float()
    a_s = s * its
    a_t = t * itt - center if fault == "centre subtracted after the temperature scaling" else (t - center) * itt

    def lse(z, it):
        a2 = z * (it * F(fb.LOG2E))
        if fault == "last class block dropped from the log-sum-exp":
            a2 = a2[:, :(K - 1) // 64 * 64]
        if fault == "pad column counted in the sum":
            a2 = torch.cat([a2, torch.zeros(a2.shape[0], 1)], 1)
        m = torch.zeros(a2.shape[0], 1) if fault == "the row's maximum not subtracted" else a2.max(1, keepdim=True).values
        return m + torch.log2(torch.exp2(a2 - m).sum(1, keepdim=True))

    l2s = lse(s, its)
    l2t = lse(a_t / itt if fault == "centre subtracted after the temperature scaling" else t - center, itt)
    Ls, Lt = l2s * F(fb.LN2), l2t * F(fb.LN2)
    if fused:
        p, q = torch.exp2(s * (its * F(fb.LOG2E)) - l2s), torch.exp2((t - center) * (itt * F(fb.LOG2E)) - l2t)
    else:
        p, q = torch.exp(a_s - Ls), torch.exp(a_t - Lt)
    q0, q1 = q[:B].repeat(nc, 1), q[B:].repeat(nc, 1)
    v = (torch.arange(nc * B) // B)[:, None]
    if fault == "q_0 and q_1 swapped for crops 0 and 1":
        qs = torch.where(v == 0, q0, torch.where(v == 1, q1, q0 + q1))
    else:
        qs = torch.where(v == 0, q1, torch.where(v == 1, q0, q0 + q1))
    nv = torch.ones_like(v, dtype=f32) if fault == "n_v = 1 for the local crops" else (1 + (v >= 2)).float()
    grad = coef * (nv * p - qs)
    term = qs * a_s
    if fault == "last class of a ragged tail dropped":
        grad[:, -1], term[:, -1] = 0, 0
    dots = term.sum(1, keepdim=True)
    loss = (nv * Ls - dots).sum() / float((2 * nc - 2) * B)
    colsum = (t[:B] if fault == "column sum over B rows instead of 2 B" else t).sum(0)
    return {"grad": grad.to(bf16) if c["g16"] else grad, "loss": loss.reshape(1), "dots": dots, "colsum": colsum, "q": q, "p": p}


def emulate_ema(c, d, fault=None):
    m, om = F(c["m"]), 1 - F(c["m"])
    if fault == "EMA with m and 1 - m exchanged":
        m, om = om, m
    return d["center"].float() * m + d["colsum"].float() * F(c["inv_rows"]) * om


# ------------------------------------------------------------------------------------------------ judges
def judge_rows(c, fault=None):
    d = dc.row_inputs(c)
    inv, y16, dx = emulate_l2(c, d, fault)
    exp = dc.l2_fwd_expected(c, d)
    fb.check(f"{c['id']}: inv_norm", inv, *exp["inv"])
    fb.check(f"{c['id']}: y", y16, *exp["y16"], True)
    inv = emulate_l2(c, d)[0]                                       # the backward is judged on a correct forward's statistics
    fb.check(f"{c['id']}: dx", dx, *dc.l2_bwd_expected(c, d, inv.double()))
    d = dc.row_inputs(c, weight=True)
    inv = torch.rsqrt((d["x"].float() ** 2).sum(1, keepdim=True))
    dv, dg = emulate_wn_bwd(c, d, inv, fault)
    exp = dc.wn_bwd_expected(c, d, inv.double())
    fb.check(f"{c['id']}: dv", dv, *exp["dv"])
    fb.check(f"{c['id']}: dg", dg, *exp["dg"])


def judge_loss(c, fault=None):
    d = dc.loss_inputs(c)
    got = emulate_loss(c, d["s"], d["t"], d["center"], fault)
    exp = dc.loss_expected(c, d)
    for k in ("q", "p", "dots", "loss"):
        fb.check(f"{c['id']}: {k}", got[k], *exp[k])
    fb.check(f"{c['id']}: grad", got["grad"], *exp["grad"], c["g16"])


def judge_head(c, fault=None):
    d = dc.head_inputs(c)
    K = c["K"]
    s, t = d["zs"].float() @ d["ws"][:K].float().t(), d["zt"].float() @ d["wt"][:K].float().t()
    got = emulate_loss(c, s, t, d["center"], fault, fused=True)
    exp = dc.head_expected(c, d)
    for k in ("loss", "colsum"):
        fb.check(f"{c['id']}: {k}", got[k], *exp[k])
    fb.check(f"{c['id']}: grad", got["grad"], *exp["grad"], True)


def judge_ema(c, fault=None):
    d = dc.ema_inputs(c)
    fb.check(f"{c['id']}: centre", emulate_ema(c, d, fault), *dc.ema_expected(c, d))


# ------------------------------------------------------------------------------------------------ (a) caps
@pytest.mark.parametrize("c", dc.ROW_CASES, ids=[c["id"] for c in dc.ROW_CASES])
def test_row_bounds_are_not_vacuous(c):
    d = dc.row_inputs(c)
    exp = dc.l2_fwd_expected(c, d)
    inv = exp["inv"][0]
    _cap32(f"{c['id']} inv", exp["inv"][1], inv)
    _cap16(f"{c['id']} y16", *exp["y16"])
    y, dy = d["x"] * inv, d["dy"]
    _cap32(f"{c['id']} dx", dc.l2_bwd_expected(c, d, inv)[1], inv * (dy.abs() + y.abs() * (y * dy).abs().sum(1, keepdim=True)))
    d = dc.row_inputs(c, weight=True)
    inv = fb.weightnorm_fwd(d["x"], d["g"])["inv"][0]
    exp = dc.wn_bwd_expected(c, d, inv)
    vh, dw = d["x"] * inv, d["dy"]
    sa = (vh * dw).abs().sum(1, keepdim=True)
    _cap32(f"{c['id']} dv", exp["dv"][1], (d["g"] * inv).abs() * (dw.abs() + vh.abs() * sa) + (d["dv_old"].abs() if c["acc"] else 0))
    _cap32(f"{c['id']} dg", exp["dg"][1], sa + (d["dg_old"].abs() if c["acc"] else 0))


@pytest.mark.parametrize("c", dc.WN_CASES, ids=[c["id"] for c in dc.WN_CASES])
def test_weightnorm_forward_bounds_are_not_vacuous(c):
    exp = dc.wn_fwd_expected(c, dc.wn_inputs(c))
    _cap32(f"{c['id']} inv", exp["inv"][1], exp["inv"][0])
    _cap16(f"{c['id']} w16", *exp["w16"])


def _loss_caps(c, exp, coef):
    nc, B = c["ncrops"], c["B"]
    A = exp["A"]
    f = (A / 32).clamp_min(1)
    p, q = exp["p"][0], exp["q"][0]
    v = (torch.arange(nc * B) // B)[:, None]
    qs = (v != 0) * q[:B].repeat(nc, 1) + (v != 1) * q[B:].repeat(nc, 1)
    nv = (1 + (v >= 2)).double()
    mag = coef * (nv * p + qs)
    # The caps are on relative precision.  v_exp_f32 flushes a result below 2^-126, which puts up to 2^-126 into the bound of p and
    # of each q: an element is capped where that stays below the cap's own 1e-4, i.e. where n_v p + sum q >= 3e4 2^-126 (fp32 and
    # bf16 share the exponent range); below, it is judged (its bound is its own magnitude) but not capped.
    live = (nv * p + qs) >= 3e4 * fb.TINY
    if c["K"] == 1:
        # One class: p = q = 1 and the gradient coef (n_v - n_v) is identically 0, which no 16-bit step measures (the step at 0 is
        # the smallest the format has).  The reference must say 0, and the bound of the bf16 gradient takes the fp32 cap in the
        # 16-bit cap's place, against the same magnitude coef (n_v p + sum q) = 2 n_v coef.  The loss's cap is the one of every case.
        assert bool((exp["grad"][0] == 0).all()) and abs(float(exp["loss"][0])) < 1e-12
        _cap32(f"{c['id']} grad", exp["grad"][1], f * mag)
    elif c["g16"]:
        _cap16(f"{c['id']} grad", exp["grad"][0][live], exp["grad"][1][live])
    else:
        _cap32(f"{c['id']} grad", exp["grad"][1][live], (f * mag)[live])
    mag = (nv * exp["lse_s"][0].abs() + exp["dots"][0].abs()).mean() * nc / (2 * nc - 2)
    _cap32(f"{c['id']} loss", exp["loss"][1], float(f.max()) * mag.reshape(1))


@pytest.mark.parametrize("c", dc.LOSS_CASES, ids=[c["id"] for c in dc.LOSS_CASES])
def test_loss_bounds_are_not_vacuous(c):
    _loss_caps(c, dc.loss_expected(c, dc.loss_inputs(c)), dc.coef_of(c))


@pytest.mark.parametrize("c", dc.HEAD_CASES, ids=[c["id"] for c in dc.HEAD_CASES])
def test_fused_head_loss_bounds_are_not_vacuous(c):
    d = dc.head_inputs(c)
    exp = dc.head_expected(c, d)
    _loss_caps(c, exp, dc.coef_of(c))
    # (the magnitude a column sum is formed from: the 256 products of every teacher logit of the column)
    _cap32(f"{c['id']} colsum", exp["colsum"][1], (d["zt"].abs() @ d["wt"][:c["K"]].abs().t()).sum(0))


def test_colsum_and_ema_bounds_are_not_vacuous():
    for c in dc.COLSUM_CASES:
        x = dc.colsum_inputs(c)["x"]
        _cap32(f"{c['id']} colsum", fb.colsum(x)[1], x.abs().sum(0))
    for c in dc.EMA_CASES:
        d = dc.ema_inputs(c)
        _cap32(f"{c['id']} centre", dc.ema_expected(c, d)[1], d["center"].abs() + d["colsum"].abs() * c["inv_rows"])


def test_every_path_named_in_the_grids_is_in_them():
    ks = {c["K"] for c in dc.LOSS_CASES}
    assert ks == set(dc.LOSS_KS)
    assert any(c["ncrops"] * c["B"] > 1024 for c in dc.LOSS_CASES)                             # loss_final_kernel's second trip
    for k in ("dist", "tt", "dev", "scale", "g16"):
        assert len({c[k] for c in dc.LOSS_CASES}) == {"dist": 6, "tt": 2, "dev": 2, "scale": 3, "g16": 2}[k], k
    assert any(c["dev"] and not c["g16"] and c["scale"] != 1 for c in dc.LOSS_CASES)
    assert {(c["g16"], c["dev"]) for c in dc.LOSS_CASES} == {(a, b) for a in (False, True) for b in (False, True)}
    assert {(c["dist"], c["tt"]) for c in dc.LOSS_CASES} >= {(d, t) for d in ("sharp", "cosine") for t in (0.04, 0.07)}
    for rows in (1, 4, 5, 7):
        assert {(c["acc"], c["dg"]) for c in dc.ROW_CASES if c["rows"] == rows} == {(a, b) for a in (0, 1) for b in (False, True)}, rows
    assert all(c["ldg"] != c["ld"] and c["ld"] in (dc.r4(c["K"]), dc.r4(c["K"]) + 8) for c in dc.LOSS_CASES)
    assert {(c["K"], c["Kpad"]) for c in dc.HEAD_CASES} == set(dc.HEAD_KS)
    assert {(c["ncrops"], c["B"]) for c in dc.HEAD_CASES} == set(dc.HEAD_NB)
    for k, n in (("ops", 3), ("colsum", 2), ("dev", 2), ("scale", 3)):
        assert len({c[k] for c in dc.HEAD_CASES}) == n, k
    assert {c["ldg"] - c["Kpad"] for c in dc.HEAD_CASES} == {0, 8}
    for kind in dc.ROW_KINDS:
        assert any(dc.row_kinds(c) == [kind] for c in dc.ROW_CASES), kind                      # every kind meets a one-row launch


# ------------------------------------------------------------------------------------------------ (b) the semantics tie
def _torch_dino_loss(s, t, center, ncrops, ts, tt):
    """The loss as the training script states it: softmax of the centred, sharpened teacher views; for every teacher view and every
    student crop that is not the same view, the batch mean of the cross-entropy; the mean over those pairs."""
    crops = (s / ts).chunk(ncrops)
    views = torch.softmax((t - center) / tt, dim=-1).detach().chunk(2)
    terms = [(-q * torch.log_softmax(crops[v], dim=-1)).sum(-1).mean() for i, q in enumerate(views) for v in range(ncrops) if v != i]
    return sum(terms) / len(terms)


@pytest.mark.parametrize("cid", ["K1027-5x3-f32-dev-third", "K5-3x2-bigc-f32", "K4100-5x3-sharp-f32"])
def test_the_loss_reference_is_the_double_loop_of_the_training_script(cid):
    c = BY_ID[cid]
    d = dc.loss_inputs(c)
    nc, B = c["ncrops"], c["B"]
    its, itt = fb.inv32(c["ts"]), fb.inv32(c["tt"])
    s = d["s"].clone().requires_grad_(True)
    loss = _torch_dino_loss(s, d["t"], d["center"], nc, 1 / its, 1 / itt)
    loss.backward()
    z = torch.zeros((), dtype=f64)
    exp = fb.dino_loss(d["s"], z, d["t"], z, d["center"], nc, B, (c["ts"], c["tt"]), 1.0, False)           # coef 1: n_terms B tau_s dL/ds
    assert abs(float(exp["loss"][0]) - float(loss)) <= 1e-12 * max(1, abs(float(loss)))
    assert (exp["grad"][0] - s.grad * (2 * nc - 2) * B / its).abs().max() <= 1e-12
    assert (exp["q"][0] - torch.softmax((d["t"] - d["center"]) * itt, -1)).abs().max() <= 1e-12
    assert (exp["p"][0] - torch.softmax(d["s"] * its, -1)).abs().max() <= 1e-12


def test_the_centre_reference_is_update_center():
    """The centre update as the training script states it, on the teacher outputs of 8 ranks with 2 B = 128 rows each: the ranks' row
    sums added up (the all-reduce), divided by rows per rank times ranks, blended with the momentum.  The kernels take the
    all-reduced row sums (`fb.colsum` per rank, as lafs_colsum_f32 and the fused kernel form them) and inv_rows = 1 / (2 B world)."""
    c = BY_ID["K257-B64-world8"]
    world, B, K = 8, 64, c["K"]
    assert c["inv_rows"] == 1.0 / (2 * B * world)
    gen = torch.Generator()
    gen.manual_seed(7)
    ranks = [2 * torch.randn(2 * B, K, generator=gen, dtype=f64) for _ in range(world)]
    center = dc.ema_inputs(c)["center"]
    m = fb.f32c(c["m"])
    batch_center = sum(torch.sum(t, dim=0, keepdim=True) for t in ranks)              # all_reduce(sum over this rank's rows)
    batch_center = batch_center / (len(ranks[0]) * world)
    ref = center[None] * m + batch_center * (1 - m)
    reduced = sum(fb.colsum(t)[0] for t in ranks)
    got = fb.center_ema(center, reduced, c["inv_rows"], c["m"])[0]
    assert (got - ref[0]).abs().max() <= 1e-12


def test_the_row_references_are_normalize_and_weight_norm():
    c = _first(dc.ROW_CASES, lambda x: x["rows"] == 7 and x["D"] == 260)                     # seven rows: every row kind
    d = dc.row_inputs(c)
    x = d["x"].clone().requires_grad_(True)
    y = torch.nn.functional.normalize(x, dim=1, eps=fb.f32c(1e-12))
    y.backward(d["dy"])
    exp = dc.l2_fwd_expected(c, d)
    tiny = torch.tensor([k == "tiny" for k in dc.row_kinds(c)])
    assert bool(tiny.any()) and bool((exp["inv"][0][tiny] == 1 / fb.f32c(1e-12)).all())
    assert (exp["y"][0] - y.detach()).abs().max() <= 1e-12
    dx = dc.l2_bwd_expected(c, d, exp["inv"][0])[0]
    # (below the clamp F.normalize is x / eps, whose gradient is dy / eps; the kernel keeps the projection, as its header states)
    assert ((dx - x.grad)[~tiny].abs() / x.grad[~tiny].abs().clamp_min(1)).max() <= 1e-12
    d = dc.row_inputs(c, weight=True)
    lin = torch.nn.utils.weight_norm(torch.nn.Linear(c["D"], c["rows"], bias=False).double(), dim=0)
    with torch.no_grad():
        lin.weight_v.copy_(d["x"]); lin.weight_g.copy_(d["g"])
    lin(torch.eye(c["D"], dtype=f64)).t().backward(d["dy"])
    fwd = fb.weightnorm_fwd(d["x"], d["g"])
    rel = lambda a, b: ((a - b).abs() / b.abs().clamp_min(1)).max()
    assert rel(fwd["w"][0], torch._weight_norm(d["x"], d["g"], 0)) <= 1e-12
    bwd = fb.weightnorm_bwd(d["dy"], d["x"], d["g"], fwd["inv"][0])
    assert rel(bwd["dv"][0], lin.weight_v.grad) <= 1e-12 and rel(bwd["dg"][0], lin.weight_g.grad) <= 1e-12


def test_the_fused_reference_is_the_unfused_one_on_the_product_of_its_operands():
    c = BY_ID["K65p256-3x5-dev-third"]
    d = dc.head_inputs(c)
    K = c["K"]
    s, t = d["zs"] @ d["ws"][:K].t(), d["zt"] @ d["wt"][:K].t()
    z = torch.zeros((), dtype=f64)
    a = fb.dino_loss(s, z, t, z, d["center"], c["ncrops"], c["B"], (c["ts"], c["tt"]), dc.coef_of(c), False, c["dev"])
    b = dc.head_expected(c, d)
    gb = fb.dino_loss(*dc.head_logits(c, d), d["center"], c["ncrops"], c["B"], (c["ts"], c["tt"]), dc.coef_of(c), False, c["dev"], fused=True)
    assert abs(float(a["loss"][0]) - float(b["loss"][0])) <= 1e-12
    assert (a["grad"][0] - gb["grad"][0]).abs().max() <= 1e-12
    assert torch.equal(fb.rbf(a["grad"][0]), b["grad"][0])
    assert (b["colsum"][0] - t.sum(0)).abs().max() <= 1e-12


# ------------------------------------------------------------------------------------------------ (c) mutations
def _first(cases, pred):
    return next(c for c in cases if pred(c))


ROW_ZERO = _first(dc.ROW_CASES, lambda c: c["rows"] >= 4 and "zero" in dc.row_kinds(c))["id"]
ROW_ACC = _first(dc.ROW_CASES, lambda c: c["rows"] == 7 and c["acc"] and c["D"] == 260)["id"]
FAULTS = [
    ("centre subtracted after the temperature scaling", judge_loss, "K5-3x2-bigc-f32"),
    ("n_v = 1 for the local crops", judge_loss, "K1027-5x3-f32-dev-third"),
    ("q_0 and q_1 swapped for crops 0 and 1", judge_loss, "K1027-5x3-f32-dev-third"),
    ("teacher temperature used for the student", judge_loss, "K1027-5x3-f32-dev-third"),
    ("coef not corrected for the device temperatures", judge_loss, "K1027-5x3-f32-dev-third"),
    ("last class of a ragged tail dropped", judge_loss, "K1027-5x3-f32-dev-third"),
    ("last class block dropped from the log-sum-exp", judge_head, "K65p256-3x5-dev-third"),
    ("the row's maximum not subtracted", judge_loss, "K1003-5x3-offset-bf16"),
    ("pad column counted in the sum", judge_head, "K65p256-3x5-dev-third"),
    ("grad_scale ignored", judge_loss, "K1027-5x3-f32-dev-third"),
    ("column sum over B rows instead of 2 B", judge_head, "K65p256-3x5-dev-third"),
    ("EMA with m and 1 - m exchanged", judge_ema, "K257-B64-world8"),
    ("l2norm clamp missing", judge_rows, ROW_ZERO),
    ("<y, dy> term dropped", judge_rows, ROW_ACC),
    ("weight-norm g missing from dv", judge_rows, ROW_ACC),
    ("accumulate overwrites", judge_rows, ROW_ACC),
    ("last row of a four-row workgroup skipped", judge_rows, ROW_ACC),
]
EMULATED = ([(judge_rows, c["id"]) for c in dc.ROW_CASES] + [(judge_loss, c["id"]) for c in dc.LOSS_CASES]
            + [(judge_head, c["id"]) for c in dc.HEAD_CASES] + [(judge_ema, c["id"]) for c in dc.EMA_CASES])


@pytest.mark.parametrize("judge,cid", EMULATED, ids=[cid for _, cid in EMULATED])
def test_the_emulated_kernels_pass(judge, cid):
    """Every case of the grids, not the fault cases alone."""
    judge(BY_ID[cid])


@pytest.mark.parametrize("c", dc.COLSUM_CASES, ids=[c["id"] for c in dc.COLSUM_CASES])
def test_the_emulated_colsum_passes_and_a_skipped_tail_row_fails(c):
    """colsum_f32_kernel: eight rows at a time into one fp32 accumulator, then the tail rows one by one."""
    x = dc.colsum_inputs(c)["x"]
    rows = c["rows"]

    def emulate(n):
        a = torch.zeros(c["K"], dtype=f32)
        for r in range(n):
            a = a + x[r].float()
        return a

    fb.check(f"colsum {c['id']}", emulate(rows), *fb.colsum(x))
    if rows % 8:                                         # (the tail loop dropped: the rows past the last full eight)
        with pytest.raises(AssertionError):
            fb.check(f"colsum {c['id']}", emulate(rows // 8 * 8), *fb.colsum(x))


@pytest.mark.parametrize("c", dc.WN_CASES, ids=[c["id"] for c in dc.WN_CASES])
def test_the_emulated_weightnorm_forward_passes(c):
    d = dc.wn_inputs(c)
    inv, w16 = emulate_wn_fwd(c, d)
    exp = dc.wn_fwd_expected(c, d)
    fb.check(f"{c['id']}: inv_norm", inv, *exp["inv"])
    fb.check(f"{c['id']}: w", w16, *exp["w16"], True)


@pytest.mark.parametrize("fault,judge,cid", FAULTS, ids=[f[0] for f in FAULTS])
def test_a_seeded_fault_fails(fault, judge, cid):
    with pytest.raises(AssertionError):
        judge(BY_ID[cid], fault)
    print(f"rejected: {fault} ({cid})")
