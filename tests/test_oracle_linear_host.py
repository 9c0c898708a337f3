"""What makes the kernel test of tests/test_gpu_linear_probe.py trustworthy without a GPU (tests/linear_cases.py is its grid and its
fp64 reference).

(a) Semantics tie: on the tie-free cases the reference equals torch.nn.functional.cross_entropy(reduction='none') in float64, its
    autograd gradient, and a rank derived from torch.topk; on the cases with ties it equals the stated tie rule, counted column by
    column in plain Python.
(b) Non-vacuity caps on the bounds, over every case of the grid, so that passing inside a bound means something.  Measured on the
    grid on a CPU (the largest figure over all cases) and asserted with a 2x margin:
        row_loss   bound / max(1, |lse|, |z_y|)                       measured 6.67e-6  -> cap 1.4e-5
        dlogits    bound before the bf16 half step / (grad_scale (softmax_j + [j == y])), over the elements where that magnitude is
                   at least 1e-30 (below it a flushed exponential alone is the whole value)
                                                                      measured 6.90e-5  -> cap 1.4e-4
        dlogits    the whole bound / one bf16 step of that magnitude, same elements
                                                                      measured 1.014    -> cap 2.03
                   (half a step, taken one binade up where the value plus its error crosses a power of two)
(c) Mutation self-test: an fp32 CPU emulation of the kernel (its formulas and number domains; torch's summation order) passes the
    oracle on every case, and each of the seeded faults fails it on at least one case of the grid."""
import pytest
import torch
import torch.nn.functional as tF

import fp64_bounds as fb
import linear_cases as lc
from fp64_bounds import bf16, f32, f64

TIE_FREE = ("normal", "peaked", "wide")
CAP_LOSS, CAP_GRAD32, CAP_GRAD16 = 1.4e-5, 1.4e-4, 2.03
_CACHE = {}


def case_data(c):
    if c["id"] not in _CACHE:
        d = lc.inputs(c)
        _CACHE[c["id"]] = (d, lc.reference(c, d))
    return _CACHE[c["id"]]


# ------------------------------------------------------------------------------------------------ (a) semantics
@pytest.mark.parametrize("c", [c for c in lc.CASES if c["dist"] in TIE_FREE], ids=lambda c: c["id"])
def test_reference_is_torch_cross_entropy_on_tie_free_cases(c):
    d, exp = case_data(c)
    z, y, gs = d["z"], d["y"], d["gs"]
    C = c["C"]
    has = exp["has"]
    assert bool(has.any())
    zt = z[has].clone().requires_grad_(True)
    yt = y[has]
    free = (zt.detach() == zt.detach().gather(1, yt[:, None])).sum(1) == 1     # (4097 fp32 draws of a row may collide; the target's must not)
    assert bool(free.any()), "the case is meant to have targets without ties"
    ce = tF.cross_entropy(zt, yt, reduction="none")
    (gs * ce.sum()).backward()
    assert torch.allclose(exp["loss"][0][has], ce.detach(), rtol=1e-12, atol=1e-12)
    # (softmax - 1 at a dominant target cancels in fp64 itself: the softmax's own error, C x 1.1e-16 at most, stays absolute)
    assert torch.allclose(exp["dl"][0][has][:, :C], zt.grad, rtol=1e-12, atol=1e-12)
    order = torch.topk(zt.detach(), C, dim=1).indices                       # descending; the target's place is unique without ties
    topk_rank = (order == yt[:, None]).int().argmax(1)
    assert torch.equal(exp["rank"][has][free], topk_rank[free])
    assert bool((exp["dl"][0][:, C:] == 0).all()) and bool((exp["dl"][1][:, C:] == 0).all())


@pytest.mark.parametrize("c", [c for c in lc.CASES if c["dist"] in ("equal", "ties", "pm80")], ids=lambda c: c["id"])
def test_reference_rank_is_the_stated_tie_rule(c):
    d, exp = case_data(c)
    z, y = d["z"], d["y"]
    C = c["C"]
    tied = 0
    for b in range(c["B"]):
        yb = int(y[b])
        if yb == -1:
            want = -1
        elif not 0 <= yb < C:
            want = -2
        else:
            row, zy = z[b].tolist(), float(z[b, yb])
            want = sum(1 for j, v in enumerate(row) if v > zy or (v == zy and j < yb))
            tied += sum(1 for j, v in enumerate(row) if v == zy and j != yb)
        assert int(exp["rank"][b]) == want, (c["id"], b)
    if c["dist"] != "pm80" and bool(exp["has"].any()):
        assert tied > 0, "the case is meant to have ties at the target"
    if c["dist"] == "equal":
        assert torch.equal(exp["rank"][exp["has"]], y[exp["has"]])


def test_conventions_of_rows_without_a_target():
    c = next(c for c in lc.CASES if c["B"] == 64)
    d, exp = case_data(c)
    y = d["y"]
    assert int(y[5]) == -1 and float(exp["loss"][0][5]) == 0.0 and int(exp["rank"][5]) == -1
    for b in (9, 11, 63):
        assert torch.isnan(exp["loss"][0][b]) and int(exp["rank"][b]) == -2
    for b in (5, 9, 11, 63):
        assert bool((exp["dl"][0][b] == 0).all()) and bool((exp["dl"][1][b] == 0).all())
    assert int(y[0]) == 0 and int(y[1]) == c["C"] - 1


# ------------------------------------------------------------------------------------------------ (b) caps
def _figures(c):
    d, exp = case_data(c)
    z, y, gs = d["z"], d["y"], d["gs"]
    C, has = c["C"], exp["has"]
    if not bool(has.any()):
        return 0.0, 0.0, 0.0
    yc = y.clamp(0, C - 1)
    L = torch.logsumexp(z, 1)
    zy = z.gather(1, yc[:, None])[:, 0]
    scale = torch.maximum(torch.maximum(L.abs(), zy.abs()), torch.ones_like(L))
    f_loss = float((exp["loss"][1] / scale)[has].max())
    oh = torch.zeros_like(z)
    oh[torch.arange(c["B"]), yc] = 1.0
    mag = gs * (exp["p"] + oh)
    sel = has[:, None] & (mag >= 1e-30)
    f32_part = float((exp["raw_ge"] / mag)[sel].max())
    ref, bound = exp["dl"]
    f16_part = float((bound[:, :C] / fb.step16(mag))[sel].max())
    return f_loss, f32_part, f16_part


def test_bounds_are_capped():
    figs = [_figures(c) for c in lc.CASES]
    worst = [max(f[i] for f in figs) for i in range(3)]
    print(f"\nlargest bound figures over {len(lc.CASES)} cases: loss {worst[0]:.3g}, gradient fp32 part {worst[1]:.3g}, "
          f"gradient in bf16 steps {worst[2]:.3g}")
    assert worst[0] <= CAP_LOSS and worst[1] <= CAP_GRAD32 and worst[2] <= CAP_GRAD16, worst


# ------------------------------------------------------------------------------------------------ (c) emulation and seeded faults
FAULTS = ["the maximum not subtracted", "the target column left out of the sum", "rank with >= for >", "tie rule reversed",
          "one-hot off by one column", "grad_scale dropped", "pad columns not zeroed", "ld used for lddl", "a -1 row contributing",
          "the last chunk skipped", "a bad label treated as -1", "loss without the target logit"]


def emulate(c, d, fault=None):
    """lafs_softmax_ce_rank in fp32 on the CPU -> (row_loss f32 [B], row_rank i64 [B], dlogits bf16 [B, lddl]); the gradient buffer
    starts as NaN, so whatever is not written shows."""
    z, y = d["z"].float(), d["y"]
    B, C, ld, lddl = c["B"], c["C"], c["ld"], c["lddl"]
    gs = torch.tensor(1.0 if fault == "grad_scale dropped" else d["gs"], dtype=f32)
    has = (y >= 0) & (y < C)
    yc = y.clamp(0, C - 1)
    rows, cols = torch.arange(B), torch.arange(C)[None]
    zy = z.gather(1, yc[:, None])
    cut = C
    if fault == "the last chunk skipped":                # the last of several chunks, or the scalar tail of the only one
        cut = (C - 1) // lc.CHUNK * lc.CHUNK if C > lc.CHUNK else (C - 1) // 4 * 4 if C > 4 else C
    use = cols < cut
    m = torch.zeros(B, 1) if fault == "the maximum not subtracted" else torch.where(use, z, torch.tensor(-float("inf"))).max(1, keepdim=True).values
    e = torch.exp(z - m) * use
    if fault == "the target column left out of the sum":
        e[rows, yc] = 0
    lse = m + torch.log(e.sum(1, keepdim=True))
    loss = (lse if fault == "loss without the target logit" else lse - zy)[:, 0]
    if fault == "rank with >= for >":
        before = (z >= zy) & (cols != yc[:, None])
    elif fault == "tie rule reversed":
        before = (z > zy) | ((z == zy) & (cols > yc[:, None]))
    else:
        before = (z > zy) | ((z == zy) & (cols < yc[:, None]))
    rank = before.sum(1)
    none = (y == -1) | (~has if fault == "a bad label treated as -1" else torch.zeros_like(has))
    loss = torch.where(has, loss, torch.where(none, torch.zeros_like(loss), torch.full_like(loss, float("nan"))))
    rank = torch.where(has, rank, torch.where(none, torch.full_like(rank, -1), torch.full_like(rank, -2)))
    hot = torch.zeros(B, C)
    hot[rows, (yc + 1) % C if fault == "one-hot off by one column" else yc] = 1.0
    g = gs * (torch.exp(z - lse) - hot)
    live = has | ((y == -1) if fault == "a -1 row contributing" else torch.zeros_like(has))
    g = torch.where(live[:, None], g, torch.zeros_like(g)).to(bf16)
    stride = ld if fault == "ld used for lddl" else lddl
    buf = torch.full((B * max(ld, lddl) + lddl,), float("nan"), dtype=bf16)
    for b in range(B):
        buf[b * stride:b * stride + cut] = g[b, :cut]
        if fault != "pad columns not zeroed":
            buf[b * stride + C:b * stride + lddl] = 0
    return loss, rank, buf[:B * lddl].view(B, lddl)


@pytest.mark.parametrize("c", lc.CASES, ids=lambda c: c["id"])
def test_emulated_kernel_passes_the_oracle(c):
    d, exp = case_data(c)
    worst = lc.judge(c, d, *emulate(c, d), exp=exp)
    assert worst <= 1.0


@pytest.mark.parametrize("fault", FAULTS)
def test_seeded_fault_fails_the_oracle(fault):
    caught = []
    for c in lc.CASES:
        d, exp = case_data(c)
        try:
            lc.judge(c, d, *emulate(c, d, fault), exp=exp)
        except AssertionError:
            caught.append(c["id"])
    print(f"\n'{fault}' fails {len(caught)} of {len(lc.CASES)} cases")
    assert caught, f"no case of the grid notices '{fault}'"


def test_the_oracle_passes_its_own_reference():
    c = lc.CASES[0]
    d, exp = case_data(c)
    lc.judge(c, d, exp["loss"][0].to(f32), exp["rank"], exp["dl"][0].to(f32).to(bf16), exp=exp)
