"""The case grid and the fp64 reference of lafs_softmax_ce_rank (csrc/linear_probe.hip), shared by tests/test_oracle_linear_host.py and
tests/test_gpu_linear_probe.py so that the CPU module judges exactly what the GPU runs.

Reference, for a row with 0 <= y < C (z: the row's logits, exactly representable fp32 values widened):
    loss = logsumexp(z) - z_y;   rank = #{j : z_j > z_y or (z_j == z_y and j < y)};   dlogits_j = grad_scale (softmax(z)_j - [j == y])
y == -1: loss 0, rank -1, a zero gradient row.  Any other label outside [0, C): loss NaN, rank -2, a zero gradient row.  The pad columns
[C, lddl) of the gradient are zero.

Bounds (tests/fp64_bounds.py's model): the log-sum-exp carries `lse_rows`' bound with the kernel's tree -- an exponential reaches the
row's sum through 4 of them (its own, thread -> wave, wave -> workgroup, chunk -> row) and through N_ROUND + chunks roundings of the
positive sum (a thread adds its 18 columns, a 6-step butterfly, four waves, the chunks, the rescaling products); the loss adds the
rounding of its subtraction.  A gradient element carries exp(z - lse) with that error propagated (`_exp_minus`), the roundings of the
subtraction and of the product with grad_scale, and half a bf16 step of the value; the reference is the unrounded fp64 value.  The rank
has no bound: comparisons of fp32 values do not round."""
import math

import torch

import fp64_bounds as fb
from fp64_bounds import U, f32, f64
from gemm_cases import seed_of

CHUNK = 4096                                             # LP_CHUNK: columns per (row, chunk) workgroup
N_EXP = 4
N_ROUND = 18 + 6 + 4 + 6
DISTS = ("normal", "pm80", "equal", "ties", "peaked", "wide")
BS, CS = (1, 3, 64), (2, 5, 37, 1000, 4097)
SENTINEL = -12345.0                                      # guard rows and columns (bf16(-12345) = -12352 in the gradient buffer)


def _cases():
    out = []
    for bi, B in enumerate(BS):
        for C in CS:
            for di, dist in enumerate(DISTS):
                for li, extra_ld in enumerate((0, 3)):      # every B x C x distribution x ld; the two lddl alternate over them
                    lddl = (C + 7) // 8 * 8 + 16 * ((bi + di + li) % 2)
                    out.append(dict(id=f"B{B}-C{C}-ld+{extra_ld}-lddl{lddl}-{dist}", B=B, C=C, ld=C + extra_ld, lddl=lddl, dist=dist,
                                    variant=li, fixed_scale=(di + li) % 2 == 1))
    return out


CASES = _cases()


def labels(c, gen):
    """Targets at column 0 and at column C - 1, a row without target and a row whose label is none, where the case has the rows."""
    B, C = c["B"], c["C"]
    y = torch.randint(0, C, (B,), generator=gen, dtype=torch.int64)
    if B == 1:
        y[0] = 0 if c["variant"] == 0 else C - 1
    elif B == 3:
        y[0], y[1], y[2] = 0, C - 1, (-1 if c["variant"] == 0 else C)
    else:
        y[0], y[1], y[5], y[9], y[11], y[63] = 0, C - 1, -1, C, -7, C + 1000
    return y


def inputs(c):
    """{"z": fp64 [B, C] of exactly representable fp32 values, "y": int64 [B], "gs": the fp32 grad_scale as a float}."""
    gen = torch.Generator()
    gen.manual_seed(seed_of("linear", c["id"]))
    B, C, dist = c["B"], c["C"], c["dist"]
    y = labels(c, gen)
    yc = y.clamp(0, C - 1)
    rn = torch.randn(B, C, generator=gen, dtype=f64)
    rows = torch.arange(B)
    if dist == "normal":
        z = 3 * rn
    elif dist == "pm80":                                 # no overflow with the maximum subtracted; exp(-160) flushes to zero
        z = 80 * torch.sign(rn) + 0.5 * torch.randn(B, C, generator=gen, dtype=f64)
    elif dist == "equal":                                # every column ties with the target: rank = y
        z = torch.full((B, C), 1.25, dtype=f64)
    elif dist == "ties":                                 # a coarse lattice, and exact ties on both sides of the target
        z = torch.round(2 * rn) / 2
        zy = z[rows, yc]
        z[rows, (yc - 1).clamp_min(0)] = zy
        z[rows, (yc + 1).clamp_max(C - 1)] = zy
    elif dist == "peaked":                               # one dominant column: the target on even rows, another on odd rows
        z = rn.clone()
        peak = torch.where(rows % 2 == 0, yc, (yc + 1 + C // 2) % C)
        z[rows, peak] += 30
    elif dist == "wide":                                 # exp(max) overflows fp32 unless the maximum is subtracted
        z = 40 * rn
    else:
        raise ValueError(dist)
    n_t = int(((y >= 0) & (y < C)).sum())
    gs = 0.37 if c["fixed_scale"] else 1.0 / max(n_t, 1)
    return {"z": z.to(f32).double(), "y": y, "gs": float(torch.tensor(gs, dtype=f32))}


def rank_of(z, y):
    """The stated rule, on the rows that have a target (others: -1 for y == -1, else -2)."""
    B, C = z.shape
    has = (y >= 0) & (y < C)
    yc = y.clamp(0, C - 1)
    zy = z.gather(1, yc[:, None])
    cols = torch.arange(C, device=z.device)[None]
    before = ((z > zy) | ((z == zy) & (cols < yc[:, None]))).sum(1)
    return torch.where(has, before, torch.where(y == -1, torch.full_like(y, -1), torch.full_like(y, -2)))


def reference(c, d):
    """{"loss": (ref [B], bound), "rank": int64 [B], "dl": (ref [B, lddl], bound), "has": bool [B], "p": softmax} in fp64."""
    z, y, gs = d["z"], d["y"], d["gs"]
    B, C = z.shape
    has = (y >= 0) & (y < C)
    yc = y.clamp(0, C - 1)
    n_round = N_ROUND + math.ceil(C / CHUNK)
    L, Le, _ = fb.lse_rows(z, torch.zeros_like(z), 1.0, n_exp=N_EXP, n_round=n_round)
    zy = z.gather(1, yc[:, None])
    loss = (L - zy)[:, 0]
    loss_e = Le[:, 0] + 2 * U * loss.abs() + fb.TINY
    nan = torch.full_like(loss, float("nan"))
    loss = torch.where(has, loss, torch.where(y == -1, torch.zeros_like(loss), nan))
    loss_e = torch.where(has, loss_e, torch.zeros_like(loss_e))
    p, pe = fb._exp_minus(z, 0.0, L, Le)
    oh = torch.zeros_like(z)
    oh[torch.arange(B), yc] = 1.0
    diff = p - oh
    g = gs * diff
    ge = gs * (pe + U * diff.abs()) + U * g.abs()
    ge = ge + 0.5 * fb.step16(g.abs() + ge) + fb.TINY
    live = has[:, None].expand_as(g)
    z0 = torch.zeros_like(g)
    dl = torch.zeros(B, c["lddl"], dtype=f64)
    dle = torch.zeros(B, c["lddl"], dtype=f64)
    dl[:, :C], dle[:, :C] = torch.where(live, g, z0), torch.where(live, ge, z0)
    return {"loss": (loss, loss_e), "rank": rank_of(z, y), "dl": (dl, dle), "has": has, "p": p, "raw_ge": gs * (pe + U * diff.abs()) + U * g.abs()}


def judge(c, d, loss, rank, dl, exp=None):
    """A kernel's (or an emulation's) outputs of case c against the reference: the rank exactly, the loss and the gradient inside their
    bounds; rows without a target as the conventions say.  dl: [B, lddl] or None."""
    exp = reference(c, d) if exp is None else exp
    name = c["id"]
    rank, ref_rank = rank.long().cpu(), exp["rank"]
    assert torch.equal(rank, ref_rank), f"{name}: row_rank {rank.tolist()[:16]}, expected {ref_rank.tolist()[:16]}"
    loss = loss.double().cpu()
    ref, bound = exp["loss"]
    bad = torch.isnan(ref)
    assert bool(torch.isnan(loss[bad]).all()), f"{name}: a label outside [0, C) that is not -1 must give loss NaN"
    ok = ~bad
    worst = [fb.check(f"{name}: row_loss", loss[ok], ref[ok], bound[ok])[0]]
    if dl is not None:
        worst.append(fb.check(f"{name}: dlogits", dl.double().cpu(), *exp["dl"])[0])
    return max(worst)
