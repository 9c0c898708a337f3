"""The case grid of tests/test_gpu_koleo.py (csrc/koleo.hip), its seeded inputs, the fp64 oracle of the KoLeo regulariser with its
per-element bounds, and the judge both test modules use.  Kept apart from the GPU module so that tests/test_koleo_host.py judges on
the CPU exactly the cases the GPU runs.  The definition is the one of include/lafs_hip.h (lafs_koleo_fwd_bwd).

The kernel pair, as far as the bounds need it: a wave holds a row, a lane the float4 pieces lane + 64 t of it (t < NV = ceil(D / 256));
the lane adds its <= 4 NV products as one chain of fma, a 6-step butterfly follows: a term of a sum over D passes through at most
depth(D) = 4 NV + 6 additions, each rounding once.  The search runs one workgroup of four waves per row: wave w scores the candidate
quads w, w + 4, ... (4 rows per wave and trip, TILE = 16 per workgroup and trip) and wave 0 picks among the four waves' winners; the
gradient pass runs one wave per row, 4 rows per workgroup.

Paths by shape:
  rows  2, 3       wave 0 alone has candidates, a partial quad (its surplus slots re-read the last row and are masked); one partial
                   workgroup of the gradient pass
        4, 5       one full quad; a second wave with one candidate, a one-row second workgroup of the gradient pass
        15, 16, 17 one tile less one, one tile, one tile + 1 (wave 0's second trip, of one candidate)
        34         two tiles + 2
        256        four trips per wave; four trips of the 64-entry scan of the neighbour list in the gather; 4 rows per lane in the loss fold
  D     4          one live lane
        64         16 live lanes
        252/256/260  the first piece per lane short by one lane, full, and the second piece (NV 1 -> 2) in lane 0 alone
        384, 768, 1024   NV 2, 3, 4 (the trunk widths of vit_small and of mynet / fvit; the largest D)
  n_groups 1, 2, 3; ldx / lddx equal to D and D + 4 / D + 8; accumulate 0 / 1 on a non-zero old dx; dx and nn NULL."""
import math

import torch

import fp64_bounds as fb
from fp64_bounds import LOG_REL, U, ULP1, f32, f64
from gemm_cases import seed_of

rf = lambda v: v.to(f32).double()
EPS = fb.f32c(1e-8)                 # the operand the kernel holds for eps = 1e-8
TILE = 16
KINDS = ("normal", "small", "large", "tiny", "zero", "outlier", "neardup", "dup")
BASE_KINDS = ("normal", "small", "large", "outlier")           # what a (near-)duplicate may copy
SCALES = (1.0, 0.1, 3.0)                                       # grad_scale


def depth(D):
    return 4 * -(-D // 256) + 6


def _gen(*key):
    g = torch.Generator()
    g.manual_seed(seed_of("koleo", *key))
    return g


# ------------------------------------------------------------------------------------------------ the grid
def case(cid, rows, D, G, n, **kw):
    c = dict(id=cid, rows=rows, D=D, G=G, mix="normal" if n % 2 == 0 else "mixed", rot=n, acc=(n // 2) % 2 == 1, ldx=D + 4 * ((n // 3) % 2),
             lddx=D + 8 * ((n // 4) % 2), scale=SCALES[n % 3], dx=True, nn=True, tie=False)
    c.update(kw)
    return c


def _grid():
    g = []
    n = 0
    rows_all = (2, 3, 4, 5, TILE - 1, TILE, TILE + 1, 2 * TILE + 2, 256)
    for i, D in enumerate((4, 64, 252, 256, 260, 384, 768, 1024)):
        for k in (0, 2, 4, 7):                                 # four of the nine row counts per D, every count at three or four D
            rows = rows_all[(2 * i + k) % 9]
            G = 1 + (n + n // 3) % 3
            g.append(case(f"{rows}x{D}-g{G}-{n}", rows, D, G, n))
            n += 1
    # the step's own shape; forward only / no neighbour output; forms the rotation does not pair
    g.append(case("64x384-g2-step", 64, 384, 2, 0, mix="normal", acc=True, scale=0.1, ldx=384, lddx=384))
    g.append(case("17x260-g2-fwd-only", 17, 260, 2, 1, dx=False))
    g.append(case("5x64-g3-no-nn", 5, 64, 3, 2, nn=False, acc=True))
    g.append(case("3x4-g1-fwd-only-no-nn", 3, 4, 1, 3, dx=False, nn=False))
    g.append(case("256x1024-g1-mixed-acc", 256, 1024, 1, 5, acc=True, ldx=1028, lddx=1032))
    g.append(case("256x4-g2-normal", 256, 4, 2, 6))
    # exact ties by construction (tie_inputs): every dot product exact, the lowest index must win bit for bit
    g.append(case("tie-10x64-g1", 10, 64, 1, 0, tie=True, mix="tie"))
    g.append(case("tie-5x4-g2", 5, 4, 2, 4, tie=True, mix="tie"))
    g.append(case("tie-256x260-g2", 256, 260, 2, 3, tie=True, mix="tie"))
    g.append(case("tie-70x1024-g3", 70, 1024, 3, 2, tie=True, mix="tie"))
    ids = [c["id"] for c in g]
    assert len(set(ids)) == len(ids)
    return g


CASES = _grid()
BY_ID = {c["id"]: c for c in CASES}


# ------------------------------------------------------------------------------------------------ inputs
def row_kinds(c):
    """[G][rows] kinds: all normal, or the eight kinds rotating with the case index, the group and the row."""
    if c["mix"] != "mixed":
        return [["normal"] * c["rows"] for _ in range(c["G"])]
    return [[KINDS[(c["rot"] + 3 * g + r) % len(KINDS)] for r in range(c["rows"])] for g in range(c["G"])]


def tie_inputs(c):
    """Rows with entries in {0, +-1} and four non-zeros: norm 2, xh = +-0.5, every product and every sum exact in fp32.  One pattern
    sits at three (rows >= 5: four) spaced indices, a second one at two, the rest are random patterns -- at D = 4 there are only 16, so
    every row has exact ties."""
    gen = _gen("tie", c["id"])
    G, n, D = c["G"], c["rows"], c["D"]
    x = torch.zeros(G * n, D, dtype=f64)
    for r in range(G * n):
        cols = torch.randperm(D, generator=gen)[:4]
        x[r, cols] = (2 * torch.randint(0, 2, (4,), generator=gen) - 1).double()
    for g in range(G):
        a = sorted({1, n // 2, n - 1} | ({n // 4} if n >= 5 else set()))
        for r in a[1:]:
            x[g * n + r] = x[g * n + a[0]]
        if n >= 10:
            x[g * n + n - 3] = x[g * n + 2]
    return x


def inputs(c):
    """x [G rows, D] and the old dx as fp64 tensors of fp32 values.  Group g > 0 is group 0 displaced by 1e-3 per element: the closest
    row of all lies across the group boundary.  Kinds: normal; scaled by 1e-3 / 1e4; norm 1e-10 (below eps: x / eps, gradient g / eps);
    all zero; one element 1e4; a near-duplicate of an earlier row at distance 1e-3 on the sphere; an exact duplicate."""
    gen = _gen("x", c["id"])
    G, n, D = c["G"], c["rows"], c["D"]
    rn = lambda *s: torch.randn(*s, generator=gen, dtype=f64)
    if c["tie"]:
        x = tie_inputs(c)
    else:
        base = rn(n, D)
        x = torch.cat([base if g == 0 else base + 1e-3 * rn(n, D) for g in range(G)])
        kinds = row_kinds(c)
        for g in range(G):
            for r, k in enumerate(kinds[g]):
                row = x[g * n + r]
                if k == "small":
                    row *= 1e-3
                elif k == "large":
                    row *= 1e4
                elif k == "tiny":
                    row *= 1e-10 / row.norm()
                elif k == "zero":
                    row.zero_()
                elif k == "outlier":
                    row[(3 * r + 1) % D] = 1e4
            for r, k in enumerate(kinds[g]):
                if k in ("neardup", "dup"):
                    p = next((q % n for q in range(r - 1, r - n, -1) if kinds[g][q % n] in BASE_KINDS), None)
                    if p is None:                                  # (a group without a row to copy: the row stays normal)
                        continue
                    src = x[g * n + p]
                    x[g * n + r] = src if k == "dup" else src + 1e-3 * src.norm() * torch.nn.functional.normalize(rn(D), dim=0)
    return dict(x=rf(x), dx_old=rf(rn(G * n, D)))


# ------------------------------------------------------------------------------------------------ the oracle
def _norms(x, eps):
    """||x||, inv = 1 / max(||x||, eps) and the bound of the kernel's inv: the sum of squares (same-sign terms, depth additions and one
    product rounding) as an interval through the root (1 ulp), the clamp (both ends clamped) and the division (1 ulp)."""
    ss = (x * x).sum(1, keepdim=True)
    sse = (depth(x.shape[1]) + 1) * U * ss
    n = ss.sqrt()
    ne = torch.maximum((ss + sse).sqrt() - n, n - (ss - sse).clamp_min(0).sqrt()) + ULP1 * n
    d, lo, hi = n.clamp_min(eps), (n - ne).clamp_min(eps), (n + ne).clamp_min(eps)
    inv = 1 / d
    return n, inv, torch.maximum(1 / lo - inv, inv - 1 / hi) + ULP1 * inv


def _targets(nn, G, rows):
    """Global row index of every row's neighbour (nn: index inside the group)."""
    base = (torch.arange(G * rows, device=nn.device) // rows) * rows
    return base + nn.long()


def reference(x, G, rows, nn, eps=EPS, grad_scale=1.0, dx_old=None):
    """The definition in fp64 for the neighbour vector nn (group-local indices, [G rows]): {"loss": (L [G], bound), "dx": (grad_scale
    dL/dx (+ dx_old), bound), "parts": the intermediate values the caps of tests/test_koleo_host.py are stated in}.  x, dx_old: fp64
    tensors of fp32 values.  Every line carries the bound of the kernel's fp32 value beside the value:
      xh   = x inv                     one product; inv from _norms
      v    = (xh_i - xh_I) + eps       both operands uncertain, two roundings; EXACTLY eps where rows i and I are identical (their xh
                                       are then the same bits, the difference is 0): the bound is 0 there, which is what keeps d =
                                       eps sqrt(D) meaningful for duplicates
      d    = ||v||                     | ||v'|| - ||v|| | <= ||v' - v||; sum of squares of depth + 1 roundings, halved by the root; 1 ulp
      lg   = log(d + eps)              the sum rounds; the interval through log exactly; logf LOG_REL
      L    = -sum lg / rows            a lane adds ceil(rows / 64) terms, 6-step butterfly; division 1 ulp
      coef = -1 / (rows (d (d + eps))) three products / sums round, the interval through the reciprocal exactly (infinite where it
                                       reaches 0), division 1 ulp -- THIS is the amplification 1 / (d (d + eps)) of the error of v
      c    = v coef                    one product
      g_j  = c_j - sum c_i             cnt subtractions, each rounding a partial sum that is at most sum |terms|
      s    = <xh_j, g_j>               both uncertain, depth + 1 roundings of sum |terms|
      dx   = (g - xh s) inv            (y s and the difference round, the product with inv rounds);  g inv where ||x|| < eps
      out  = old + grad_scale dx       one rounding each"""
    D = x.shape[1]
    dep = depth(D)
    nrm, inv, inve = _norms(x, eps)
    xh = x * inv
    xhe = x.abs() * inve + U * xh.abs()
    J = _targets(nn, G, rows)
    same = (x == x[J]).all(1, keepdim=True)
    diff = xh - xh[J]
    v = diff + eps
    ve = torch.where(same, torch.zeros_like(v), xhe + xhe[J] + U * diff.abs() + U * v.abs())
    d = (v * v).sum(1, keepdim=True).sqrt()
    ven = (ve * ve).sum(1, keepdim=True).sqrt()
    de = ven + ((dep + 2) / 2 * U + ULP1) * (d + ven)
    t = d + eps
    te = de + U * t
    lg = t.log()
    inf = torch.full_like(t, float("inf"))
    lge = torch.where(te < t, -torch.log1p(-(te / t).clamp_max(1 - 1e-16)), inf) + LOG_REL * lg.abs()
    dep_r = -(-rows // 64) + 6
    lgG, lgeG = lg.view(G, rows), lge.view(G, rows)
    L = -lgG.sum(1) / rows
    Le = lgeG.sum(1) / rows + dep_r * U * lgG.abs().sum(1) / rows + ULP1 * L.abs()
    p = d * t
    pe = de * t + d * te + de * te + U * p
    m = rows * p
    me = rows * pe + U * m
    coef = -1 / m
    lo = m - me
    coefe = torch.where(lo > 0, 1 / lo.clamp_min(1e-300) - 1 / m, inf) + ULP1 * (1 / lo.clamp_min(1e-300)).abs()
    c = v * coef
    ce = ve * coef.abs() + v.abs() * coefe + ve * coefe + U * c.abs()
    ce = torch.where(torch.isfinite(ce), ce, inf.expand_as(ce))            # (0 * inf)
    gather = lambda a: torch.zeros_like(a).index_add_(0, J, a)
    cnt = torch.zeros(G * rows, 1, dtype=f64, device=x.device).index_add_(0, J, torch.ones(G * rows, 1, dtype=f64, device=x.device))
    g = c - gather(c)
    ca = c.abs() + gather(c.abs())
    ge = ce + gather(ce) + cnt * U * ca
    tm = xh * g
    s = tm.sum(1, keepdim=True)
    se = (xhe * g.abs() + xh.abs() * ge + xhe * ge).sum(1, keepdim=True) + (dep + 1) * U * ((xh.abs() + xhe) * (g.abs() + ge)).sum(1, keepdim=True)
    ys = xh * s
    inner = g - ys
    ie = ge + xhe * s.abs() + (xh.abs() + xhe) * se + U * ys.abs() + U * (g.abs() + ys.abs())
    tiny = nrm < eps
    inner, ie = torch.where(tiny, g, inner), torch.where(tiny, ge, ie)
    o = inner * inv
    oe = inv * ie + inve * (inner.abs() + ie) + U * o.abs()
    gs = fb.f32c(grad_scale)
    r = gs * o
    re = abs(gs) * oe + U * r.abs()
    if dx_old is not None:
        r = dx_old + r
        re = re + U * r.abs()
    re = torch.where(torch.isfinite(re), re, inf.expand_as(re))
    return {"loss": (L, Le), "dx": (r, re), "parts": dict(xh=xh, inv=inv, J=J, d=d, lg=lg, coef=coef, cnt=cnt, gs=gs)}


def dots_and_gap(x, G, rows, eps=EPS):
    """Per group, in fp64: dots [G, rows, rows] of the normalised rows with the diagonal at -inf (a row is never its own candidate), and
    gap [G, rows, 1] = 2 (4 sqrt(D) + 8) U max_j sum_k |xh_ik xh_jk|, twice the bound of one fp32 dot product of normalised rows.
    The kernel ranks row i's candidates by fl(<x_i, x_j>) fl(inv_j) = ||x_i|| dots (1 + e): the sum is off by at most (depth + 1) U
    sum |terms|, inv_j by ((depth + 1) / 2 + 4) U relative and the product by U, in units of the dots at most (1.5 depth + 6.5) U
    sum_k |xh_ik xh_jk| -- 12.5 of the 16 U this form allows at D = 4, 39.5 of 136 at D = 1024 -- so the form bounds the kernel."""
    D = x.shape[1]
    _, inv, _ = _norms(x, eps)
    xh = (x * inv).view(G, rows, D)
    dots = xh @ xh.transpose(1, 2)
    absd = xh.abs() @ xh.abs().transpose(1, 2)
    eye = torch.eye(rows, dtype=torch.bool, device=x.device)
    dots = dots.masked_fill(eye, float("-inf"))
    absd = absd.masked_fill(eye, 0.0)
    gap = 2 * (4 * math.sqrt(D) + 8) * U * absd.max(2, keepdim=True).values
    return dots, gap


def admissible(x, G, rows, eps=EPS):
    """[G, rows, rows] bool: the neighbours a correct fp32 search may choose for every row."""
    dots, gap = dots_and_gap(x, G, rows, eps)
    return dots >= dots.max(2, keepdim=True).values - gap


def lowest_argmax(dots):
    """argmax over the last axis, the lowest index among exactly equal values."""
    idx = torch.arange(dots.shape[-1], device=dots.device).expand_as(dots)
    return torch.where(dots == dots.max(-1, keepdim=True).values, idx, dots.shape[-1]).min(-1).values


def expected_nn(c, d):
    """The neighbour vector an exact search gives: what the tie cases demand bit for bit (their dot products are exact in fp32)."""
    dots, _ = dots_and_gap(d["x"], c["G"], c["rows"])
    return lowest_argmax(dots).reshape(-1)


def judge(c, d, loss, nn, dx):
    """The two steps of the neighbour rule and the comparison, for every row: (1) nn[i] is a row of the group other than i and
    admissible (tie cases: equal to expected_nn); (2) loss and dx within the oracle's bounds, the oracle evaluated WITH nn.
    d: fp64 inputs on the device of the results; dx None: forward only.  Returns the worst |err| / bound of loss and dx."""
    G, rows, cid = c["G"], c["rows"], c["id"]
    nn = nn.reshape(-1).long()
    own = torch.arange(G * rows, device=nn.device) % rows
    bad = (nn < 0) | (nn >= rows) | (nn == own)
    assert not bool(bad.any()), f"{cid}: nn of rows {bad.nonzero().flatten()[:8].tolist()} is no other row of the group: {nn[bad][:8].tolist()}"
    ok = admissible(d["x"], G, rows).view(G * rows, rows).gather(1, nn[:, None])[:, 0]
    assert bool(ok.all()), f"{cid}: rows {(~ok).nonzero().flatten()[:8].tolist()} chose a neighbour outside the admissible set"
    if c["tie"]:
        want = expected_nn(c, d)
        assert torch.equal(nn, want), f"{cid}: exact ties: rows {(nn != want).nonzero().flatten()[:8].tolist()} did not choose the lowest index"
    exp = reference(d["x"], G, rows, nn, EPS, c["scale"], d["dx_old"] if c["acc"] else None)
    out = [fb.check(f"{cid}: loss", loss, *exp["loss"])[0]]
    if dx is not None:
        out.append(fb.check(f"{cid}: dx", dx, *exp["dx"])[0])
    return out
