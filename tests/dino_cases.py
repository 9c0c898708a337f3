"""The case grids of tests/test_gpu_dino_head.py (head.hip, dino_loss.hip, dino_head_loss.hip), their seeded input distributions and
what the oracle of tests/fp64_bounds.py expects for a case.  Kept apart from the GPU module so that tests/test_oracle_dino_host.py
judges on the CPU exactly the cases the GPU runs.  Every shape is the smallest that reaches its code path (the paths are named beside
the grids); the references run on whatever device the operands live on."""
import torch

import fp64_bounds as fb
from fp64_bounds import f32, f64, rbf
from gemm_cases import seed_of

rf = lambda v: v.to(f32).double()


def _gen(*key):
    g = torch.Generator()
    g.manual_seed(seed_of("dino", *key))
    return g


def r4(n):
    return (n + 3) // 4 * 4


def r8(n):
    return (n + 7) // 8 * 8


# ------------------------------------------------------------------------------------------------ row kernels of head.hip
# One wave per row, four rows per workgroup (rows 1, 4, 5, 7: a partial, a full, a full + 1 and a partial second workgroup), a lane's
# float4 at lane * 4 + 256 i (D 4: one lane; 252 / 256 / 260: around the first chunk's end; 1024: the largest D).
ROW_KINDS = ("normal", "zero", "tiny", "small", "outlier")


def _row_grid():
    g = []
    for i, (rows, D) in enumerate((r, D) for D in (4, 64, 252, 256, 260, 1024) for r in (1, 4, 5, 7)):
        # (rows cycle with i % 4, D with d = i // 4: over the six D every row count meets accumulate 0 / 1 with dg NULL / present)
        r, d = i % 4, i // 4
        g.append(dict(id=f"{rows}x{D}-k{i % 5}", rows=rows, D=D, rot=i, acc=(r + d) % 2, dg=(r + d // 2) % 2 == 0))
    return g


ROW_CASES = _row_grid()


def row_kinds(c, weight=False):
    """The kind of every row: the five kinds rotate with the case index so that the one-row cases meet each.  weight: no zero rows (a
    zero row of v gives NaN, as in torch)."""
    kinds = tuple(k for k in ROW_KINDS if not (weight and k == "zero"))
    return [kinds[(c["rot"] + r) % len(kinds)] for r in range(c["rows"])]


def row_inputs(c, weight=False):
    """x [rows, D] by row kind -- normal; all zero (y = 0, inv = 1e12, dx = 1e12 dy); norm about 1e-13 (below the 1e-12 clamp); norm
    about 1e-3; one element 1e4 times the rest -- and dy, g (!= 1), old dv / dg: fp64 tensors of fp32 values."""
    gen = _gen("row", c["id"], weight)
    R, D = c["rows"], c["D"]
    rn = lambda *s: torch.randn(*s, generator=gen, dtype=f64)
    x = rn(R, D)
    for r, k in enumerate(row_kinds(c, weight)):
        if k == "zero":
            x[r] = 0
        elif k == "tiny":
            x[r] *= 1e-13 / x[r].norm()
        elif k == "small":
            x[r] *= 1e-3 / x[r].norm()
        elif k == "outlier":
            x[r, (3 * r + 1) % D] = 1e4
    return dict(x=rf(x), dy=rf(rn(R, D)), g=rf(1.5 + 0.5 * rn(R, 1).clamp(-2, 2)), dv_old=rf(rn(R, D)), dg_old=rf(rn(R, 1)))


def l2_fwd_expected(c, d):
    return fb.l2norm_fwd(d["x"])


def l2_bwd_expected(c, d, inv):
    return fb.l2norm_bwd(d["x"], d["dy"], inv)


def wn_bwd_expected(c, d, inv):
    return fb.weightnorm_bwd(d["dy"], d["x"], d["g"], inv, d["dv_old"] if c["acc"] else None, d["dg_old"] if c["acc"] else None)


# weightnorm_fwd: 64 rows per workgroup (K 1, 63, 64, 65, 130: one row, a block less one, a block, a block + 1, two blocks + 2); Kpad
# = K rounded up to 8 / to 128 / K + 72 (the last gives a workgroup of pad rows only); w_t NULL at D 4, 260, 1024 and present at D 64,
# 256 with ldwt > Kpad (then Kpad is rounded up to 8, as the entry point demands).
def _wn_grid():
    g = []
    i = 0
    for K in (1, 63, 64, 65, 130):
        for pad in ("r8", "r128", "p72"):
            Kpad = {"r8": r8(K), "r128": (K + 127) // 128 * 128, "p72": K + 72}[pad]
            g.append(dict(id=f"K{K}-{pad}-D{(4, 260, 1024)[i % 3]}", K=K, Kpad=Kpad, D=(4, 260, 1024)[i % 3], wt=False))
            g.append(dict(id=f"K{K}-{pad}-D{(64, 256)[i % 2]}-wt", K=K, Kpad=r8(Kpad), D=(64, 256)[i % 2], wt=True))
            i += 1
    return g


WN_CASES = _wn_grid()


def wn_inputs(c):
    gen = _gen("wn", c["id"])
    K, D = c["K"], c["D"]
    v = torch.randn(K, D, generator=gen, dtype=f64) * torch.logspace(-2, 1, K, dtype=f64)[torch.randperm(K, generator=gen)][:, None]
    return dict(v=rf(v), g=rf(1.5 + 0.5 * torch.randn(K, 1, generator=gen, dtype=f64).clamp(-2, 2)))


def wn_fwd_expected(c, d):
    return fb.weightnorm_fwd(d["v"], d["g"])


# ------------------------------------------------------------------------------------------------ lafs_dino_loss_fwd_bwd
# K: 2, 3 (the tail loop of row_stats only, the clamped re-read at column 0), 4, 5, 1003, 1027, 4100, 14337 (ragged tails of every
# length), 1024, 4096, 14336 (none); 4096 / 4100: one and two trips of the 4096-class loop; 14336 / 14337: exactly 14 chunks and 14 + 1
# in loss_final_kernel.  (16, 65): 1040 > 1024 rows, loss_final_kernel's second trip.
LOSS_DISTS = ("normal", "cosine", "sharp", "offset", "flat-student", "big-center")
LOSS_KS = (2, 3, 4, 5, 1003, 1024, 1027, 4096, 4100, 14336, 14337)
LOSS_NB = ((2, 1), (3, 2), (5, 3), (10, 6), (16, 2))
TEMPS = ((0.04, False), (0.07, False), (0.04, True), (0.07, True))       # (teacher temperature, from dev_temps)
HOST_WRONG = (0.2, 0.05)                                                  # what the host arguments hold when dev_temps is given
SCALES = (1.0, 1.0 / 3.0, 1024.0)


def loss_case(cid, K, ncrops, B, n, **kw):
    c = dict(id=cid, K=K, ncrops=ncrops, B=B, dist=LOSS_DISTS[n % 6], ld=r4(K) + 8 * ((n // 3) % 2), g16=(n // 2) % 2 == 0,
             scale=SCALES[(n // 4) % 3], tt=TEMPS[n % 4][0], dev=TEMPS[n % 4][1], ts=0.1)
    c.update(kw)
    c["ldg"] = c["ld"] + 4
    return c


def _loss_grid():
    g = []
    n = 0
    for i, K in enumerate(LOSS_KS):
        pairs = [LOSS_NB[(i + j) % 5] for j in range(3)] + ([(16, 65)] if K <= 8 else [])
        for nc, B in pairs:
            g.append(loss_case(f"K{K}-{nc}x{B}-{n}", K, nc, B, n))
            n += 1
    # forms the rotation above does not pair: an fp32 gradient with ldg != ld behind a ragged tail under device temperatures and a
    # grad_scale != 1; `offset` rows at a ragged K; the sharp teacher in fp32
    g.append(loss_case("K1027-5x3-f32-dev-third", 1027, 5, 3, 0, dist="normal", g16=False, scale=1.0 / 3.0, tt=0.04, dev=True))
    g.append(loss_case("K1003-5x3-offset-bf16", 1003, 5, 3, 0, dist="offset", g16=True, scale=1.0, tt=0.04, dev=False))
    g.append(loss_case("K4100-5x3-sharp-f32", 4100, 5, 3, 0, dist="sharp", g16=False, scale=1024.0, tt=0.04, dev=False, ld=4108))
    g.append(loss_case("K5-3x2-bigc-f32", 5, 3, 2, 0, dist="big-center", g16=False, scale=1.0, tt=0.07, dev=True))
    # the rotation gives every bf16 case host temperatures, `sharp` tau_t 0.04 only and `cosine` 0.07 only: a bf16 gradient under
    # device temperatures (the coef correction in loss_grad_kernel<true>) and the two other pairings
    g.append(loss_case("K1027-5x3-bf16-dev-third", 1027, 5, 3, 0, dist="cosine", g16=True, scale=1.0 / 3.0, tt=0.04, dev=True))
    g.append(loss_case("K4100-3x2-sharp-bf16-dev-07", 4100, 3, 2, 0, dist="sharp", g16=True, scale=1024.0, tt=0.07, dev=True, ld=4108))
    g.append(loss_case("K1003-10x6-cosine-f32-04", 1003, 10, 6, 0, dist="cosine", g16=False, scale=1.0, tt=0.04, dev=False))
    ids = [c["id"] for c in g]
    assert len(set(ids)) == len(ids)
    return g


LOSS_CASES = _loss_grid()


def logits(dist, rows_s, rows_t, K, gen):
    """normal: N(0, 3^2) student, N(0, 2^2) teacher;  cosine: uniform in [-1, 1] (what training produces);  sharp: teacher rows near
    one-hot (one class 0.8 above a +-0.2 floor: 20 units at tau_t 0.04);  offset: +-50 added to whole rows of either sign;
    flat-student: all student logits equal;  big-center: centre entries up to +-5.  (Never student and teacher both flat: that gradient is
    a pure cancellation.)"""
    rn = lambda *s: torch.randn(*s, generator=gen, dtype=f64)
    ru = lambda *s: 2 * torch.rand(*s, generator=gen, dtype=f64) - 1
    center = 0.3 * rn(K)
    if dist == "cosine":
        s, t, center = ru(rows_s, K), ru(rows_t, K), 0.1 * rn(K)
    elif dist == "sharp":
        s, t, center = ru(rows_s, K), 0.2 * ru(rows_t, K), 0.05 * rn(K)
        t[torch.arange(rows_t), torch.randint(0, K, (rows_t,), generator=gen)] = 1.0
    else:
        s, t = 3 * rn(rows_s, K), 2 * rn(rows_t, K)
    if K <= 8:
        # A tenth of the teacher's and the centre's scale (N(0, 0.2^2) for `normal`): over a handful of classes the full scales leave student and
        # teacher one-hot on the same class in some rows, where n_v p - sum q is a pure cancellation of two values near 1 whose
        # arguments round by more than their difference -- no bound can hold that to a bf16 step of the result.
        # The student a third of that again: a sharp teacher (big-center) must not meet a student that is one-hot on the same class.
        # The row offsets of `offset` are +-5 here: at +-50 the arguments (700) round by 1e-4, a bf16 step of differences of 0.05.
        s, t, center = s / 30, 0.1 * t, 0.1 * center
    if dist == "offset":
        off = 5.0 if K <= 8 else 50.0
        s = s + off * (1 - 2 * (torch.arange(rows_s) % 2).double())[:, None]
        t = t - off * (1 - 2 * (torch.arange(rows_t) % 2).double())[:, None]
    elif dist == "flat-student":
        s = torch.full((rows_s, K), 0.25, dtype=f64)
    elif dist == "big-center":
        center = 5 * ru(K)
    return rf(s), rf(t), rf(center)


def loss_inputs(c):
    s, t, center = logits(c["dist"], c["ncrops"] * c["B"], 2 * c["B"], c["K"], _gen("loss", c["id"]))
    return dict(s=s, t=t, center=center)


def host_temps(c):
    """The (student, teacher) temperatures passed as host arguments."""
    return HOST_WRONG if c["dev"] else (c["ts"], c["tt"])


def coef_of(c):
    return fb.dino_coef(c["ncrops"], c["B"], host_temps(c)[0], c["scale"], c["ts"] if c["dev"] else None)


def loss_expected(c, d):
    z = torch.zeros((), dtype=f64, device=d["s"].device)
    return fb.dino_loss(d["s"], z, d["t"], z, d["center"], c["ncrops"], c["B"], (c["ts"], c["tt"]), coef_of(c), c["g16"], c["dev"])


# ------------------------------------------------------------------------------------------------ lafs_dino_head_loss
# 64-class blocks, 32-row tiles, four waves.  (K, Kpad): (1, 8) one class; (63, 64), (64, 64) around a block; (65, 72) a block cut by
# both K and Kpad; (65, 256), (200, 256) pad-only blocks; (4096, 4096) 64 blocks, (4100, 4224) 65 (row_lse_kernel's second trip) and
# a pad-only block.  (ncrops, B): rows_t 2 and 128, rows_s no multiple of 32, rows_s > 128 (several tiles per wave), 1024 rows.
HEAD_KS = ((1, 8), (63, 64), (64, 64), (65, 72), (65, 256), (200, 256), (4096, 4096), (4100, 4224))
HEAD_NB = ((2, 1), (3, 5), (10, 16), (16, 64), (4, 64))
HEAD_OPS = ("l2", "unnormalised", "aligned")


def head_case(cid, K, Kpad, ncrops, B, n, **kw):
    c = dict(id=cid, K=K, Kpad=Kpad, ncrops=ncrops, B=B, ops=HEAD_OPS[n % 3], ldg=Kpad + 8 * (n % 2), colsum=(n // 2) % 2 == 0,
             scale=SCALES[(n // 3) % 3], tt=TEMPS[n % 4][0], dev=TEMPS[n % 4][1], ts=0.1, g16=True)
    c.update(kw)
    return c


def _head_grid():
    g = []
    n = 0
    for i, (K, Kpad) in enumerate(HEAD_KS):
        for j in range(3):
            nc, B = HEAD_NB[(i + j) % 5]
            if (nc, B) == (16, 64) and K > 200:
                continue
            g.append(head_case(f"K{K}p{Kpad}-{nc}x{B}-{n}", K, Kpad, nc, B, n))
            n += 1
    g.append(head_case("K65p256-3x5-dev-third", 65, 256, 3, 5, 0, ops="l2", scale=1.0 / 3.0, tt=0.04, dev=True, ldg=264))
    g.append(head_case("K200p256-16x64-aligned", 200, 256, 16, 64, 0, ops="aligned", scale=1.0, tt=0.04, dev=False))
    ids = [c["id"] for c in g]
    assert len(set(ids)) == len(ids)
    return g


HEAD_CASES = _head_grid()


def head_inputs(c):
    """zs [ncrops B, 256], zt [2 B, 256], ws, wt [Kpad, 256] (pad rows zero) as fp64 tensors of bf16 values, centre [K].  l2: rows
    normalised before the bf16 rounding;  unnormalised: student and teacher rows of norm about 3 (the weights stay normalised);  aligned:
    every third student row and every second teacher row equals a weight row of its network (logit 1: sharp)."""
    gen = _gen("head", c["id"])
    K, Kpad, rows_s, rows_t = c["K"], c["Kpad"], c["ncrops"] * c["B"], 2 * c["B"]
    unit = lambda n: torch.nn.functional.normalize(torch.randn(n, 256, generator=gen, dtype=f64), dim=1)
    zs, zt = unit(rows_s), unit(rows_t)
    ws, wt = torch.zeros(Kpad, 256, dtype=f64), torch.zeros(Kpad, 256, dtype=f64)
    ws[:K], wt[:K] = unit(K), unit(K)
    if c["ops"] == "unnormalised":
        zs, zt = 3 * zs, 3 * zt
    elif c["ops"] == "aligned":
        zs[::3] = ws[torch.randint(0, K, (zs[::3].shape[0],), generator=gen)]
        zt[::2] = wt[torch.randint(0, K, (zt[::2].shape[0],), generator=gen)]
    return dict(zs=rbf(zs), zt=rbf(zt), ws=rbf(ws), wt=rbf(wt), center=rf(0.1 * torch.randn(K, generator=gen, dtype=f64)))


def head_logits(c, d):
    """The logits of the fused kernel and their bounds: `gemm` on the exact bf16 operands, K = 256."""
    K = c["K"]
    s, se = fb.gemm(d["zs"], None, d["ws"][:K])
    t, te = fb.gemm(d["zt"], None, d["wt"][:K])
    return s, se, t, te


def head_expected(c, d):
    s, se, t, te = head_logits(c, d)
    out = fb.dino_loss(s, se, t, te, d["center"], c["ncrops"], c["B"], (c["ts"], c["tt"]), coef_of(c), True, c["dev"], fused=True)
    cs, cse = fb.colsum(t)
    out["colsum"] = (cs, cse + te.sum(0))
    return out


# ------------------------------------------------------------------------------------------------ colsum, centre EMA
# colsum: eight rows in flight (rows 1, 7, 8, 9, 17), 256 classes per workgroup (K 1, 255, 256, 257), ld > K
COLSUM_CASES = [dict(id=f"{rows}x{K}", rows=rows, K=K, ld=r4(K) + 4) for rows in (1, 7, 8, 9, 17) for K in (1, 255, 256, 257)]
EMA_CASES = [dict(id=f"K{K}-B{B}-world{w}", K=K, m=0.9, inv_rows=1.0 / (2 * B * w)) for K in (1, 256, 257) for B, w in ((3, 1), (64, 8))]


def colsum_inputs(c):
    return dict(x=rf(2 * torch.randn(c["rows"], c["K"], generator=_gen("colsum", c["id"]), dtype=f64)))


def ema_inputs(c):
    gen = _gen("ema", c["id"])
    return dict(center=rf(0.3 * torch.randn(c["K"], generator=gen, dtype=f64)), colsum=rf(8 * torch.randn(c["K"], generator=gen, dtype=f64)))


def ema_expected(c, d):
    return fb.center_ema(d["center"], d["colsum"], c["inv_rows"], c["m"])
