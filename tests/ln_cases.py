"""The case grid of tests/test_gpu_layernorm.py, its seeded input distributions and what the oracle of tests/fp64_bounds.py expects for a
case.  Kept apart from the GPU module so that tests/test_oracle_rowops_host.py judges on the CPU exactly the cases the GPU runs.  The
guarded buffers are those of tests/gemm_cases.py (`inp`, `Out`)."""
import torch

import fp64_bounds as fb
from fp64_bounds import f32, f64, rbf
from gemm_cases import seed_of

SEQ_SCALE = [0.0, 1.0, 2.0, 0.5]        # per-sequence DropPath scales; a sequence is 3 rows, so boundaries fall inside a wave's pair of rows
DROP_P, DROP_ROW0, DROP_STEP = 0.25, 96, 3
DISTS = ("normal", "offset", "spread")


def ln_case(cid, rows, D, dist="normal", **kw):
    """fwd: which outputs the forward stores ('both', 'y', 'yf').  dyf: fp32 dy instead of bf16; acc: accumulate into g_io (0: g_io is
    pre-filled with NaN); gb: gb_out given; scale: seq_scale given; drop: dropout on gb_out; params: 'slot' (part_out + fold) or
    'atomic'.  The grid's ids name the kernel family a shape reaches (one row or two rows per wave; the dispatch is by shape alone)."""
    c = dict(id=cid, rows=rows, D=D, dist=dist, eps=1e-6, fwd="both", dyf=False, acc=True, gb=True, scale=True, drop=False, params="slot")
    c.update(kw)
    return c


def _grid():
    g = []
    small = [(1, 4), (3, 4), (5, 4), (7, 64), (50, 260), (333, 192), (64, 768), (9, 1028), (5, 2044), (7, 2048)]
    gate = [(r, D) for D in (128, 256, 384, 512) for r in (4095, 4096, 4097)]
    big = [(8201, 384), (4100, 192), (4099, 640)]
    for i, (rows, D) in enumerate(small + gate + big):
        two = rows >= 4096 and D % 128 == 0 and D <= 512
        tag = f"{rows}x{D}-{'two-row' if two else 'one-row'}"
        # the operand forms rotate over the shapes; every form meets every kernel family below
        g.append(ln_case(f"{tag}-{DISTS[i % 3]}", rows, D, DISTS[i % 3], eps=(1e-6, 1e-5)[i % 2], fwd=("both", "y", "yf")[i % 3],
                         acc=bool(i % 2), gb=i % 4 != 3, scale=i % 3 != 2, params=("slot", "atomic")[(i // 2) % 2]))
    # every distribution and both eps on a small and a two-row shape
    for dist in DISTS:
        for eps in (1e-6, 1e-5):
            g.append(ln_case(f"dist-333x192-{dist}-eps{eps}", 333, 192, dist, eps=eps))
            g.append(ln_case(f"dist-4097x384-{dist}-eps{eps}", 4097, 384, dist, eps=eps, params="atomic"))
    # fp32 dy: stays on the one-row kernel past the two-row gate
    g.append(ln_case("dyf-4097x384-one-row", 4097, 384, dyf=True, acc=False, gb=False, scale=False))
    g.append(ln_case("dyf-4096x128-one-row-atomic", 4096, 128, dyf=True, params="atomic"))
    g.append(ln_case("dyf-50x260", 50, 260, dyf=True, acc=False))
    g.append(ln_case("dyf-5x2044-atomic", 5, 2044, dyf=True, params="atomic", eps=1e-5))
    # accumulate 0 / 1, with and without gb_out, slots and atomics on both kernel families
    for rows, D in ((333, 192), (4097, 256)):
        for acc in (False, True):
            for gb in (False, True):
                for params in ("slot", "atomic"):
                    g.append(ln_case(f"forms-{rows}x{D}-acc{int(acc)}-gb{int(gb)}-{params}", rows, D, acc=acc, gb=gb, scale=gb, params=params))
    # dropout inside the backward at drop_row0 != 0 with a device step counter
    g.append(ln_case("drop-50x260", 50, 260, drop=True))
    g.append(ln_case("drop-4097x384-two-row", 4097, 384, drop=True, eps=1e-5))
    g.append(ln_case("drop-4097x384-dyf-one-row", 4097, 384, drop=True, dyf=True, scale=False))
    ids = [c["id"] for c in g]
    assert len(set(ids)) == len(ids)
    return g


LN_CASES = _grid()


def const_rows(rows):
    """The exactly constant rows (variance 0) of a case."""
    return [] if rows < 3 else sorted({1, rows // 2})


def ln_inputs(c, rows=None):
    """The operands of case c as fp64 CPU tensors of exactly representable values.
    normal: 2 randn + 0.5;  offset: mean 30, std 0.5 (a one-pass variance fails here);  spread: randn with a per-row scale from 1e-3
    to 1e3;  in every distribution rows 1 and rows // 2 are exactly constant.  rows: keep only the first `rows` rows."""
    gen = torch.Generator()
    gen.manual_seed(seed_of("ln", c["id"]))
    R, D = c["rows"], c["D"]
    rn = lambda *s: torch.randn(*s, generator=gen, dtype=f64)
    rf = lambda v: v.to(f32).double()
    if c["dist"] == "normal":
        x = 2 * rn(R, D) + 0.5
    elif c["dist"] == "offset":
        x = 30 + 0.5 * rn(R, D)
    else:
        x = rn(R, D) * torch.logspace(-3, 3, R, dtype=f64)[torch.randperm(R, generator=gen)][:, None]
    for i, r in enumerate(const_rows(R)):
        # (small values: at variance 0 rstd = eps^-1/2 multiplies the mean's rounding allowance, sum_depth u |value|, by up to 1000 --
        # with values near 1 that allowance alone would exceed a bf16 step of the outputs, which equal beta here)
        x[r] = (2.0 ** -10, -2.0 ** -9)[i % 2]
    d = dict(x=rf(x), gamma=rf(1 + 0.5 * rn(D)), beta=rf(rn(D)), g_old=rf(rn(R, D)), dgamma_old=rf(rn(D)), dbeta_old=rf(rn(D)))
    d["dy"] = rf(rn(R, D)) if c["dyf"] else rbf(rn(R, D))
    d["row2seq"] = ((torch.arange(R) // 3) % len(SEQ_SCALE)).int()
    d["seq_scale"] = torch.tensor(SEQ_SCALE, dtype=f64)
    if rows is not None and rows < R:
        for k in ("x", "g_old", "dy", "row2seq"):
            d[k] = d[k][:rows]
    return d


def fwd_expected(c, d):
    return fb.ln_fwd(d["x"], d["gamma"], d["beta"], fb.f32c(c["eps"]))


def bwd_expected(c, d, mean, rstd, drop=None):
    """The backward of case c on operands d (fp64, any device) and the fp32 statistics the kernel is handed ([R, 1] each)."""
    s = d["seq_scale"][d["row2seq"].long()][:, None] if c["scale"] else None
    return fb.ln_bwd(d["dy"], d["x"], mean, rstd, d["gamma"], d["g_old"] if c["acc"] else None, s, drop, d["dgamma_old"], d["dbeta_old"])
