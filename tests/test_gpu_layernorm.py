"""The LayerNorm family (csrc/layernorm.hip) against the fp64 oracle of tests/fp64_bounds.py, element by element: lafs_layernorm_fwd,
lafs_layernorm_bwd on both parameter-gradient paths, lafs_layernorm_bwd_fold on its own, lafs_scale_cast_bf16, lafs_dropout_f32 and the
stride checks.  The grid (ln_cases.LN_CASES) reaches every kernel instantiation and both sides of the two-rows-per-wave gate.

Every matrix operand is a column slice of a wider NaN-filled buffer (gemm_cases.inp), every output a slice of a NaN-filled buffer with
guard rows and columns (gemm_cases.Out) that must be bit-identical outside the owned region afterwards; vectors sit between guard
elements.  The C entry points are called directly: the wrappers of ops.py allocate contiguous outputs.  The backward is judged on the
fp32 statistics the kernel's own forward stored -- they are its operands.  tests/test_oracle_rowops_host.py shows on the CPU that these
bounds mean something and reject seeded faults."""
import ctypes as C

import pytest
import torch

pytestmark = pytest.mark.gpu

from lafs_cvpr2024_amd import _lib, ops  # noqa: E402
from lafs_cvpr2024_amd._lib import call  # noqa: E402

import fp64_bounds as fb  # noqa: E402
import gemm_cases as gc  # noqa: E402
import ln_cases as lc  # noqa: E402
from fp64_bounds import U, bf16, f32, f64  # noqa: E402

DEV = "cuda"
GV = 16                                  # guard elements on both sides of a vector


def _p(t):
    return None if t is None else C.c_void_p(t.data_ptr())


class Vec:
    """A contiguous vector (or [n, k] image) between NaN guard elements."""

    def __init__(self, n, dtype=f32, fill=float("nan")):
        self.buf = torch.full((GV + n + GV,), float("nan"), device=DEV, dtype=dtype)
        self.v = self.buf[GV:GV + n]
        self.v.fill_(fill)

    def intact(self, name):
        g = torch.cat([self.buf[:GV], self.buf[-GV:]])
        assert bool(torch.isnan(g).all()), f"{name}: a guard element was written"


def to_dev(d):
    return {k: v.to(DEV) for k, v in d.items()}


def forward(c, d, dd):
    """lafs_layernorm_fwd of case c, checked; returns the kernel's statistics [R, 2] (fp32)."""
    R, D = c["rows"], c["D"]
    x = gc.inp(d["x"], f32, DEV)
    gam, bet = dd["gamma"].float(), dd["beta"].float()
    y = gc.Out(R, D, bf16, DEV).arm() if c["fwd"] in ("both", "y") else None
    yf = gc.Out(R, D, f32, DEV, off=4).arm() if c["fwd"] in ("both", "yf") else None
    st = Vec(2 * R)
    call("lafs_layernorm_fwd", _p(x), x.stride(0), _p(gam), _p(bet), float(c["eps"]), _p(y and y.v), y.v.stride(0) if y else D,
         _p(yf and yf.v), yf.v.stride(0) if yf else D, _p(st.v), R, D)
    torch.cuda.synchronize()
    st.intact(f"{c['id']}: stats")
    exp = lc.fwd_expected(c, dd)
    stats = st.v.view(R, 2)
    fb.check(f"{c['id']}: mean", stats[:, :1], *exp["mean"])
    fb.check(f"{c['id']}: rstd", stats[:, 1:], *exp["rstd"])
    if y is not None:
        y.intact(f"{c['id']}: y")
        fb.check(f"{c['id']}: y", y.v, *exp["y16"], True)
    if yf is not None:
        yf.intact(f"{c['id']}: y_f32")
        fb.check(f"{c['id']}: y_f32", yf.v, *exp["y"])
    if y is not None and yf is not None:
        assert torch.equal(y.v, yf.v.to(bf16)), f"{c['id']}: y is not the bf16 rounding of y_f32"
    return stats.clone()


def drop_factors(c, R, D):
    """(factors fp64 [R, D] or None, seed, device step counter): rows [DROP_ROW0, DROP_ROW0 + R) of a larger mask of
    lafs_debug_dropout_mask, the seed advanced by 7919 * step as the kernel does with its device counter."""
    if not c["drop"]:
        return None, 0, None
    seed = gc.seed_of("drop", c["id"]) & 0xFFFFFF
    step = torch.tensor([float(lc.DROP_STEP)], device=DEV, dtype=f32)
    full = ops.dropout_mask(lc.DROP_ROW0 + R + 5, D, lc.DROP_P, seed + 7919 * lc.DROP_STEP)
    return full[lc.DROP_ROW0:lc.DROP_ROW0 + R].double(), seed, step


def backward(c, d, dd, stats, check=True):
    """lafs_layernorm_bwd of case c (+ the fold on the slot path); returns (dgamma, dbeta) as the kernel left them."""
    R, D = c["rows"], c["D"]
    cid = c["id"]
    x = gc.inp(d["x"], f32, DEV)
    dy = gc.inp(d["dy"], f32 if c["dyf"] else bf16, DEV, off=4 if c["dyf"] else 8)
    gam = dd["gamma"].float()
    g = gc.Out(R, D, f32, DEV, off=4)
    if c["acc"]:
        g.v.copy_(dd["g_old"])
    g.arm()
    gb = gc.Out(R, D, bf16, DEV).arm() if c["gb"] else None
    dgam, dbet = Vec(D), Vec(D)
    dgam.v.copy_(dd["dgamma_old"]); dbet.v.copy_(dd["dbeta_old"])
    sc = dd["seq_scale"].float() if c["scale"] else None
    r2s = dd["row2seq"] if c["scale"] else None
    drop, seed, step = drop_factors(c, R, D)
    n_parts = int(_lib.lib().lafs_layernorm_bwd_parts(R, D))
    part = Vec(n_parts * 2 * D) if c["params"] == "slot" else None
    atomic = part is None
    call("lafs_layernorm_bwd", _p(None if c["dyf"] else dy), dy.stride(0), _p(dy if c["dyf"] else None), dy.stride(0), _p(x), x.stride(0),
         _p(stats), _p(gam), _p(g.v), g.v.stride(0), int(c["acc"]), _p(gb and gb.v), gb.v.stride(0) if gb else D, _p(sc), _p(r2s),
         _p(dgam.v if atomic else None), _p(dbet.v if atomic else None), R, D, lc.DROP_P if c["drop"] else 0.0, seed, _p(step),
         lc.DROP_ROW0 if c["drop"] else 0, _p(part and part.v))
    if not atomic:
        torch.cuda.synchronize()
        assert bool(torch.isfinite(part.v).all()), f"{cid}: a partial slot was left unwritten"
        part.intact(f"{cid}: slots")
        assert torch.equal(dgam.v, dd["dgamma_old"].float()) and torch.equal(dbet.v, dd["dbeta_old"].float()), f"{cid}: the slot path touched dgamma / dbeta"
        item = (_lib.LnFoldItem * 1)()
        item[0].part[0], item[0].n_parts[0] = part.v.data_ptr(), n_parts
        item[0].dgamma, item[0].dbeta = dgam.v.data_ptr(), dbet.v.data_ptr()
        call("lafs_layernorm_bwd_fold", item, 1, D)
    torch.cuda.synchronize()
    g.intact(f"{cid}: g_io")
    dgam.intact(f"{cid}: dgamma"); dbet.intact(f"{cid}: dbeta")
    if gb is not None:
        gb.intact(f"{cid}: gb_out")
    if check:
        st = stats.double()
        exp = lc.bwd_expected(c, dd, st[:, :1], st[:, 1:], drop)
        fb.check(f"{cid}: g_io", g.v, *exp["g"])
        if gb is not None:
            fb.check(f"{cid}: gb_out", gb.v, *exp["gb"], True)
        fb.check(f"{cid}: dgamma", dgam.v, *exp["dgamma"])
        fb.check(f"{cid}: dbeta", dbet.v, *exp["dbeta"])
    return dgam.v.clone(), dbet.v.clone()


@pytest.mark.parametrize("c", lc.LN_CASES, ids=[c["id"] for c in lc.LN_CASES])
def test_layernorm(c):
    d = lc.ln_inputs(c)
    dd = to_dev(d)
    stats = forward(c, d, dd)
    backward(c, d, dd, stats)


@pytest.mark.parametrize("rows,D", [(333, 192), (4097, 384), (4099, 640)])
def test_slot_path_parameter_gradients_are_bitwise_reproducible(rows, D):
    c = lc.ln_case(f"repro-{rows}x{D}", rows, D, fwd="yf")
    d = lc.ln_inputs(c)
    dd = to_dev(d)
    stats = forward(c, d, dd)
    a = backward(c, d, dd, stats)
    b = backward(c, d, dd, stats, check=False)
    assert torch.equal(a[0].view(torch.int32), b[0].view(torch.int32)) and torch.equal(a[1].view(torch.int32), b[1].view(torch.int32))


def test_rsqrtf_allowance():
    """The measurement behind fb.RSQ_REL: rows (-a, -a, a, a) with 11-bit a have mean 0 and variance a^2 exactly (a^2, 2 a^2, 3 a^2 and
    4 a^2 are all fp32 values), so rstd is rsqrtf of the fp32 sum a^2 + eps, which the reference forms with the same single rounding."""
    n = 20000
    a = (torch.arange(n, dtype=f64) % 2047 + 1) * 2.0 ** (torch.arange(n) % 21 - 21).double()
    x = torch.stack([-a, -a, a, a], 1)
    assert torch.equal(x.float().double(), x)
    xd = x.float().to(DEV)
    one, zero, st = torch.ones(4, device=DEV), torch.zeros(4, device=DEV), torch.empty(n, 2, device=DEV)
    yf = torch.empty(n, 4, device=DEV)
    worst = 0.0
    for eps in (1e-6, 1e-5):
        call("lafs_layernorm_fwd", _p(xd), 4, _p(one), _p(zero), eps, None, 4, _p(yf), 4, _p(st), n, 4)
        torch.cuda.synchronize()
        assert bool((st[:, 0] == 0).all())
        arg = ((a * a).float() + torch.tensor(eps, dtype=f32)).double()          # fp32 a^2 (exact) + eps, rounded once
        ref = arg.rsqrt()
        got = st[:, 1].double().cpu()
        ulp = torch.exp2(torch.floor(torch.log2(ref)) - 23)
        worst = max(worst, float(((got - ref).abs() / ulp).max()))
        rel = float(((got - ref).abs() / ref).max())
        assert rel <= fb.RSQ_REL, f"rsqrtf is off by {rel / U:.2f} u relative, allowed {fb.RSQ_REL / U:.0f} u"
    print(f"rsqrtf: worst error {worst:.3f} ulp over {2 * n} arguments")


# ------------------------------------------------------------------------------------------------ the fold on its own
def _fold(D, items):
    """items: [[n_parts of chain 0..3 (None: a NULL chain)]].  Returns nothing; checks every item against the fp64 sum of its slots."""
    gen = torch.Generator()
    gen.manual_seed(gc.seed_of("fold", D, len(items)))
    arr = (_lib.LnFoldItem * len(items))()
    keep = []
    for i, chains in enumerate(items):
        dg, db = Vec(D), Vec(D)
        old = torch.randn(2, D, generator=gen, dtype=f64).float()
        dg.v.copy_(old[0]); db.v.copy_(old[1])
        slots = []
        for ch, n in enumerate(chains):
            if n is None:
                arr[i].part[ch], arr[i].n_parts[ch] = None, 0
                continue
            pv = Vec(n * 2 * D)
            pv.v.copy_(torch.randn(n * 2 * D, generator=gen, dtype=f64).float())
            arr[i].part[ch], arr[i].n_parts[ch] = pv.v.data_ptr(), n
            slots.append(pv)
        arr[i].dgamma, arr[i].dbeta = dg.v.data_ptr(), db.v.data_ptr()
        keep.append((dg, db, old.to(DEV), slots))
    call("lafs_layernorm_bwd_fold", arr, len(items), D)
    torch.cuda.synchronize()
    for i, (dg, db, old, slots) in enumerate(keep):
        dg.intact(f"fold item {i}: dgamma"); db.intact(f"fold item {i}: dbeta")
        allp = torch.cat([s.v.view(-1, 2, D) for s in slots]).double()
        for j, out in enumerate((dg, db)):
            ref, bound = fb.colsum(torch.cat([allp[:, j], old[j:j + 1].double()]))
            fb.check(f"fold D{D} item {i}: {'dgamma' if j == 0 else 'dbeta'}", out.v, ref, bound)


@pytest.mark.parametrize("D", [4, 384, 2048])
def test_fold_four_chains_of_unequal_length(D):
    _fold(D, [[5, None, 17, 33]])
    _fold(D, [[1, 40, None, None]])


@pytest.mark.parametrize("D", [4, 2048])
def test_fold_more_items_than_one_launch_takes(D):
    assert _lib.LnFoldItem is not None
    _fold(D, [[1 + i % 3, None if i % 2 else 2 + i, None, None] for i in range(25)])      # LAFS_LN_FOLD_MAX = 24: two launches


# ------------------------------------------------------------------------------------------------ scale + cast, dropout
SC_CASES = [("50x260-scale-drop", 50, 260, True, True), ("7x4-plain", 7, 4, False, False), ("333x192-scale", 333, 192, True, False),
            ("4100x1028-scale-past-one-sweep", 4100, 1028, True, False), ("4100x1028-drop-past-one-sweep", 4100, 1028, False, True)]


@pytest.mark.parametrize("cid,rows,D,scale,drop", SC_CASES, ids=[c[0] for c in SC_CASES])
def test_scale_cast_bf16(cid, rows, D, scale, drop):
    """bf16(seq_scale g dropfactor): the scales are powers of two (or 0), so without dropout the stored value is the fp64 product
    rounded once, bit for bit; the dropout factor 4/3 rounds the product to fp32 first, which `flip` allows for (u |value|)."""
    c = lc.ln_case("sc-" + cid, rows, D, drop=drop)
    d = lc.ln_inputs(c)
    dd = to_dev(d)
    g = gc.inp(d["g_old"], f32, DEV, off=4)
    out = gc.Out(rows, D, bf16, DEV).arm()
    factors, seed, step = drop_factors(c, rows, D)
    call("lafs_scale_cast_bf16", _p(g), g.stride(0), _p(out.v), out.v.stride(0), _p(dd["seq_scale"].float() if scale else None),
         _p(dd["row2seq"] if scale else None), rows, D, lc.DROP_P if drop else 0.0, seed, _p(step), lc.DROP_ROW0 if drop else 0)
    torch.cuda.synchronize()
    out.intact(cid)
    v = dd["g_old"]
    if scale:
        v = v * dd["seq_scale"][dd["row2seq"].long()][:, None]
    e = torch.zeros_like(v)
    if drop:
        v = v * factors
        e = U * v.abs()
    fb.check(f"scale_cast {cid}", out.v, *fb.flip(v, e), True)


@pytest.mark.parametrize("rows,D", [(50, 260), (3, 1), (2100, 1000)])          # 2100 x 1000: past one grid sweep of 8192 x 256 elements
def test_dropout_f32_in_place(rows, D):
    """x *= factor in place on a strided buffer, with a device step counter: the fp64 product rounded once to fp32, bit for bit."""
    gen = torch.Generator()
    gen.manual_seed(gc.seed_of("dropout", rows, D))
    x = torch.randn(rows, D, generator=gen, dtype=f64).float()
    out = gc.Out(rows, D, f32, DEV, off=3)
    out.v.copy_(x)
    out.arm()
    seed, step = 0x5EED5, torch.tensor([float(lc.DROP_STEP)], device=DEV, dtype=f32)
    call("lafs_dropout_f32", _p(out.v), out.v.stride(0), rows, D, lc.DROP_P, seed, _p(step))
    torch.cuda.synchronize()
    out.intact(f"dropout {rows}x{D}")
    f = ops.dropout_mask(rows, D, lc.DROP_P, seed + 7919 * lc.DROP_STEP).double()
    assert 0.6 < float((f > 0).double().mean()) < 0.9 or rows * D < 100
    ref = (x.double().to(DEV) * f).float()
    assert torch.equal(out.v.view(torch.int32), ref.view(torch.int32)), f"{int((out.v != ref).sum())} elements differ from the product rounded once"


# ------------------------------------------------------------------------------------------------ refusals (nothing is launched)
def test_misaligned_row_strides_are_refused():
    """The vector loads and stores of the backward and of the scale + cast need row strides that are multiples of 4 elements, as the
    forward's do (include/lafs_hip.h).  Only the refusal is tested: a refused request never reaches a kernel, and the outputs keep
    their sentinel."""
    R, D, S = 8, 64, 768.0
    F = lambda: torch.full((R + 2, 132), S, device=DEV, dtype=f32)
    B = lambda: torch.full((R + 2, 132), S, device=DEV, dtype=bf16)
    x, g, dyf, dy, gb = F(), F(), F(), B(), B()
    stats, gam = torch.zeros(R, 2, device=DEV), torch.ones(D, device=DEV)
    dgam, dbet = torch.zeros(D, device=DEV), torch.zeros(D, device=DEV)

    def bwd(ldx=132, ldg=132, lddyf=132, lddy=132, ldgb=132, use_f32=False, use_gb=True):
        call("lafs_layernorm_bwd", _p(None if use_f32 else dy), lddy, _p(dyf if use_f32 else None), lddyf, _p(x), ldx, _p(stats), _p(gam), _p(g), ldg,
             1, _p(gb if use_gb else None), ldgb, None, None, _p(dgam), _p(dbet), R, D, 0.0, 0, None, 0, None)

    def cast(ldg=132, ldgb=132):
        call("lafs_scale_cast_bf16", _p(g), ldg, _p(gb), ldgb, None, None, R, D, 0.0, 0, None, 0)

    refused = [lambda: bwd(ldx=130), lambda: bwd(ldg=130), lambda: bwd(lddyf=130, use_f32=True), lambda: bwd(lddy=130), lambda: bwd(ldgb=130),
               lambda: bwd(ldx=66), lambda: bwd(lddy=65), lambda: cast(ldg=130), lambda: cast(ldgb=130), lambda: cast(ldgb=67)]
    for fn in refused:
        with pytest.raises(_lib.LafsHipError, match="row strides must be multiples of 4"):
            fn()
    torch.cuda.synchronize()
    for t in (g, gb):
        assert bool((t == S).all()), "an output was written by a refused call"
    assert bool((dgam == 0).all()) and bool((dbet == 0).all())
    # the strides of operands that are not in use are not looked at, and the same requests run once aligned
    x.zero_(); dy.zero_(); dyf.zero_(); g.zero_()
    bwd(lddyf=130)
    bwd(lddy=130, use_f32=True)
    bwd(ldgb=130, use_gb=False)
    cast()
    torch.cuda.synchronize()
    assert bool((g[:R, :D] == 0).all()) and bool((gb[:R, :D] == 0).all()) and bool((gb[:, D:] == S).all()) and bool((g[:, D:] == 0).all())
