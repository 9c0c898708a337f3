"""lafs_mlp_fused (csrc/mlp_fused.hip) against a plain fp64 restatement of the same operation, over the whole domain
lafs_mlp_fused_supported accepts: every hidden width, ragged and multi-launch row counts, the three modes and the four fusions.

The reference rounds to bf16 only where include/lafs_hip.h says the kernel stores bf16, and carries next to every value a bound on
how far the kernel's value may lie from it, element by element (never normalised by a tensor's maximum).  Where the kernel stores a
bf16 value the bound is the distance to the neighbouring bf16 values that the kernel's unrounded value can reach: 0 where no
rounding boundary lies within reach, so most bf16 outputs must match the reference exactly.  Later stages take an earlier stage's
bound along, so a single flipped bf16 operand is never mistaken for an error and a wrong row is never hidden by a large one."""
import ctypes as C
import math
import zlib

import pytest
import torch

pytestmark = pytest.mark.gpu

from lafs_cvpr2024_amd import _lib, ops  # noqa: E402

DEV = "cuda"
bf16, f32, f64 = torch.bfloat16, torch.float32, torch.float64
D = 384
EPS = 1e-6              # LayerNorm eps of the ViT blocks
GR = 16                 # guard rows past M in every buffer (a wave owns 16 rows)
GUARD = 12345.0
FWD, SAVE, BWD = _lib.MLP_FWD, _lib.MLP_FWD_SAVE, _lib.MLP_BWD
MODE_NAME = {FWD: "fwd", SAVE: "save", BWD: "bwd"}
SEQ_SCALE = [0.0, 1 / 0.9, 1.25, 0.0, 0.5, 1 / 0.9, 2.0]          # per-sequence DropPath scales, zeros included


class _NullCtx:
    handle = None                                    # lafs_mlp_args.ctx = NULL: one launch of 128-row units


def n_cu():
    return torch.cuda.get_device_properties(0).multi_processor_count     # what lafs_ctx_create reads


# ---- row counts.  Small ones, a last 128-row unit with 1..7 active waves, and the shapes of the launch split (launch() in
# mlp_fused.hip): one full round of the chip, a second launch of 64-row units with 1, 2, 3 active waves in its last unit, and a
# remainder too large for one round of 64-row units (whole 128-row units again).
M_SMALL = [1, 15, 16, 17, 127, 128, 129]
M_WAVES = [256 + 16 * (w - 1) + 1 + (3 * w + 5) % 16 for w in range(1, 8)]
M_CU = {"ncu*128": lambda n: n * 128,
        "ncu*128+64*2+5": lambda n: n * 128 + 64 * 2 + 5,
        "ncu*128+64*5+25": lambda n: n * 128 + 64 * 5 + 25,
        "ncu*128+64*7+33": lambda n: n * 128 + 64 * 7 + 33,
        "ncu*192+33": lambda n: n * 192 + 33}
M_GRID = [str(m) for m in M_SMALL + M_WAVES] + list(M_CU)


def rows_of(spec):
    return M_CU[spec](n_cu()) if spec in M_CU else int(spec)


H_ALL = list(range(128, 1537, 64))                   # the 24 accepted hidden widths
H_GRID = [128, 192, 256, 512, 704, 1472, 1536]       # NI = H / 64 of every residue mod 3 (the ring of three LDS buffers), both ends
H_OPT = [256, 704, 1536]                             # NI % 3 = 1, 2, 0


# ------------------------------------------------------------------------------------------------ fp64 reference with bounds
# rbf, flip, gemm (4 sqrt(K) u sum|terms| + K u |bias|) and gelu (EPS_PHI) live in tests/fp64_bounds.py, shared with the GEMM modules
from fp64_bounds import EPS_PHI, U, flip, gelu, gemm, rbf  # noqa: E402,F401


def mlp_fwd(X, Xe, Wa, Wb, ba, bb, resid, s, a_kernel=None):
    """y = resid + s (bf16(gelu(X Wa^T + ba)) Wb^T + bb); a = bf16(gelu(u)), gd = bf16(gelu'(u)), each with its bound.  With
    a_kernel (the gelu(u) the kernel stored, checked against a by the caller) y is formed from it instead."""
    u, ue = gemm(X, Xe, Wa, ba)
    g, ge, dg, dge = gelu(u, ue)
    del u, ue
    a, ae = flip(g, ge)
    gd, gde = flip(dg, dge)
    del g, ge, dg, dge
    z, ze = gemm(a, ae, Wb, bb) if a_kernel is None else gemm(a_kernel, None, Wb, bb)
    y = resid + s * z
    # the residual epilogue: two fp32 roundings
    return y, s.abs() * ze + 2 * U * (resid.abs() + (s * z).abs()), a, ae, gd, gde


def mlp_bwd(dY, Wa, Wb, gd):
    """du = bf16((dY Wa^T) * gelu'(u)), dX = bf16(du Wb^T), each with its bound."""
    t, te = gemm(dY, None, Wa)
    v = t * gd
    # the product with the saved gelu'(u): one fp32 rounding
    du, due = flip(v, te * gd.abs() + U * v.abs())
    dx, dxe = gemm(du, due, Wb)
    dxb, dxbe = flip(dx, dxe)
    return du, due, dxb, dxbe


def layernorm(x, gam, bet):
    """LayerNorm of exact fp32 rows as the kernel evaluates it (fp32, mean first, then the sum of squares around it): the output
    before its bf16 rounding, the mean and rstd, each with its bound."""
    m = x.mean(1, keepdim=True)
    c = x - m
    var = (c * c).mean(1, keepdim=True)
    r = (var + EPS).rsqrt()
    # fp32 sum of D values, then / D
    me = D * U * x.abs().mean(1, keepdim=True) + U * m.abs()
    # sum (c - dm)^2 = sum c^2 + D dm^2 (sum c = 0), fp32 sum of D rounded squares, / D, + eps
    ve = me * me + (D + 5) * U * (var + me * me) + U * EPS
    # rsqrt of a value off by ve (first order, doubled) and the 1-ulp hardware rsqrt
    re = r * (ve / (var + EPS) + 2 * U)
    # (x - mean) * rstd: two roundings
    he = r * me + c.abs() * (re + 3 * U * r) + me * re
    h = c * r * gam + bet
    # fma with gamma and beta: one rounding
    return h, gam.abs() * he + U * h.abs(), m, me, r, re


def layernorm_bwd(dxb, dxbe, x, mean, rstd, gam, g0, s):
    """The LayerNorm-backward epilogue on bf16 dX known to within dxbe: the new gradient stream, its bf16 DropPath-scaled copy and
    dgamma / dbeta, each with its bound (x-hat from the fp32 statistics the kernel is handed)."""
    xh = (x - mean) * rstd
    # two fp32 roundings
    xhe = 2 * U * xh.abs()
    d = dxb * gam
    de = dxbe * gam.abs() + U * d.abs()
    # row means: fp32 sums of D values
    m1 = d.mean(1, keepdim=True)
    m1e = (de.sum(1, keepdim=True) + D * U * d.abs().sum(1, keepdim=True)) / D + U * m1.abs()
    p = d * xh
    pe = de * xh.abs() + d.abs() * xhe + U * p.abs()
    m2 = p.mean(1, keepdim=True)
    m2e = (pe.sum(1, keepdim=True) + D * U * p.abs().sum(1, keepdim=True)) / D + U * m2.abs()
    dx = rstd * (d - m1 - xh * m2)
    # three fp32 roundings inside the parenthesis, one for the product with rstd
    dxe = rstd * (de + m1e + xh.abs() * m2e + xhe * m2.abs() + 3 * U * (d.abs() + m1.abs() + (xh * m2).abs())) + U * dx.abs()
    gn = g0 + dx
    gne = dxe + U * gn.abs()
    gb, gbe = flip(s * gn, s.abs() * gne + U * (s * gn).abs())
    # column sums: fp32 within a slot of at most 128 rows, the slots summed here in fp64
    dg = (dxb * xh).sum(0)
    dge = (dxbe * xh.abs() + dxb.abs() * xhe + U * (dxb * xh).abs()).sum(0) + 128 * U * (dxb * xh).abs().sum(0)
    db, dbe = dxb.sum(0), dxbe.sum(0) + 128 * U * dxb.abs().sum(0)
    return gn, gne, gb, gbe, dg, dge, db, dbe


# ------------------------------------------------------------------------------------------------ buffers and checks
def inp(v, dtype, pad=0):
    """v as a view into a NaN-filled buffer with `pad` more columns and GR more rows: a read of either poisons a checked value."""
    buf = torch.full((v.shape[0] + GR, v.shape[1] + pad), float("nan"), device=DEV, dtype=dtype)
    buf[:v.shape[0], :v.shape[1]] = v
    return buf[:v.shape[0], :v.shape[1]]


class Out:
    """Output view [rows, cols] into a guard-filled buffer with `pad` more columns and GR more rows."""

    def __init__(self, rows, cols, dtype, pad=0):
        self.buf = torch.full((rows + GR, cols + pad), GUARD, device=DEV, dtype=dtype)
        self.v = self.buf[:rows, :cols]

    def untouched(self, name, whole=False):
        g = torch.tensor(GUARD, dtype=self.buf.dtype, device=DEV)
        rows, cols = self.v.shape
        if whole:
            assert bool((self.buf == g).all()), f"{name}: written although the launch must not write it"
        assert bool((self.buf[rows:] == g).all()), f"{name}: rows past M were written"
        assert bool((self.buf[:rows, cols:] == g).all()), f"{name}: columns past the logical width were written"


def check(name, got, ref, bound):
    got, ref, bound = got.double(), ref.double(), bound.double()
    if got.dim() == 1:
        got, ref, bound = got[None], ref[None], bound[None]
    fin = torch.isfinite(got)
    if not bool(fin.all()):
        rows = (~fin).any(1).nonzero().flatten()
        raise AssertionError(f"{name}: {int((~fin).sum())} non-finite values in {rows.numel()} rows, first rows {rows[:8].tolist()}")
    bad = (got - ref).abs() > bound
    if bool(bad.any()):
        rows = bad.any(1).nonzero().flatten()
        r = int(rows[0])
        c = int(bad[r].nonzero()[0])
        raise AssertionError(f"{name}: {int(bad.sum())} values in {rows.numel()} rows out of bounds (first rows {rows[:8].tolist()}); "
                             f"[{r}, {c}]: kernel {float(got[r, c]):.7g}, fp64 reference {float(ref[r, c]):.7g}, bound {float(bound[r, c]):.3g}")


def ln_input(M, gen):
    """LayerNorm rows: N(0.3, 1.5^2), every 11th row with mean 50 and std 0.1 (a one-pass variance fails there), one constant row
    (variance 0: rstd = 1 / sqrt(eps))."""
    x = torch.randn(M, D, generator=gen, device=DEV, dtype=f64) * 1.5 + 0.3
    off = torch.arange(M, device=DEV) % 11 == 4
    x[off] = 50.0 + 0.1 * torch.randn(int(off.sum()), D, generator=gen, device=DEV, dtype=f64)
    x[(2 * M) // 3] = 3.0
    return x.to(f32)


# ------------------------------------------------------------------------------------------------ one case
def run(mode, H, M, seed, ctx=None, bias=True, scale=True, alias=False, pad=False, ln=None, nln=None, prj=None, lnb=False):
    """One launch of lafs_mlp_fused and every output it writes against the fp64 reference.
    ln: None or (ln_out wanted, ln_stats wanted) -- LayerNorm 2 in the prologue; nln: None or next_ln_stats wanted -- the next block's
    LayerNorm 1 in the epilogue; prj: None or (proj_bias and scales present) -- the projection in front (implies ln); lnb: the
    LayerNorm backward in the epilogue of BWD (seq_scale present iff `scale`); pad: every strided operand gets the smallest legal
    padding (8 elements where lafs_mlp_fused checks a multiple of 8, else 4)."""
    gen = torch.Generator(device=DEV)
    gen.manual_seed(seed)
    rn = lambda *s: torch.randn(*s, generator=gen, device=DEV, dtype=f64)
    p8, p4 = (8, 4) if pad else (0, 0)
    row_mul = torch.tensor([1.0, 0.01, 3.0], device=DEV, dtype=f64)[torch.arange(M, device=DEV) % 3][:, None]   # u near 0 and in both GELU tails
    nseq = len(SEQ_SCALE)
    row2seq = torch.randint(0, nseq, (M,), generator=gen, device=DEV, dtype=torch.int32)
    sc = torch.tensor(SEQ_SCALE, device=DEV, dtype=f32)
    s = sc.double()[row2seq.long()][:, None] if scale else torch.ones(M, 1, device=DEV, dtype=f64)
    kw = dict(seq_scale=sc, row2seq=row2seq) if scale else {}
    outs = []
    nm = f"{MODE_NAME[mode]} H={H} M={M}"

    if mode == BWD:
        dY = inp((rn(M, D) * row_mul).to(bf16), bf16, p8)
        Wa = inp((rn(H, D) / math.sqrt(D)).to(bf16), bf16, p8)                   # fc2.weight^T shadow [H, 384]
        Wb = inp((rn(D, H) / math.sqrt(H)).to(bf16), bf16, p8)                   # fc1.weight^T shadow [384, H]
        gd = torch.rand(M, H, generator=gen, device=DEV, dtype=f64) * 1.4 - 0.2
        gd[torch.rand(M, H, generator=gen, device=DEV) < 0.1] = 0.0
        gd = inp(gd.to(bf16), bf16, p8)
        out = Out(M, D, bf16, p8)
        du = Out(M, H, bf16, p8)
        ops.mlp_fused(dY, Wa, Wb, BWD, out=out.v, save_grad=gd, save_act=du.v, ctx=ctx)
        torch.cuda.synchronize()
        out.untouched(f"{nm}: dX")
        du.untouched(f"{nm}: du")
        dur, due, dxb, dxbe = mlp_bwd(dY.double(), Wa.double(), Wb.double(), gd.double())
        check(f"{nm}: du", du.v, dur, due)
        check(f"{nm}: dX", out.v, dxb, dxbe)
        if not lnb:
            return
        # the same launch with the LayerNorm backward in its epilogue: LN'(bf16(dX)) of the dX just checked (the header's contract:
        # what lafs_layernorm_bwd computes from the stored dX)
        x = ln_input(M, gen)
        xd = x.double()
        mean, var = xd.mean(1, keepdim=True), xd.var(1, unbiased=False, keepdim=True)
        st = torch.cat([mean, (var + EPS).rsqrt()], 1).to(f32)
        gam = (1.0 + 0.2 * rn(D)).to(f32)
        g0 = rn(M, D).to(f32)
        gio = Out(M, D, f32, p4)
        gio.v.copy_(g0)
        gbo = Out(M, D, bf16, p8)
        units = int(_lib.lib().lafs_mlp_fused_ln_parts(M))
        part = Out(units, 2 * D, f32)
        out2, du2 = Out(M, D, bf16, p8), Out(M, H, bf16, p8)
        lnb_args = (inp(x, f32, p4), inp(st, f32), gam, gio.v, gbo.v, part.v)
        ops.mlp_fused(dY, Wa, Wb, BWD, out=out2.v, save_grad=gd, save_act=du2.v, ctx=ctx, ln_bwd=lnb_args, **kw)
        torch.cuda.synchronize()
        out2.untouched(f"{nm}: out (not written with the LayerNorm backward)", whole=True)
        for name, o in (("du", du2), ("g_io", gio), ("gb", gbo), ("gamma/beta slots", part)):
            o.untouched(f"{nm} + LN backward: {name}")
        check(f"{nm} + LN backward: du", du2.v, dur, due)
        st64 = st.double()
        gn, gne, gb, gbe, dg, dge, db, dbe = layernorm_bwd(out.v.double(), torch.zeros_like(dxbe), xd, st64[:, :1], st64[:, 1:],
                                                           gam.double(), g0.double(), s)
        check(f"{nm}: g_io + dx", gio.v, gn, gne)
        check(f"{nm}: bf16(s g_io)", gbo.v, gb, gbe)
        slots = part.v.view(units, 2, D).double().sum(0)
        check(f"{nm}: dgamma (sum of the slots)", slots[0], dg, dge)
        check(f"{nm}: dbeta (sum of the slots)", slots[1], db, dbe)
        return

    Wa = inp((rn(H, D) * (2 / math.sqrt(D))).to(bf16), bf16, p8)                    # fc1.weight [H, 384]: u ~ 2 x row scale
    Wb = inp((rn(D, H) / math.sqrt(H)).to(bf16), bf16, p8)                          # fc2.weight [384, H]
    ba = (torch.rand(H, generator=gen, device=DEV, dtype=f64) * 4 - 2).to(f32) if bias else None
    bb = (0.5 * rn(D)).to(f32) if bias else None
    ba64 = None if ba is None else ba.double()
    bb64 = None if bb is None else bb.double()
    out = Out(M, D, f32, p8)
    outs.append(("out", out))
    call = dict(bias_a=ba, bias_b=bb, out=out.v, ctx=ctx, **kw)
    sg = sa = None
    if mode == SAVE:
        sg, sa = Out(M, H, bf16, p8), Out(M, H, bf16, p8)
        outs += [("save_grad", sg), ("save_act", sa)]
        call.update(save_grad=sg.v, save_act=sa.v)
    if ln is None and prj is None:
        X = inp((rn(M, D) * row_mul).to(bf16), bf16, p8)
        resid = rn(M, D).to(f32)
        if alias:
            out.v.copy_(resid)
            call["resid"] = out.v
        else:
            call["resid"] = inp(resid, f32, p4)
    else:
        X = None
        gam, bet = (1.0 + 0.2 * rn(D)).to(f32), (0.1 * rn(D)).to(f32)
        call["ln"] = (gam, bet, EPS)
        want_out, want_stats = ln if ln is not None else (True, True)
        lno = Out(M, D, bf16, p4) if want_out else None
        lns = Out(M, 2, f32) if want_stats else None
        if lno is not None:
            outs.append(("ln_out", lno))
            call["ln_out"] = lno.v
        if lns is not None:
            outs.append(("ln_stats", lns))
            call["ln_stats"] = lns.v
        if prj is None:
            resid = ln_input(M, gen)
            call["resid"] = inp(resid, f32, p4)
        else:
            x0 = ln_input(M, gen)
            po = inp((rn(M, D) * row_mul).to(bf16), bf16, p8)
            Wp = inp((rn(D, D) / math.sqrt(D)).to(bf16), bf16, p8)
            bp = (0.1 * rn(D)).to(f32) if prj else None
            sp = torch.tensor(SEQ_SCALE[::-1], device=DEV, dtype=f32) if prj else None
            x1 = Out(M, D, f32, p4)
            outs.append(("x1", x1))
            call["resid"] = x1.v
            call["proj"] = (po, Wp, bp, inp(x0, f32, p4), sp)
    if nln is not None:
        ngam, nbet = (1.0 + 0.2 * rn(D)).to(f32), (0.1 * rn(D)).to(f32)
        nlo = Out(M, D, bf16, p4)
        nls = Out(M, 2, f32) if nln else None
        outs.append(("next_ln_out", nlo))
        if nls is not None:
            outs.append(("next_ln_stats", nls))
        call["next_ln"] = (ngam, nbet, EPS, nlo.v, None if nls is None else nls.v)
    ops.mlp_fused(X, Wa, Wb, mode, **call)
    torch.cuda.synchronize()
    for name, o in outs:
        o.untouched(f"{nm}: {name}")

    Xe = None
    if X is not None:
        Xv, res = X.double(), resid.double()
    else:
        if prj is not None:
            pz, pze = gemm(po.double(), None, Wp.double(), None if bp is None else bp.double())
            ps = sp.double()[row2seq.long()][:, None] if sp is not None else torch.ones(M, 1, device=DEV, dtype=f64)
            x1r = x0.double() + ps * pz
            # the residual epilogue of the projection: two fp32 roundings
            check(f"{nm}: x1", x1.v, x1r, ps.abs() * pze + 2 * U * (x0.double().abs() + (ps * pz).abs()))
            res = x1.v.double()                     # LayerNorm 2 and the final residual read the x1 the kernel wrote
        else:
            res = resid.double()
        h, he, m, me, r, re = layernorm(res, gam.double(), bet.double())
        Xv, Xe = flip(h, he)
        if lno is not None:
            check(f"{nm}: ln_out", lno.v, Xv, Xe)
        if lns is not None:
            check(f"{nm}: ln_stats mean", lns.v[:, :1], m, me)
            check(f"{nm}: ln_stats rstd", lns.v[:, 1:], r, re)
    y, ye, a, ae, gdr, gde = mlp_fwd(Xv, Xe, Wa.double(), Wb.double(), ba64, bb64, res, s, None if sa is None else sa.v.double())
    check(f"{nm}: out", out.v, y, ye)
    if mode == SAVE:
        check(f"{nm}: save_act = gelu(u)", sa.v, a, ae)
        check(f"{nm}: save_grad = gelu'(u)", sg.v, gdr, gde)
    del a, ae, gdr, gde
    if nln is not None:
        h2, he2, m2, me2, r2, re2 = layernorm(out.v.double(), ngam.double(), nbet.double())     # of the rows the kernel wrote
        hr, hre = flip(h2, he2)
        check(f"{nm}: next_ln_out", nlo.v, hr, hre)
        if nls is not None:
            check(f"{nm}: next_ln_stats mean", nls.v[:, :1], m2, me2)
            check(f"{nm}: next_ln_stats rstd", nls.v[:, 1:], r2, re2)


def _seed(*k):
    return zlib.crc32(repr(k).encode())


# ------------------------------------------------------------------------------------------------ the grids
@pytest.mark.parametrize("H", H_ALL, ids=[f"H{h}" for h in H_ALL])
@pytest.mark.parametrize("mode", [FWD, SAVE, BWD], ids=["fwd", "save", "bwd"])
def test_every_accepted_hidden_width(mode, H):
    """Each of the 24 widths lafs_mlp_fused_supported accepts, at a ragged M of three units (the last with 3 active waves)."""
    run(mode, H, 128 * 2 + 16 * 2 + 5, _seed("w", mode, H))


@pytest.mark.parametrize("M", M_GRID, ids=[f"M={m}" for m in M_GRID])
@pytest.mark.parametrize("H", H_GRID, ids=[f"H{h}" for h in H_GRID])
@pytest.mark.parametrize("mode", [FWD, SAVE, BWD], ids=["fwd", "save", "bwd"])
def test_row_counts(mode, H, M):
    """Ragged units, idle waves and the launch split by the device's CU count (the default context)."""
    run(mode, H, rows_of(M), _seed("m", mode, H, M))


M_NULL = ["17", "ncu*128+64*5+25", "ncu*192+33"]


@pytest.mark.parametrize("M", M_NULL, ids=[f"M={m}" for m in M_NULL])
@pytest.mark.parametrize("H", [128, 704, 1536], ids=["H128", "H704", "H1536"])
@pytest.mark.parametrize("mode", [FWD, SAVE, BWD], ids=["fwd", "save", "bwd"])
def test_row_counts_without_a_context(mode, H, M):
    """ctx = NULL: one launch of 128-row units whatever M is."""
    run(mode, H, rows_of(M), _seed("n", mode, H, M), ctx=_NullCtx())


FWD_OPTIONS = {
    "no_bias": dict(bias=False),
    "no_seq_scale": dict(scale=False),
    "resid_is_out": dict(alias=True),
    "strided": dict(pad=True),
    "ln": dict(ln=(False, False)),
    "ln_out_stats": dict(ln=(True, True)),
    "next_ln": dict(ln=(False, False), nln=False),
    "next_ln_stats": dict(ln=(True, False), nln=True),
    "prj": dict(prj=True),
    "prj_no_bias_scale": dict(prj=False, ln=(False, True), scale=False),      # (and no ln_out: 24 fewer stores behind the first stages)
    "strided_ln_next_ln": dict(pad=True, ln=(True, True), nln=True),
    "strided_prj": dict(pad=True, prj=True, nln=True),
}
BWD_OPTIONS = {
    "strided": dict(pad=True),
    "ln_bwd": dict(lnb=True, scale=False),
    "ln_bwd_seq_scale": dict(lnb=True),
    "strided_ln_bwd": dict(lnb=True, pad=True),
}
OPT_CASES = [(m, o) for m in (FWD, SAVE) for o in FWD_OPTIONS] + [(BWD, o) for o in BWD_OPTIONS]
M_OPT = ["695", "ncu*128+64*5+25"]


@pytest.mark.parametrize("M", M_OPT, ids=[f"M={m}" for m in M_OPT])
@pytest.mark.parametrize("H", H_OPT, ids=[f"H{h}" for h in H_OPT])
@pytest.mark.parametrize("mode,opt", OPT_CASES, ids=[f"{MODE_NAME[m]}-{o}" for m, o in OPT_CASES])
def test_options(mode, opt, H, M):
    """Optional operands and the fusions: biases / seq_scale absent, the residual aliasing the output, strided views of every
    operand with a stride, LayerNorm 2 in the prologue with and without its by-products, the next block's LayerNorm 1 with and
    without statistics, the projection in front with and without bias / scale, the LayerNorm backward with and without seq_scale."""
    run(mode, H, rows_of(M), _seed("o", mode, opt, H, M), **(FWD_OPTIONS if mode != BWD else BWD_OPTIONS)[opt])


# ------------------------------------------------------------------------------------------------ the accepted domain
def test_supported_geometry_is_the_documented_one():
    sup = _lib.lib().lafs_mlp_fused_supported
    assert [H for H in range(0, 2049, 8) if sup(D, H, 1)] == H_ALL
    assert sup(383, 768, 100) == 0 and sup(768, 768, 100) == 0
    for H in (0, 64, 120, 1600):
        assert sup(D, H, 100) == 0, H
    assert sup(D, 768, 0) == 0 and sup(D, 768, -1) == 0 and sup(D, 768, 1 << 20) == 1
    parts = _lib.lib().lafs_mlp_fused_ln_parts
    assert [parts(m) for m in (0, 1, 128, 129, 256, 257)] == [0, 1, 1, 2, 2, 3]


def test_invalid_arguments_fail_loudly_and_launch_nothing():
    """Every rejected request returns an error naming the reason, and no kernel ran: the outputs keep their guard values."""
    M, H = 200, 256
    X, dY = torch.zeros(M, D, device=DEV, dtype=bf16), torch.zeros(M, D, device=DEV, dtype=bf16)
    Wa, Wb = torch.zeros(H, D, device=DEV, dtype=bf16), torch.zeros(D, H, device=DEV, dtype=bf16)
    resid = torch.zeros(M, D, device=DEV)
    st = torch.ones(M, 2, device=DEV)
    gam = torch.ones(D, device=DEV)
    sc, r2s = torch.ones(4, device=DEV), torch.zeros(M, dtype=torch.int32, device=DEV)
    out = torch.full((M, D), GUARD, device=DEV)
    outb = torch.full((M, D), GUARD, device=DEV, dtype=bf16)
    sg, sa = torch.full((M, H), GUARD, device=DEV, dtype=bf16), torch.full((M, H), GUARD, device=DEV, dtype=bf16)
    gio, part = torch.full((M, D), GUARD, device=DEV), torch.full((2, 2 * D), GUARD, device=DEV)
    p = lambda t: t.data_ptr()

    def args(mode=SAVE, **kw):
        a = _lib.MlpArgs()
        a.X, a.ldx, a.Wa, a.ldwa, a.Wb, a.ldwb, a.M, a.H, a.mode = p(X), D, p(Wa), D, p(Wb), H, M, H, mode
        a.resid, a.ldr, a.out, a.ldo = p(resid), D, p(out), D
        a.save_grad, a.ldsg, a.save_act, a.ldsa = p(sg), H, p(sa), H
        if mode == BWD:
            a.X, a.out, a.resid = p(dY), p(outb), None
        for k, v in kw.items():
            setattr(a, k, v)
        return a

    def lnb(**kw):
        d = dict(resid=p(resid), ldr=D, ln_gamma=p(gam), ln_stats=p(st), ln_g_io=p(gio), ldgio=D, ln_gb_out=p(outb), ldgb=D,
                 ln_part_out=p(part))
        d.update(kw)
        return args(BWD, **d)

    cases = [
        ("hidden width", args(H=120)), ("hidden width", args(H=1600)), ("hidden width", args(H=64)), ("hidden width", args(H=0)),
        ("hidden width", args(M=0)), ("bad mode", args(mode=3)),
        ("multiples of 8", args(ldx=D + 4)), ("multiples of 8", args(ldx=D - 8)), ("multiples of 8", args(ldwa=D + 4)),
        ("multiples of 8", args(ldwb=H - 8)), ("multiples of 8", args(ldwb=H + 4)), ("output stride", args(ldo=D + 4)),
        ("residual", args(ldr=D + 2)), ("gelu'", args(ldsg=H + 4)), ("gelu\\(u\\) / du", args(ldsa=H - 8)),
        ("residual", args(resid=None)), ("residual", args(FWD, resid=None, save_grad=None, save_act=None)),
        ("gelu'", args(BWD, save_grad=None)), ("du buffer", args(BWD, save_act=None)),
        ("seq_scale needs row2seq", args(seq_scale=p(sc))),
        ("null operand", args(X=None)), ("null operand", args(Wb=None)),
        ("LayerNorm prologue", args(ln_gamma=p(gam), ln_beta=None)),
        ("next block", args(next_ln_gamma=p(gam), next_ln_beta=p(gam), next_ln_out=None)),
        ("projection prologue", args(ln_gamma=p(gam), ln_beta=p(gam), proj_x=p(X), ldpx=D + 4, proj_w=p(Wa), ldpw=D, proj_resid=p(resid), ldpr=D)),
        ("proj_scale needs row2seq", args(ln_gamma=p(gam), ln_beta=p(gam), proj_x=p(X), ldpx=D, proj_w=p(Wa), ldpw=D, proj_resid=p(resid),
                                          ldpr=D, proj_scale=p(sc))),
        ("statistics", lnb(ln_stats=None)), ("statistics", lnb(resid=None)),
        ("gradient stream", lnb(ldgb=D + 4)), ("gradient stream", lnb(ln_part_out=None)),
        ("seq_scale needs row2seq", lnb(seq_scale=p(sc))),
    ]
    torch.cuda.synchronize()
    for why, a in cases:
        with pytest.raises(_lib.LafsHipError, match=why):
            _lib.call("lafs_mlp_fused", C.byref(a))
    with pytest.raises(_lib.LafsHipError, match="null arguments"):
        _lib.call("lafs_mlp_fused", None)
    torch.cuda.synchronize()
    g = torch.tensor(GUARD, device=DEV)
    for name, t in (("out", out), ("bf16 out", outb), ("save_grad", sg), ("save_act", sa), ("g_io", gio), ("slots", part)):
        assert bool((t == g.to(t.dtype)).all()), f"{name} written by a rejected call"
    # the same arguments with nothing wrong run (the cases above fail for the one reason each names)
    _lib.call("lafs_mlp_fused", C.byref(args(seq_scale=p(sc), row2seq=p(r2s))))
    _lib.call("lafs_mlp_fused", C.byref(lnb()))
    torch.cuda.synchronize()
    assert bool((out == 0).all()) and bool((part == 0).all())
