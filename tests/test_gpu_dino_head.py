"""Everything after the DINO head's bottleneck against the fp64 oracle of tests/fp64_bounds.py, element by element: lafs_l2norm_fwd /
_bwd, lafs_weightnorm_fwd / _bwd (head.hip), lafs_dino_loss_fwd_bwd, lafs_colsum_f32, lafs_center_ema (dino_loss.hip) and
lafs_dino_head_loss (dino_head_loss.hip).  The grids (tests/dino_cases.py) name the code path every shape is there for.

The C entry points are called directly.  Matrix operands with a row stride are column slices of NaN-filled buffers (gemm_cases.inp, or
`Img` where the case prescribes the stride), so whatever lies behind column K is NaN; every output is armed and must be bit-identical
outside its owned region afterwards (gemm_cases.Out, `Img`), which includes the columns K..ldg of the unfused gradient; vectors and
contiguous images -- the centre, inv_norm, colsum, loss and the workspace, sized by the library's own query -- sit between guard
elements (`Vec`).  Each backward is judged on the statistics its own forward stored.  tests/test_oracle_dino_host.py shows on the CPU
that these bounds mean something and reject seeded faults."""
import ctypes as C

import pytest
import torch

pytestmark = pytest.mark.gpu

from lafs_cvpr2024_amd import _lib  # noqa: E402
from lafs_cvpr2024_amd._lib import call  # noqa: E402

import dino_cases as dc  # noqa: E402
import fp64_bounds as fb  # noqa: E402
import gemm_cases as gc  # noqa: E402
from fp64_bounds import bf16, f32, f64  # noqa: E402

DEV = "cuda"
GV = 16                                  # guard elements on both sides of a vector
NAN = float("nan")


def _p(t):
    return None if t is None else C.c_void_p(t.data_ptr())


def _bits(t):
    return t.view(torch.int32 if t.element_size() == 4 else torch.int16)


class Img:
    """[rows, cols] at the row stride ld the case prescribes, inside a flat NaN-filled buffer between GV guard elements.  As an
    operand: fill .v, the columns cols..ld stay NaN.  As an output: arm() after pre-filling, intact() demands every element outside
    the owned columns bit-identical afterwards (guards and row tails alike)."""

    def __init__(self, rows, cols, ld, dtype, src=None):
        self.buf = torch.full((GV + rows * ld + GV,), NAN, device=DEV, dtype=dtype)
        self.v = self.buf[GV:GV + rows * ld].view(rows, ld)[:, :cols]
        self.owned = torch.zeros(self.buf.shape, dtype=torch.bool, device=DEV)
        self.owned[GV:GV + rows * ld].view(rows, ld)[:, :cols] = True
        self.before = None
        if src is not None:
            self.v.copy_(src)

    def arm(self):
        self.before = _bits(self.buf).clone()
        return self

    def intact(self, name):
        bad = (_bits(self.buf) != self.before) & ~self.owned
        assert not bool(bad.any()), f"{name}: {int(bad.sum())} elements outside the owned region were written, first at flat index {int(bad.nonzero()[0]) - GV}"


def Vec(n, dtype=f32, src=None):
    """A contiguous vector (or image) of n elements between guard elements, armed."""
    return Img(1, n, n, dtype, None if src is None else src.reshape(1, -1)).arm()


def vec(o):
    return o.v[0]


def to_dev(d):
    return {k: v.to(DEV) for k, v in d.items()}


def ids(cases):
    return [c["id"] for c in cases]


# ------------------------------------------------------------------------------------------------ head.hip
@pytest.mark.parametrize("c", dc.ROW_CASES, ids=ids(dc.ROW_CASES))
def test_l2norm_forward_and_backward(c):
    R, D, cid = c["rows"], c["D"], c["id"]
    d = dc.row_inputs(c)
    dd = to_dev(d)
    x = gc.inp(d["x"], f32, DEV)
    y = gc.Out(R, D, bf16, DEV).arm()
    inv = Vec(R)
    call("lafs_l2norm_fwd", _p(x), x.stride(0), _p(y.v), y.v.stride(0), _p(inv.v), R, D)
    torch.cuda.synchronize()
    inv.intact(f"{cid}: inv_norm"); y.intact(f"{cid}: y")
    exp = dc.l2_fwd_expected(c, dd)
    fb.check(f"{cid}: inv_norm", vec(inv)[:, None], *exp["inv"])
    fb.check(f"{cid}: y", y.v, *exp["y16"], True)
    dy = gc.inp(d["dy"], f32, DEV, off=4)
    dx = gc.Out(R, D, f32, DEV, off=4).arm()
    call("lafs_l2norm_bwd", _p(x), x.stride(0), _p(dy), dy.stride(0), _p(inv.v), _p(dx.v), dx.v.stride(0), R, D)
    torch.cuda.synchronize()
    inv.intact(f"{cid}: inv_norm (backward)"); dx.intact(f"{cid}: dx")
    fb.check(f"{cid}: dx", dx.v, *dc.l2_bwd_expected(c, dd, vec(inv).double()[:, None]))


@pytest.mark.parametrize("c", dc.ROW_CASES, ids=ids(dc.ROW_CASES))
def test_weightnorm_backward(c):
    K, D, cid = c["rows"], c["D"], c["id"]
    d = dc.row_inputs(c, weight=True)
    dd = to_dev(d)
    v, g, dw = Vec(K * D, src=dd["x"]), Vec(K, src=dd["g"]), Vec(K * D, src=dd["dy"])
    w, inv = Vec(K * D, bf16), Vec(K)
    call("lafs_weightnorm_fwd", _p(v.v), _p(g.v), K, K, D, _p(w.v), None, 0, _p(inv.v))
    dv = Img(1, K * D, K * D, f32, dd["dv_old"].reshape(1, -1) if c["acc"] else None).arm()
    dg = Img(1, K, K, f32, dd["dg_old"].reshape(1, -1) if c["acc"] else None).arm() if c["dg"] else None
    call("lafs_weightnorm_bwd", _p(dw.v), _p(v.v), _p(g.v), _p(inv.v), K, D, _p(dv.v), _p(dg and dg.v), int(c["acc"]))
    torch.cuda.synchronize()
    for name, o in (("v", v), ("g", g), ("dw", dw), ("w", w), ("inv_norm", inv), ("dv", dv), ("dg", dg)):
        if o is not None:
            o.intact(f"{cid}: {name}")
    fwd = fb.weightnorm_fwd(dd["x"], dd["g"])
    fb.check(f"{cid}: inv_norm", vec(inv)[:, None], *fwd["inv"])
    fb.check(f"{cid}: w", vec(w).view(K, D), *fwd["w16"], True)
    exp = dc.wn_bwd_expected(c, dd, vec(inv).double()[:, None])
    fb.check(f"{cid}: dv", vec(dv).view(K, D), *exp["dv"])
    if dg is not None:
        fb.check(f"{cid}: dg", vec(dg)[:, None], *exp["dg"])


@pytest.mark.parametrize("c", dc.WN_CASES, ids=ids(dc.WN_CASES))
def test_weightnorm_forward(c):
    K, Kpad, D, cid = c["K"], c["Kpad"], c["D"], c["id"]
    dd = to_dev(dc.wn_inputs(c))
    v, g = Vec(K * D, src=dd["v"]), Vec(K, src=dd["g"])
    w, inv = Vec(Kpad * D, bf16), Vec(K)
    wt = gc.Out(D, Kpad, bf16, DEV).arm() if c["wt"] else None
    call("lafs_weightnorm_fwd", _p(v.v), _p(g.v), K, Kpad, D, _p(w.v), _p(wt and wt.v), wt.v.stride(0) if wt else 0, _p(inv.v))
    torch.cuda.synchronize()
    for name, o in (("v", v), ("g", g), ("w", w), ("inv_norm", inv), ("w_t", wt)):
        if o is not None:
            o.intact(f"{cid}: {name}")
    exp = dc.wn_fwd_expected(c, dd)
    W = vec(w).view(Kpad, D)
    fb.check(f"{cid}: inv_norm", vec(inv)[:, None], *exp["inv"])
    fb.check(f"{cid}: w", W[:K], *exp["w16"], True)
    assert bool((_bits(W[K:]) == 0).all()), f"{cid}: a pad row of w is not zero"
    if wt is not None:
        assert torch.equal(_bits(wt.v), _bits(W.t().contiguous())), f"{cid}: w_t is not the transpose of w"


# ------------------------------------------------------------------------------------------------ dino_loss.hip
def run_loss(c, dd):
    nc, B, K, ld, ldg = c["ncrops"], c["B"], c["K"], c["ld"], c["ldg"]
    s, t = Img(nc * B, K, ld, f32, dd["s"]).arm(), Img(2 * B, K, ld, f32, dd["t"]).arm()
    center, loss = Vec(K, src=dd["center"]), Vec(1)
    ws = Vec(int(_lib.lib().lafs_dino_loss_workspace(nc, B, K)))
    grad = Img(nc * B, K, ldg, bf16 if c["g16"] else f32).arm()
    temps = Vec(2, src=torch.tensor([c["ts"], c["tt"]], dtype=f32)) if c["dev"] else None
    hs, ht = dc.host_temps(c)
    call("lafs_dino_loss_fwd_bwd", _p(s.v), _p(t.v), ld, _p(center.v), nc, B, K, hs, ht, _p(loss.v), _p(grad.v), ldg, int(c["g16"]),
         c["scale"], _p(ws.v), _p(temps and temps.v))
    torch.cuda.synchronize()
    for name, o in (("student", s), ("teacher", t), ("centre", center), ("loss", loss), ("workspace", ws), ("grad", grad), ("dev_temps", temps)):
        if o is not None:
            o.intact(f"{c['id']}: {name}")
    return loss, grad, ws


@pytest.mark.parametrize("c", dc.LOSS_CASES, ids=ids(dc.LOSS_CASES))
def test_dino_loss(c):
    nc, B, K, cid = c["ncrops"], c["B"], c["K"], c["id"]
    dd = to_dev(dc.loss_inputs(c))
    loss, grad, ws = run_loss(c, dd)
    exp = dc.loss_expected(c, dd)
    w = vec(ws)
    rs, rt = nc * B, 2 * B
    fb.check(f"{cid}: student lse", w[:2 * rs].view(rs, 2)[:, 1:], *exp["lse_s"])
    fb.check(f"{cid}: teacher lse", w[2 * rs:2 * (rs + rt)].view(rt, 2)[:, 1:], *exp["lse_t"])
    dots = w[2 * (rs + rt):].view(-1, B, nc).double().sum(0).t().reshape(rs, 1)           # [chunk][b][v] -> rows v B + b
    fb.check(f"{cid}: dots", dots, *exp["dots"])
    fb.check(f"{cid}: loss", vec(loss), *exp["loss"])
    fb.check(f"{cid}: grad", grad.v, *exp["grad"], c["g16"])


@pytest.mark.parametrize("c", dc.COLSUM_CASES, ids=ids(dc.COLSUM_CASES))
def test_colsum_f32(c):
    rows, K = c["rows"], c["K"]
    dd = to_dev(dc.colsum_inputs(c))
    x, out = Img(rows, K, c["ld"], f32, dd["x"]).arm(), Vec(K)
    call("lafs_colsum_f32", _p(x.v), c["ld"], rows, K, _p(out.v))
    torch.cuda.synchronize()
    x.intact(f"{c['id']}: x"); out.intact(f"{c['id']}: colsum")
    fb.check(f"colsum {c['id']}", vec(out), *fb.colsum(dd["x"]))


@pytest.mark.parametrize("c", dc.EMA_CASES, ids=ids(dc.EMA_CASES))
def test_center_ema(c):
    K = c["K"]
    dd = to_dev(dc.ema_inputs(c))
    center, cs = Vec(K, src=dd["center"]), Vec(K, src=dd["colsum"])
    call("lafs_center_ema", _p(center.v), _p(cs.v), K, c["inv_rows"], c["m"])
    torch.cuda.synchronize()
    center.intact(f"{c['id']}: centre"); cs.intact(f"{c['id']}: colsum")
    fb.check(f"centre {c['id']}", vec(center), *dc.ema_expected(c, dd))


# ------------------------------------------------------------------------------------------------ dino_head_loss.hip
@pytest.mark.parametrize("c", dc.HEAD_CASES, ids=ids(dc.HEAD_CASES))
def test_fused_head_loss(c):
    nc, B, K, Kpad, ldg, cid = c["ncrops"], c["B"], c["K"], c["Kpad"], c["ldg"], c["id"]
    dd = to_dev(dc.head_inputs(c))
    rs = nc * B
    ops = {k: Vec(dd[k].numel(), bf16, dd[k]) for k in ("zs", "zt", "ws", "wt")}
    center, loss = Vec(K, src=dd["center"]), Vec(1)
    colsum = Vec(K) if c["colsum"] else None
    ws = Vec(int(_lib.lib().lafs_dino_head_loss_workspace(nc, B, K)))
    grad = Img(rs, Kpad, ldg, bf16).arm()
    temps = Vec(2, src=torch.tensor([c["ts"], c["tt"]], dtype=f32)) if c["dev"] else None
    hs, ht = dc.host_temps(c)

    def run():
        call("lafs_dino_head_loss", _p(ops["zs"].v), _p(ops["zt"].v), _p(ops["ws"].v), _p(ops["wt"].v), 256, _p(center.v), nc, B, K, Kpad,
             hs, ht, _p(temps and temps.v), _p(loss.v), _p(grad.v), ldg, c["scale"], _p(colsum and colsum.v), _p(ws.v))
        torch.cuda.synchronize()
        for name, o in list(ops.items()) + [("centre", center), ("loss", loss), ("colsum", colsum), ("workspace", ws), ("grad", grad), ("dev_temps", temps)]:
            if o is not None:
                o.intact(f"{cid}: {name}")
        return [_bits(o.v).clone() for o in (loss, grad, colsum) if o is not None]

    first = run()
    exp = dc.head_expected(c, dd)
    fb.check(f"{cid}: loss", vec(loss), *exp["loss"])
    fb.check(f"{cid}: grad", grad.v[:, :K], *exp["grad"], True)
    assert bool((_bits(grad.v[:, K:]) == 0).all()), f"{cid}: a pad column of the gradient is not zero"
    if colsum is not None:
        fb.check(f"{cid}: colsum", vec(colsum), *exp["colsum"])
    for o in (loss, grad, colsum):
        if o is not None:
            o.v.fill_(NAN)
    again = run()
    assert all(torch.equal(a, b) for a, b in zip(first, again)), f"{cid}: the second run differs from the first"


# ------------------------------------------------------------------------------------------------ refusals (nothing is launched)
S = 768.0


def test_invalid_arguments_are_refused_and_nothing_is_written():
    Fb = lambda n: torch.full((n,), S, device=DEV, dtype=f32)
    Bb = lambda n: torch.full((n,), S, device=DEV, dtype=bf16)
    x, dy, dx, inv, g, w32 = Fb(8 * 1100), Fb(8 * 1100), Fb(8 * 1100), Fb(64), Fb(64), Fb(4096)
    y, w, wt = Bb(8 * 1100), Bb(64 * 1100), Bb(1100 * 64)
    loss, cen, ws, temps = Fb(1), Fb(4096), Fb(1 << 16), Fb(2)
    z, gr = Bb(2048 * 256), Bb(1 << 16)
    outs = (dx, inv, y, w, wt, loss, ws, gr, w32)

    def head(ncrops=2, B=2, dim=256, K=10, Kpad=16, ldg=16):
        call("lafs_dino_head_loss", _p(z), _p(z), _p(z), _p(z), dim, _p(cen), ncrops, B, K, Kpad, 0.1, 0.04, None, _p(loss), _p(gr), ldg, 1.0, None, _p(ws))

    def unfused(ncrops=2, B=2, K=10, ld=12, ldg=12):
        call("lafs_dino_loss_fwd_bwd", _p(x), _p(dy), ld, _p(cen), ncrops, B, K, 0.1, 0.04, _p(loss), _p(w32), ldg, 0, 1.0, _p(ws), None)

    refused = []
    for D in (6, 1028):                                                                            # D % 4 != 0, D > 1024
        refused += [lambda D=D: call("lafs_l2norm_fwd", _p(x), 1100, _p(y), 1100, _p(inv), 4, D),
                    lambda D=D: call("lafs_l2norm_bwd", _p(x), 1100, _p(dy), 1100, _p(inv), _p(dx), 1100, 4, D),
                    lambda D=D: call("lafs_weightnorm_fwd", _p(x), _p(g), 4, 8, D, _p(w), None, 0, _p(inv)),
                    lambda D=D: call("lafs_weightnorm_bwd", _p(dy), _p(x), _p(g), _p(inv), 4, D, _p(dx), None, 0)]
    refused += [lambda: call("lafs_weightnorm_fwd", _p(x), _p(g), 4, 8, 260, _p(w), _p(wt), 16, _p(inv)),      # w_t with D > 256
                lambda: call("lafs_weightnorm_fwd", _p(x), _p(g), 4, 12, 64, _p(w), _p(wt), 16, _p(inv)),       # w_t with Kpad % 8 != 0
                lambda: unfused(ncrops=1), lambda: unfused(ncrops=17), lambda: unfused(ld=8), lambda: unfused(ldg=8),
                lambda: head(ncrops=1), lambda: head(ncrops=17), lambda: head(B=65), lambda: head(dim=128), lambda: head(dim=512),
                lambda: head(Kpad=12, ldg=16), lambda: head(K=20, Kpad=16), lambda: head(ldg=8)]
    for i, fn in enumerate(refused):
        with pytest.raises(_lib.LafsHipError):
            fn()
    torch.cuda.synchronize()
    for t in outs:
        assert bool((t == S).all()), "an output was written by a refused call"
