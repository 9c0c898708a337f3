"""lafs_koleo_fwd_bwd (csrc/koleo.hip) against the fp64 oracle of tests/koleo_cases.py, element by element, on every case of its grid
(which names the code path every shape is there for).  The C entry point is called directly.  x, dx, loss, nn and the workspace --
sized by the library's own query -- each sit inside a larger poisoned buffer: x and dx at the row stride the case prescribes with NaN
behind column D, everything between guard elements; whatever lies outside an output's owned region must be bit-identical afterwards.
The neighbours are judged in two steps (koleo_cases.judge): admissible, then loss and gradient against the oracle evaluated with the
kernel's own neighbours, so that no row is left out.  tests/test_koleo_host.py shows on the CPU that the bounds mean something and
reject seeded faults.  Run with -s for each case's worst |error| / bound."""
import ctypes as C

import pytest
import torch

pytestmark = pytest.mark.gpu

from lafs_cvpr2024_amd import _lib, ops  # noqa: E402
from lafs_cvpr2024_amd._lib import call  # noqa: E402
from lafs_cvpr2024_amd.koleo_loss import KoLeoLoss  # noqa: E402

import fp64_bounds as fb  # noqa: E402
import koleo_cases as kc  # noqa: E402
from fp64_bounds import U, f32, f64  # noqa: E402

DEV = "cuda"
GV = 16                                  # guard elements on both sides (64 bytes: the owned region stays 16-byte aligned)
i32 = torch.int32


def _p(t):
    return None if t is None else C.c_void_p(t.data_ptr())


class Buf:
    """[rows, cols] at row stride ld inside a flat poisoned buffer (NaN, or -7 for integers) between GV guard elements.  arm() after
    pre-filling; intact() demands every element outside the owned columns bit-identical afterwards."""

    def __init__(self, rows, cols, ld, dtype=f32, src=None):
        poison = float("nan") if dtype.is_floating_point else -7
        self.buf = torch.full((GV + rows * ld + GV,), poison, device=DEV, dtype=dtype)
        self.v = self.buf[GV:GV + rows * ld].view(rows, ld)[:, :cols]
        self.owned = torch.zeros(self.buf.shape, dtype=torch.bool, device=DEV)
        self.owned[GV:GV + rows * ld].view(rows, ld)[:, :cols] = True
        if src is not None:
            self.v.copy_(src)
        self.arm()

    def arm(self):
        self.before = self.buf.view(i32).clone()
        return self

    def intact(self, name):
        bad = (self.buf.view(i32) != self.before) & ~self.owned
        assert not bool(bad.any()), f"{name}: {int(bad.sum())} elements outside the owned region were written, first at flat index {int(bad.nonzero()[0]) - GV}"


def _ws(c):
    n = int(_lib.lib().lafs_koleo_workspace_bytes(c["G"], c["rows"], c["D"]))
    assert n > 0 and n % 4 == 0
    return Buf(1, n // 4, n // 4)


def _run(c, d, with_nn=None):
    """One call on fresh buffers.  Returns (loss, nn or None, dx or None) as device tensors after the guards were checked, and x's
    buffer bits unchanged."""
    R, D, cid = c["G"] * c["rows"], c["D"], c["id"]
    x = Buf(R, D, c["ldx"], src=d["x"])
    dx = Buf(R, D, c["lddx"], src=d["dx_old"] if c["acc"] else None) if c["dx"] else None
    loss, ws = Buf(1, c["G"], c["G"]), _ws(c)
    nn = Buf(1, R, R, i32) if (c["nn"] if with_nn is None else with_nn) else None
    call("lafs_koleo_fwd_bwd", _p(x.v), c["ldx"], c["G"], c["rows"], D, 1e-8, c["scale"], _p(loss.v), _p(nn.v if nn else None),
         _p(dx.v if dx else None), c["lddx"] if dx else 0, 1 if c["acc"] else 0, _p(ws.v))
    torch.cuda.synchronize()
    for name, b in (("loss", loss), ("nn", nn), ("dx", dx), ("workspace", ws)):
        if b is not None:
            b.intact(f"{cid}: {name}")
    assert torch.equal(x.buf.view(i32), x.before), f"{cid}: x was written"
    return loss.v[0].clone(), None if nn is None else nn.v[0].clone(), None if dx is None else dx.v.clone()


@pytest.mark.parametrize("c", kc.CASES, ids=[c["id"] for c in kc.CASES])
def test_koleo_against_fp64(c):
    d = {k: v.to(DEV) for k, v in kc.inputs(c).items()}
    loss, nn, dx = _run(c, d)
    loss2, nn2, dx2 = _run(c, d, with_nn=True)                       # two calls give identical bits; nn NULL changes nothing else
    assert torch.equal(loss.view(i32), loss2.view(i32)), f"{c['id']}: the loss differs between two calls"
    assert nn is None or torch.equal(nn, nn2), f"{c['id']}: nn differs between two calls"
    assert dx is None or torch.equal(dx.view(i32), dx2.view(i32)), f"{c['id']}: dx differs between two calls"
    kc.judge(c, d, loss, nn2, dx)


def test_module_forward_and_backward():
    """KoLeoLoss forward + backward() with a grad_output != 1: the saved gradient times 2.5, one more rounding."""
    c = kc.BY_ID["64x384-g2-step"]
    d = kc.inputs(c)
    x = d["x"][:c["rows"]].to(DEV, f32).requires_grad_(True)
    loss = KoLeoLoss()(x)
    (2.5 * loss).backward()
    _, nn = ops.koleo(x.detach(), 1, c["rows"])
    torch.cuda.synchronize()
    one = dict(c, G=1, acc=False, scale=1.0, id="module")
    dd = dict(x=x.detach().double(), dx_old=None)
    kc.judge(one, dd, loss.detach().reshape(1), nn, None)
    r, re = kc.reference(dd["x"], 1, c["rows"], nn.long())["dx"]
    fb.check("module: x.grad", x.grad, 2.5 * r, 2.5 * re + U * (2.5 * r).abs())
    with pytest.raises(_lib.LafsHipError):
        ops.koleo(torch.zeros(8, 64), 1, 8)                          # host tensors: no CPU fallback


def test_invalid_arguments_are_refused_and_nothing_is_written():
    h = _lib.lib()

    def refused(rows=4, D=64, G=2, ldx=None, lddx=None, off=0):
        ldx, lddx = ldx or D, lddx or D
        R = max(G, 1) * rows
        x = Buf(R, D, max(ldx, D), src=torch.randn(R, D))
        dx, loss, nn = Buf(R, D, max(lddx, D)), Buf(1, G, G), Buf(1, R, R, i32)
        ws = Buf(1, R * (D + 3), R * (D + 3))
        rc = h.lafs_koleo_fwd_bwd(C.c_void_p(x.v.data_ptr() + off), ldx, G, rows, D, 1e-8, 1.0, _p(loss.v), _p(nn.v), _p(dx.v), lddx, 0, _p(ws.v), None)
        torch.cuda.synchronize()
        assert rc < 0 and h.lafs_last_error(), (rows, D, G, ldx, lddx, off, rc)
        for b in (dx, loss, nn, ws):
            assert torch.equal(b.buf.view(i32), b.before)

    refused(rows=1)
    refused(D=6)
    refused(rows=1025)
    refused(D=1028)
    refused(G=0)
    refused(ldx=66)                                                   # misaligned row stride
    refused(lddx=62)
    refused(off=4)                                                    # x not 16-byte aligned
    assert h.lafs_koleo_workspace_bytes(1, 1, 64) < 0 and h.lafs_koleo_workspace_bytes(1, 2, 6) < 0
    assert h.lafs_koleo_workspace_bytes(2, 64, 384) == 2 * 64 * (384 + 3) * 4
