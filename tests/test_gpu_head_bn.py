"""lafs_bn1d_gelu_fwd / lafs_bn1d_gelu_bwd (csrc/head_bn.hip: BatchNorm1d + GELU of DINOHead(use_bn=True)) against fp64, element by
element, inside the operation-count bounds of tests/head_bn_cases.py (which never look at what a kernel returns; test_head_bn_host.py
shows that they are tight and fail seeded faults).  u, da, a and du are [n, D] views of NaN-filled [n + 3, ld] buffers: the ld padding
and the guard rows must still be NaN after a call.  Column 0 is constant over the rows, column 1 has mean 1000 and spread 1e-2."""
import pytest
import torch

pytestmark = pytest.mark.gpu

import fp64_bounds as fb  # noqa: E402
import head_bn_cases as hc  # noqa: E402
from lafs_cvpr2024_amd import _lib, ops  # noqa: E402

DEV = "cuda"
f32, bf16 = torch.float32, torch.bfloat16
GUARD = 3


def bits(t):
    t = t.detach().contiguous()
    return (t.view(torch.int16) if t.dtype == bf16 else t.view(torch.int32)).cpu()


def padded(t, ld, dtype=f32):
    """t [n, D] on the device as a view of a NaN-filled [n + GUARD, ld] buffer (t None: all NaN).  Returns (view, buffer)."""
    n, D = t if isinstance(t, tuple) else t.shape
    buf = torch.full((n + GUARD, ld), float("nan"), device=DEV, dtype=dtype)
    if not isinstance(t, tuple):
        buf[:n, :D] = t.to(DEV)
    return buf[:n, :D], buf


def guards_untouched(buf, n, D):
    return bool(torch.isnan(buf[n:]).all()) and bool(torch.isnan(buf[:, D:]).all())


def run_forward(c, n, D, ld, training):
    u, ubuf = padded(c["u"], ld)
    a, abuf = padded((n, D), ld, bf16)
    rm, rv = c["rm"].to(DEV), c["rv"].to(DEV)
    _, mean, rstd = ops.bn1d_gelu_fwd(u, c["gamma"].to(DEV), c["beta"].to(DEV), hc.EPS, hc.MOM, training, rm, rv, out=a)
    torch.cuda.synchronize()
    assert guards_untouched(abuf, n, D) and guards_untouched(ubuf, n, D), "pad columns / guard rows were written"
    assert torch.equal(bits(u), bits(c["u"])), "the input was written"
    return dict(a=a, save_mean=mean, save_rstd=rstd, running_mean=rm, running_var=rv), u


def run_backward(c, n, D, ld, training, accumulate, fw, u):
    da, dabuf = padded(c["da"], ld)
    du, dubuf = padded((n, D), ld, bf16)
    dg = c["old_dg"].to(DEV) if accumulate else torch.full((D,), float("nan"), device=DEV)
    db = c["old_db"].to(DEV) if accumulate else torch.full((D,), float("nan"), device=DEV)
    ops.bn1d_gelu_bwd(da, u, fw["save_mean"], fw["save_rstd"], c["gamma"].to(DEV), c["beta"].to(DEV), training, dg, db, accumulate=accumulate,
                      out=du)
    torch.cuda.synchronize()
    assert guards_untouched(dubuf, n, D) and guards_untouched(dabuf, n, D), "pad columns / guard rows were written"
    assert torch.equal(bits(da), bits(c["da"])) and torch.equal(bits(u), bits(c["u"])), "an input was written"
    return dict(du=du, dgamma=dg, dbeta=db)


@pytest.mark.parametrize("n,D,ld", hc.SHAPES, ids=lambda v: str(v))
@pytest.mark.parametrize("training", [True, False], ids=["train", "eval"])
def test_forward_and_backward_against_fp64(n, D, ld, training):
    c = hc.inputs(n, D)
    tag = f"bn1d_gelu {'train' if training else 'eval'} {n}x{D}/{ld}"
    fw, u = run_forward(c, n, D, ld, training)
    again, _ = run_forward(c, n, D, ld, training)
    ref = hc.forward_reference(c, training)
    fb.check(f"{tag} a", fw["a"].float().cpu(), *ref["a"], is16=True)
    for k in ("save_mean", "save_rstd", "running_mean", "running_var"):
        fb.check(f"{tag} {k}", fw[k].cpu(), *ref[k])
    for k in fw:
        assert torch.equal(bits(fw[k]), bits(again[k])), f"{k}: two runs differ"
    if training:
        assert float(fw["save_rstd"][0]) == pytest.approx(hc.f32val(hc.EPS) ** -0.5, rel=1e-6)         # the constant column
        assert not torch.equal(bits(fw["running_mean"]), bits(c["rm"]))
    else:                                                                                              # eval updates nothing
        assert torch.equal(bits(fw["running_mean"]), bits(c["rm"])) and torch.equal(bits(fw["running_var"]), bits(c["rv"]))
    for accumulate in (False, True):
        bw = run_backward(c, n, D, ld, training, accumulate, fw, u)
        bw2 = run_backward(c, n, D, ld, training, accumulate, fw, u)
        rb = hc.backward_reference(c, training, accumulate)
        fb.check(f"{tag} acc={int(accumulate)} du", bw["du"].float().cpu(), *rb["du"], is16=True)
        fb.check(f"{tag} acc={int(accumulate)} dgamma", bw["dgamma"].cpu(), *rb["dgamma"])
        fb.check(f"{tag} acc={int(accumulate)} dbeta", bw["dbeta"].cpu(), *rb["dbeta"])
        for k in bw:
            assert torch.equal(bits(bw[k]), bits(bw2[k])), f"{k}: two runs differ"


def test_statistics_are_those_of_bn1d_fwd_bit_for_bit():
    """One arithmetic serves both heads (csrc/bn_rows.hpp): save_mean, save_rstd and the running buffers of the fused kernel carry the
    bits of lafs_bn1d_fwd on the same rows."""
    n, D, ld = 37, 200, 208
    c = hc.inputs(n, D)
    fw, u = run_forward(c, n, D, ld, True)
    rm, rv = c["rm"].to(DEV), c["rv"].to(DEV)
    _, mean, rstd = ops.bn1d_fwd(u, c["gamma"].to(DEV), c["beta"].to(DEV), hc.EPS, hc.MOM, True, rm, rv)
    for k, v in (("save_mean", mean), ("save_rstd", rstd), ("running_mean", rm), ("running_var", rv)):
        assert torch.equal(bits(fw[k]), bits(v)), k


def test_one_row_is_refused_in_training_and_works_in_eval():
    D = 64
    c = hc.inputs(2, D)
    u = c["u"][:1].to(DEV).contiguous()
    rm, rv = c["rm"].to(DEV), c["rv"].to(DEV)
    a = torch.full((1, D), float("nan"), device=DEV, dtype=bf16)
    with pytest.raises(_lib.LafsHipError, match="more than one row"):
        ops.bn1d_gelu_fwd(u, c["gamma"].to(DEV), c["beta"].to(DEV), hc.EPS, hc.MOM, True, rm, rv, out=a)
    torch.cuda.synchronize()
    assert bool(torch.isnan(a).all()) and torch.equal(bits(rm), bits(c["rm"])), "a refused call launched"
    dg, db = torch.zeros(D, device=DEV), torch.zeros(D, device=DEV)
    with pytest.raises(_lib.LafsHipError, match="more than one row"):
        ops.bn1d_gelu_bwd(u, u, rm, rv, c["gamma"].to(DEV), c["beta"].to(DEV), True, dg, db)
    one = {k: (v[:1] if v.dim() == 2 else v) for k, v in c.items()}
    got, _, rstd = ops.bn1d_gelu_fwd(u, c["gamma"].to(DEV), c["beta"].to(DEV), hc.EPS, hc.MOM, False, rm, rv)
    fb.check("bn1d_gelu eval 1 row a", got.float().cpu(), *hc.forward_reference(one, False)["a"], is16=True)
    assert torch.equal(bits(rm), bits(c["rm"])) and torch.equal(bits(rv), bits(c["rv"]))
