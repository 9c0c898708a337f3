"""lafs_unfold_bf16 / lafs_fold_f32 (csrc/unfold.hip: fViT's nn.Unfold + transpose and its adjoint) and the two padding helpers
against torch.nn.functional.unfold / fold on the CPU.  The unfold comparison is exact: the kernel moves values and rounds them to bf16
once, the way lafs_patchify does (round to nearest even = torch's .to(bfloat16)).  The fold is an fp32 sum of at most t window entries
per pixel, compared with the fp64 sum under t * 2^-23 * sum|terms| per element."""
import pytest
import torch
import torch.nn.functional as F

pytestmark = pytest.mark.gpu

from fvit_cases import UNFOLD_CASES, windows  # noqa: E402
from lafs_cvpr2024_amd import _lib, ops  # noqa: E402
from lafs_cvpr2024_amd.ops import _p, call  # noqa: E402

DEV = "cuda"
bf16, f32, f64 = torch.bfloat16, torch.float32, torch.float64
GUARD = 4                           # sentinel rows in front of and behind the output
SENTINEL = 0x7B7B                   # bf16 bit pattern of the guard rows (and of the output before the launch)


def _ids(c):
    return "S%d_k%d_s%d_p%d" % c[:4]


def coded_image(B, S):
    """value = ((b * 3 + c) * S + y) * S + x + 1: a wrong index shows as another pixel's code (exact in fp32; bf16 keeps its top 8 bits)."""
    return (torch.arange(B * 3 * S * S, dtype=f32) + 1).view(B, 3, S, S)


def run_unfold(img, k, stride, pad):
    """The kernel's rows written into the middle of a sentinel-filled buffer: (rows bf16 [B n n, ldp] on the CPU, guards untouched?)."""
    B, _, S, _ = img.shape
    n, ldp = windows(S, k, stride, pad), ops.unfold_ld(k)
    rows = B * n * n
    buf = torch.full((rows + 2 * GUARD, ldp), SENTINEL, dtype=torch.int16, device=DEV)
    out = buf[GUARD:GUARD + rows].view(bf16)
    ops.unfold(img.to(DEV), k, stride, pad, out=out, ldp=ldp)
    torch.cuda.synchronize()
    host = buf.cpu()
    guards_ok = bool((host[:GUARD] == SENTINEL).all()) and bool((host[GUARD + rows:] == SENTINEL).all())
    return host[GUARD:GUARD + rows].view(bf16), guards_ok


def expected_rows(img, k, stride, pad):
    B = img.shape[0]
    cols = F.unfold(img, k, stride=stride, padding=pad).transpose(1, 2)       # [B, n n, 3 k^2], column (c, i, j)
    return cols.reshape(-1, 3 * k * k).to(bf16)


def explain(case, img, got, exp):
    """Name the first wrong element: its window, its tap, the pixel it should hold and the pixels whose value the kernel wrote."""
    S, k, stride, pad, B = case
    n, K3 = windows(S, k, stride, pad), 3 * k * k
    bad = (got[:, :K3].view(torch.int16) != exp.view(torch.int16)).nonzero()
    r, col = int(bad[0, 0]), int(bad[0, 1])
    b, wy, wx = r // (n * n), (r // n) % n, r % n
    c, i, j = col // (k * k), (col // k) % k, col % k
    y, x = wy * stride - pad + i, wx * stride - pad + j
    same = (img.to(bf16) == got[r, col]).nonzero()[:4].tolist()
    return (f"{len(bad)} wrong elements; first: row {r} = (b {b}, wy {wy}, wx {wx}), column {col} = (c {c}, i {i}, j {j}) should hold "
            f"img[{b}, {c}, {y}, {x}] = {float(exp[r, col])}, kernel wrote {float(got[r, col])} (pixels with that value: {same})")


@pytest.mark.parametrize("case", UNFOLD_CASES, ids=_ids)
@pytest.mark.parametrize("coded", [False, True], ids=["random", "coded"])
def test_unfold_matches_nn_unfold_exactly(case, coded):
    S, k, stride, pad, B = case
    torch.manual_seed(S * 100 + k)
    img = coded_image(B, S) if coded else torch.rand(B, 3, S, S) * 2 - 1
    got, guards_ok = run_unfold(img, k, stride, pad)
    exp = expected_rows(img, k, stride, pad)
    K3 = 3 * k * k
    assert got.shape == (B * windows(S, k, stride, pad) ** 2, ops.unfold_ld(k))
    assert guards_ok, "a guard row in front of or behind the output was written"
    assert bool((got[:, K3:].view(torch.int16) == 0).all()), "tail columns [3 k^2, ldp) must be exactly 0"
    assert torch.equal(got[:, :K3].view(torch.int16), exp.view(torch.int16)), explain(case, img, got, exp)


def test_unfold_8_8_0_is_patchify_bit_for_bit():
    torch.manual_seed(1)
    img = (torch.rand(3, 3, 16, 16) * 2 - 1).to(DEV)
    a = ops.unfold(img, 8, 8, 0)
    b = ops.patchify(img, _lib.PATCH_ORDER_CHW)
    assert a.shape == b.shape == (12, 192) and torch.equal(a.view(torch.int16), b.view(torch.int16))


@pytest.mark.parametrize("case", UNFOLD_CASES, ids=_ids)
def test_fold_is_the_adjoint_within_fp32_summation(case):
    S, k, stride, pad, B = case
    n, ldp, K3 = windows(S, k, stride, pad), ops.unfold_ld(k), 3 * k * k
    torch.manual_seed(S * 100 + k + 7)
    dp = torch.randn(B * n * n, ldp)                                          # (the tail columns are random too: they must be ignored)
    cols = dp[:, :K3].double().view(B, n * n, K3).transpose(1, 2)
    kw = dict(output_size=(S, S), kernel_size=k, stride=stride, padding=pad)
    ref, mag, t = F.fold(cols, **kw), F.fold(cols.abs(), **kw), F.fold(torch.ones_like(cols), **kw)
    bound = t * 2.0 ** -23 * mag                                              # an fp32 sum of at most t terms
    d = dp.to(DEV)
    outs = []
    for _ in range(2):
        out = torch.full((B, 3, S, S), float("nan"), device=DEV)              # written, not accumulated: no NaN may survive
        call("lafs_fold_f32", _p(d), ldp, B, S, k, stride, pad, _p(out))
        outs.append(out.cpu())
    got = outs[0]
    assert torch.equal(outs[0].view(torch.int32), outs[1].view(torch.int32)), "two runs differ"
    assert bool(torch.isfinite(got).all())
    err = (got.double() - ref).abs()
    print(f"fold {_ids(case)}: worst |err|/bound {float((err[bound > 0] / bound[bound > 0]).max()):.3f}, {int((t == 0).sum())} pixels under no window")
    assert bool((err <= bound).all()), (int((err > bound).sum()), (err > bound).nonzero()[0].tolist())
    assert bool((got[t == 0] == 0).all())
    if case[:4] == (18, 12, 8, 4):
        assert int((t == 0).sum()) == B * 3 * (18 * 18 - 16 * 16)             # bottom / right edges: covered by no window
    assert torch.equal(ops.fold(d, B, S, k, stride, pad).cpu().view(torch.int32), got.view(torch.int32))


@pytest.mark.parametrize("what,k,pad,ldp", [("pad >= k", 8, 8, 192), ("ldp % 32 != 0", 12, 4, 440), ("ldp < 3 k^2", 12, 4, 416)])
def test_bad_arguments_return_an_error_and_launch_nothing(what, k, pad, ldp):
    img = torch.zeros(1, 3, 16, 16, device=DEV)
    out = torch.full((64, 512), SENTINEL, dtype=torch.int16, device=DEV)
    h = _lib.lib()
    rc = h.lafs_unfold_bf16(_p(img), 1, 16, k, 8, pad, _p(out), ldp, None)
    assert rc < 0 and h.lafs_last_error(), what
    rc = h.lafs_fold_f32(_p(out), 192, 1, 16, 8, 8, 8, _p(img), None)          # pad >= k on the adjoint too
    assert rc < 0
    torch.cuda.synchronize()
    assert bool((out == SENTINEL).all()) and bool((img == 0).all())
    with pytest.raises(_lib.LafsHipError):
        call("lafs_unfold_bf16", _p(img), 1, 16, k, 8, pad, _p(out), ldp)


def test_pad_cast_and_add_cols():
    """lafs_pad_cast_bf16 (weight / ready patch vectors widened to ldp columns) and lafs_add_cols_f32 (the first 3 k^2 columns of the
    padded weight gradient into the arena): exact -- a rounding to bf16, and a single fp32 addition per element."""
    torch.manual_seed(3)
    src = torch.randn(37, 75)
    got = ops.pad_cast_bf16(src.to(DEV), 96).cpu()
    assert torch.equal(got[:, :75].view(torch.int16), src.to(bf16).view(torch.int16)) and bool((got[:, 75:].view(torch.int16) == 0).all())
    wide, dst = torch.randn(37, 96), torch.randn(37, 75)
    for acc in (True, False):
        d = dst.clone().to(DEV)
        ops.add_cols(wide.to(DEV), d, accumulate=acc)
        assert torch.equal(d.cpu(), dst + wide[:, :75] if acc else wide[:, :75].clone())
