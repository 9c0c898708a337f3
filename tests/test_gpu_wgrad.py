"""The reductions over the token axis -- lafs_gemm_tn_acc, lafs_gemm_tn_part + lafs_reduce_partials (csrc/gemm.hip), lafs_wgrad,
lafs_wgrad_f16, lafs_wgrad_group (csrc/wgrad.hip), lafs_colsum_bf16_acc, lafs_sum_slices -- against the fp64 oracle of
tests/fp64_bounds.py, element by element, with the guard and stride discipline of tests/test_gpu_gemm.py: operands are column slices
of NaN-filled buffers, outputs sit between guard rows and guard columns that must be bit-identical afterwards.  One-hot rows of A make
C an exact copy of (sums of) rows of B."""
import ctypes as C

import pytest
import torch

pytestmark = pytest.mark.gpu

from lafs_cvpr2024_amd import _lib, ops  # noqa: E402

import fp64_bounds as fb  # noqa: E402
import gemm_cases as gc  # noqa: E402
from fp64_bounds import U, bf16, f16, f32, f64  # noqa: E402

DEV = "cuda"
N_XCD = 8


class Vec:
    """A float vector [n] with 8 NaN guard elements behind it."""

    def __init__(self, init):
        self.buf = torch.full((init.numel() + 8,), float("nan"), device=DEV, dtype=f32)
        self.v = self.buf[:init.numel()]
        self.v.copy_(init)

    def intact(self, name):
        assert bool(torch.isnan(self.buf[self.v.numel():]).all()), f"{name}: written past its end"


def fused(mats, dtype):
    """Column slices of ONE NaN-filled buffer (the layout of a fused qkv activation), 8 NaN columns between neighbours."""
    M = mats[0].shape[0]
    buf = torch.full((M + gc.GR, sum(m.shape[1] + 8 for m in mats) + 8), float("nan"), device=DEV, dtype=dtype)
    views, c0 = [], 8
    for m in mats:
        buf[:M, c0:c0 + m.shape[1]] = m.to(device=DEV, dtype=dtype)
        views.append(buf[:M, c0:c0 + m.shape[1]])
        c0 += m.shape[1] + 8
    return views


def run(c):
    worst = c["dist"] == "positive"
    h16 = f16 if c["half"] else bf16
    data = gc.tn_inputs(c)
    items = gc.tn_items(c)
    As, Bs = fused([d[0] for d in data], h16), fused([d[1] for d in data], h16)
    fn = c["fn"]

    def launch():
        """One run on fresh outputs: returns [(C Out, colsum Vec or None)], workspace guard."""
        outs, ws = [], None
        for (a, b, co, so), (n1, n2, acc, cs) in zip(data, items):
            o = gc.Out(n1, n2, f32, DEV, off=4)
            if acc or fn in ("tn_acc", "tn_part"):
                o.v.copy_(co)                            # (accumulate = 0 leaves C NaN-filled: it must not be read)
            outs.append((o.arm(), Vec(so.to(DEV)) if cs else None))
        if fn == "tn_acc":
            (o, v), = outs
            ops.gemm_tn_acc(As[0], Bs[0], o.v, splits=c["splits"], colsum=None if v is None else v.v)
        elif fn in ("wgrad", "wgrad_f16"):
            (o, v), = outs
            nbytes = int(_lib.lib().lafs_wgrad_workspace_bytes(c["M"], c["N1"], c["N2"]))
            ws = torch.full((nbytes // 4 + 64,), float("nan"), device=DEV, dtype=f32)
            ops.wgrad(As[0], Bs[0], o.v, accumulate=items[0][2], colsum=None if v is None else v.v, workspace=ws[:max(nbytes // 4, 4)])
            ws = ws[max(nbytes // 4, 4):]
        else:
            probs = [(A, B, o.v, it[2], None if v is None else v.v) for A, B, (o, v), it in zip(As, Bs, outs, items)]
            st, M = ops._wgrad_items(probs)
            nbytes = int(_lib.lib().lafs_wgrad_group_workspace_bytes(st, len(probs), M, c["wg"]))
            assert nbytes >= 0
            ws = torch.full((nbytes // 4 + 64,), float("nan"), device=DEV, dtype=f32)
            ops.wgrad_group(probs, workspace=ws[:max(nbytes // 4, 4)], max_workgroups=c["wg"])
            ws = ws[max(nbytes // 4, 4):]
        torch.cuda.synchronize()
        return outs, ws

    outs, ws = launch()
    if ws is not None:
        assert bool(torch.isnan(ws).all()), f"{c['id']}: written behind the workspace lafs_wgrad*_workspace_bytes asks for"
    for i, ((a, b, co, so), (n1, n2, acc, cs), (o, v)) in enumerate(zip(data, items, outs)):
        a, b, co, so = a.to(DEV), b.to(DEV), co.to(DEV), so.to(DEV)
        name = f"{c['id']}[{i}]"
        o.intact(name)
        ref, bound = fb.gemm_tn(a, b, co if (acc or fn == "tn_acc") else None, worst)
        fb.check(f"{name}: C", o.v, ref, bound)
        if v is not None:
            v.intact(name)
            fb.check(f"{name}: colsum_a", v.v, *fb.colsum(a, so, worst))
    if fn != "tn_acc":                                   # the header promises determinism for C and colsum_a (no atomics)
        again, _ = launch()
        for (o, v), (o2, v2) in zip(outs, again):
            assert torch.equal(o.v.view(torch.int32), o2.v.view(torch.int32)), f"{c['id']}: C differs between two runs"
            assert v is None or torch.equal(v.v.view(torch.int32), v2.v.view(torch.int32)), f"{c['id']}: colsum_a differs between two runs"


def run_part(c):
    """lafs_gemm_tn_part into zeroed per-XCD images with part_stride > N1 ldc, then lafs_reduce_partials."""
    worst = c["dist"] == "positive"
    (a, b, co, so), = gc.tn_inputs(c)
    n1, n2, ld = c["N1"], c["N2"], c["N2"] + 8
    A, B = fused([a], bf16)[0], fused([b], bf16)[0]
    part = torch.zeros(N_XCD, n1 + gc.GR, ld, device=DEV, dtype=f32)
    part[:, n1:] = float("nan")
    v = Vec(so.to(DEV)) if c["colsum"] else None
    ops.gemm_tn_part(A, B, part[:, :n1, :n2], splits=c["splits"], colsum=None if v is None else v.v)
    torch.cuda.synchronize()
    a, b, co, so = a.to(DEV), b.to(DEV), co.to(DEV), so.to(DEV)
    assert bool(torch.isnan(part[:, n1:]).all()) and bool((part[:, :n1, n2:].view(torch.int32) == 0).all()), f"{c['id']}: images written outside N1 x N2"
    ref, bound = fb.gemm_tn(a, b, None, worst)
    fb.check(f"{c['id']}: sum of the XCD images", part[:, :n1, :n2].double().sum(0), ref, bound)
    if v is not None:
        v.intact(c["id"])
        fb.check(f"{c['id']}: colsum_a", v.v, *fb.colsum(a, so, worst))
    images = part[:, :n1, :n2].double().clone()
    out = torch.zeros(n1 + 1, ld, device=DEV, dtype=f32)
    out[n1] = float("nan")
    out[:n1, :n2] = co
    ops.reduce_partials(part[:, :n1], out[:n1])
    torch.cuda.synchronize()
    assert bool(torch.isnan(out[n1]).all()) and bool((out[:n1, n2:].view(torch.int32) == 0).all())
    # out += the images, added one by one in fp32
    tot = co + images.sum(0)
    fb.check(f"{c['id']}: out += images", out[:n1, :n2], tot, N_XCD * U * (co.abs() + images.abs().sum(0)))
    assert bool((part[:, :n1].view(torch.int32) == 0).all()), f"{c['id']}: the images are not exactly zero after lafs_reduce_partials"


@pytest.mark.parametrize("c", gc.TN_CASES, ids=[c["id"] for c in gc.TN_CASES])
def test_token_axis_reduction(c):
    (run_part if c["fn"] == "tn_part" else run)(c)


@pytest.mark.parametrize("M,N", [(1, 4), (257, 4), (300, 68), (33, 200), (4099, 8)])
def test_colsum_bf16_acc(M, N):
    gen = torch.Generator()
    gen.manual_seed(gc.seed_of("colsum", M, N))
    x = fb.rbf(torch.randn(M, N, generator=gen, dtype=f64))
    old = torch.randn(N, generator=gen, dtype=f64).to(f32)
    v = Vec(old.to(DEV))
    ops.colsum_bf16_acc(gc.inp(x, bf16, DEV), v.v)
    torch.cuda.synchronize()
    v.intact("colsum")
    fb.check(f"colsum_bf16_acc M={M} N={N}", v.v, *fb.colsum(x.to(DEV), old.double().to(DEV)))


@pytest.mark.parametrize("n,n_part", [(4, 1), (4, 5), (1028, 3), (2048, 8)])
def test_sum_slices(n, n_part):
    gen = torch.Generator()
    gen.manual_seed(gc.seed_of("slices", n, n_part))
    stride = n + 12
    part = torch.full((n_part, stride), float("nan"), device=DEV, dtype=f32)
    part[:, :n] = torch.randn(n_part, n, generator=gen).to(DEV)
    v = Vec(torch.full((n,), float("nan")))               # plain store: the old contents must not matter
    _lib.call("lafs_sum_slices", C.c_void_p(part.data_ptr()), stride, n_part, n, C.c_void_p(v.v.data_ptr()))
    torch.cuda.synchronize()
    v.intact("sum_slices")
    p = part[:, :n].double()
    fb.check(f"sum_slices n={n} x{n_part}", v.v, p.sum(0), n_part * U * p.abs().sum(0))
    for bad in (dict(n=6), dict(stride=stride + 2)):
        with pytest.raises(_lib.LafsHipError, match="multiples of 4"):
            _lib.call("lafs_sum_slices", C.c_void_p(part.data_ptr()), bad.get("stride", stride), n_part, bad.get("n", n), C.c_void_p(v.v.data_ptr()))
