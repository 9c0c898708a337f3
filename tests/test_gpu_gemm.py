"""lafs_gemm_nt (csrc/gemm.hip, gemm_kres.hip, gemm_big.hip) against the fp64 oracle of tests/fp64_bounds.py, element by element: every
route and instantiation, every epilogue form, N % 8 != 0, ragged rows, short and long and split reductions, dropout, and the
argument checks.  The grid (gemm_cases.NT_CASES) names the intended kernel instantiation in each case id; the route is asserted
through lafs_gemm_nt_route wherever that entry point tells routes apart.

Every operand and output is a column slice of a wider buffer (every row stride exceeds the logical width); inputs sit in NaN, outputs
in NaN-filled buffers with guard rows past M and guard columns on both sides of N: the owned region must be overwritten completely,
everything else must be bit-identical afterwards.  tests/test_oracle_gemm_host.py shows on the CPU that these bounds reject seeded
faults."""
import ctypes as C

import pytest
import torch

pytestmark = pytest.mark.gpu

from lafs_cvpr2024_amd import _lib, ops  # noqa: E402

import fp64_bounds as fb  # noqa: E402
import gemm_cases as gc  # noqa: E402
from fp64_bounds import bf16, f16, f32, f64  # noqa: E402

DEV = "cuda"
SENTINEL = 768.0                         # (exact in bf16)
_CTX = {}
BY_ID = {c["id"]: c for c in gc.NT_CASES}
SEEDS = {c["seed"] for c in gc.NT_CASES if c["seed"]}
_BASE = {}                               # outputs of the cases that have an A/B partner, for the partner's comparison


def ctx_for(opts):
    """A context with the given LAFS_OPT_* values (the A/B partners of the routes); None: the process's default context."""
    if not opts:
        return None
    key = tuple(sorted(opts.items()))
    if key not in _CTX:
        _CTX[key] = _lib.Ctx(options=dict(opts))
    return _CTX[key]


def drop_factors(c, M, N):
    """The factor matrix the kernels apply, from lafs_debug_dropout_mask: rows [drop_row0, drop_row0 + M) of a larger mask, the seed
    advanced by 7919 * step when the launch reads a device step counter.  Returns (factors fp64 [M, N], seed, step tensor or None)."""
    if not c["drop_p"] > 0:
        return None, 0, None
    seed = gc.seed_of("drop", c["id"]) & 0xFFFFFF
    step = None if c["drop_step"] is None else torch.tensor([float(c["drop_step"])], device=DEV, dtype=f32)
    eff = seed + 7919 * (c["drop_step"] or 0)
    full = ops.dropout_mask(c["drop_row0"] + M + 37, N, c["drop_p"], eff)
    return full[c["drop_row0"]:c["drop_row0"] + M].double(), seed, step


def run(c):
    """One request against the oracle; returns {name: (kernel output, bound)}."""
    epi, M, N, K = c["epi"], c["M"], c["N"], c["K"]
    h16 = f16 if c["half"] else bf16
    d = gc.nt_inputs(c)
    dd = {k: v.to(DEV) for k, v in d.items()}
    ctx = ctx_for(c["opts"])
    A, B = gc.inp(d["A"], h16, DEV), gc.inp(d["B"], h16, DEV)
    kw = dict(ctx=ctx, splits=c["splits"], act=c["act"])
    if c["bias"]:
        kw["bias"] = dd["bias"].to(f32)
    drop, seed, step = drop_factors(c, M, N)
    if drop is not None:
        kw.update(drop_p=c["drop_p"], drop_seed=seed, drop_step=step, drop_row0=c["drop_row0"])
    if "aux" in d:
        kw["aux"] = gc.inp(d["aux"], h16, DEV, pad=16)
    if c["form"] == "save":
        kw["act"] = 1                                    # LAFS_GELU_SAVE_GRAD
    slices = gc.nt_slices(K, c["splits"])
    n_img = len(slices) if epi == fb.EPI_F32 and c["splits"] > 1 else 1
    out_rows = M + M // c["npatch"] if epi == fb.EPI_EMBED_F32 else M
    out = gc.Out(out_rows * n_img, N, f32 if epi in fb.F32_EPIS else h16, DEV)
    outs = {"C": out}
    if epi == fb.EPI_RESID_F32:
        kw.update(row2seq=dd["row2seq"], seq_scale=None if "seq_scale" not in d else dd["seq_scale"].to(f32))
        if kw["seq_scale"] is None:
            kw.pop("row2seq")
        if c["alias"]:
            out.v.copy_(dd["resid"])
            kw["resid"] = out.v
        else:
            kw["resid"] = gc.inp(d["resid"], f32, DEV, off=4, pad=4)
    if epi == fb.EPI_ATOMIC_F32:
        out.v.zero_()
    if epi == fb.EPI_EMBED_F32:
        kw.update(pos=dd["pos"].to(f32).contiguous(), npatch=c["npatch"], out_rows=out_rows)
        cls = torch.arange(0, out_rows, c["npatch"] + 1, device=DEV)
        out.v[cls] = SENTINEL                            # the cls rows belong to lafs_embed_cls: not this kernel's to write
        out.owned[0, cls] = False
    if epi == fb.EPI_BF16_GELU:
        outs["C2"] = gc.Out(M, N, bf16, DEV, off=16)
        kw["out2"] = outs["C2"].v
        if c["form"] == "noC":
            kw["skip_pre"] = True
            out.owned[:] = False
    for o in outs.values():
        o.arm()
    if c["route"] is not None:
        got = ops.gemm_nt(A, B, epi, out=out.v, route_only=True, **kw)
        assert got == c["route"], f"{c['id']}: lafs_gemm_nt_route says {got}, the case is meant for route {c['route']}"
    if n_img > 1:
        assert int(_lib.lib().lafs_gemm_nt_slices(K, c["splits"])) == n_img
    ops.gemm_nt(A, B, epi, out=out.v, **kw)
    torch.cuda.synchronize()
    for name, o in outs.items():
        o.intact(f"{c['id']}: {name}")

    exp = gc.nt_expected(c, dd, drop)
    res = {}
    ld = out.buf.shape[2]
    for name, (ref, bound, is16) in exp.items():
        if name == "sum":
            total = torch.full((M, ld), SENTINEL, device=DEV, dtype=f32)
            _lib.call("lafs_sum_slices", C.c_void_p(out.buf.data_ptr()), M * ld, n_img, M * ld, C.c_void_p(total.data_ptr()))
            torch.cuda.synchronize()
            got = total[:, 8:8 + N]
        elif name.startswith("C["):
            got = out.buf[0, :M * n_img].view(n_img, M, ld)[int(name[2:-1]), :, 8:8 + N]
        elif name == "C" and c["form"] == "noC":
            continue
        elif epi == fb.EPI_EMBED_F32:
            m = torch.arange(M, device=DEV)
            got = out.v[m + m // c["npatch"] + 1]
        else:
            got = outs[name].v
        fb.check(f"{c['id']}: {name}", got, ref, bound, is16)
        res[name] = (got.double(), bound)
    return res


@pytest.mark.parametrize("c", gc.NT_CASES, ids=[c["id"] for c in gc.NT_CASES])
def test_gemm_nt(c):
    res = run(c)
    if c["id"] in SEEDS:
        _BASE[c["id"]] = res                             # (a base runs once: its partner finds the result here)
    if c["seed"] is None:
        return
    # an A/B partner: the same operands as case `seed` on another kernel.  Both were just held to the same fp64 reference; held to
    # each other they may differ by the sum of their bounds (bound 0: bit for bit)
    if c["seed"] not in _BASE:                           # (only when the partner was selected without its base)
        _BASE[c["seed"]] = run(BY_ID[c["seed"]])
    for name, (got, bound) in res.items():
        other, obound = _BASE[c["seed"]][name]
        bad = (got - other).abs() > bound + obound
        assert not bool(bad.any()), f"{c['id']}: {name} differs from {c['seed']} by more than the two bounds at {bad.nonzero()[0].tolist()}"


# ------------------------------------------------------------------------------------------------ refusals (nothing is launched)
def test_misaligned_operands_and_a_biased_k_split_are_refused():
    """The alignment contract of include/lafs_hip.h: what the 16-byte loads and stores cannot take returns a negative code.  Only the
    refusal is tested -- a misaligned request never reaches a kernel, and the outputs keep their guard values."""
    M, N, K = 64, 64, 64
    wide = lambda dt: torch.full((M, 128), SENTINEL, device=DEV, dtype=dt)
    A, B, Cb, C2, Cf, R, X = wide(bf16), wide(bf16), wide(bf16), wide(bf16), wide(f32), wide(f32), wide(bf16)
    a, b = A[:, :K], B[:N, :K]
    bias = torch.zeros(N, device=DEV)
    cases = [
        ("A and B must be 16-byte aligned", lambda: ops.gemm_nt(A[:, 4:4 + K], b, fb.EPI_BF16, out=Cb[:, :N])),
        ("A and B must be 16-byte aligned", lambda: ops.gemm_nt(a, B[:N, 2:2 + K], fb.EPI_BF16, out=Cb[:, :N])),
        ("C must be 16-byte aligned", lambda: ops.gemm_nt(a, b, fb.EPI_BF16, out=Cb[:, 4:4 + N])),
        ("C must be 16-byte aligned", lambda: ops.gemm_nt(a, b, fb.EPI_F32, out=Cf[:, 2:2 + N])),
        ("C2 must be 16-byte aligned", lambda: ops.gemm_nt(a, b, fb.EPI_BF16_GELU, out=Cb[:, :N], out2=C2[:, 4:4 + N])),
        ("resid must be 16-byte aligned", lambda: ops.gemm_nt(a, b, fb.EPI_RESID_F32, out=Cf[:, :N], resid=R[:, 2:2 + N])),
        ("residual epilogue needs resid", lambda: ops.gemm_nt(a, b, fb.EPI_RESID_F32, out=Cf[:, :N], resid=R.view(-1)[:M * 126].view(M, 126)[:, :N])),
        ("aux must be 16-byte aligned", lambda: ops.gemm_nt(a, b, fb.EPI_DGELU_BF16, out=Cb[:, :N], aux=X[:, 4:4 + N])),
        ("ldaux a multiple of 8", lambda: ops.gemm_nt(a, b, fb.EPI_DGELU_BF16, out=Cb[:, :N], aux=X.view(-1)[:M * 124].view(M, 124)[:, :N])),
        ("ldc must be a multiple of 8", lambda: ops.gemm_nt(a, b, fb.EPI_BF16, out=Cb.view(-1)[:M * 124].view(M, 124)[:, :N])),
        ("lda/ldb must be multiples of 8", lambda: ops.gemm_nt(A.view(-1)[:M * 124].view(M, 124)[:, :K], b, fb.EPI_BF16, out=Cb[:, :N])),
        ("takes no bias", lambda: ops.gemm_nt(a, b, fb.EPI_F32, out=Cf[:, :N], splits=2, bias=bias)),
        # the float4 folds: base pointers
        ("part and out must be 16-byte aligned", lambda: _lib.call("lafs_sum_slices", C.c_void_p(R.data_ptr() + 4), 128, 2, 64, C.c_void_p(Cf.data_ptr()))),
        ("part and out must be 16-byte aligned", lambda: _lib.call("lafs_sum_slices", C.c_void_p(R.data_ptr()), 128, 2, 64, C.c_void_p(Cf.data_ptr() + 8))),
        ("part and out must be 16-byte aligned", lambda: _lib.call("lafs_reduce_partials", C.c_void_p(R.data_ptr() + 8), 128, 2, 64, C.c_void_p(Cf.data_ptr()))),
        ("part and out must be 16-byte aligned", lambda: _lib.call("lafs_reduce_partials", C.c_void_p(R.data_ptr()), 128, 2, 64, C.c_void_p(Cf.data_ptr() + 4))),
    ]
    # lafs_gemm_nt_route gives no route for what lafs_gemm_nt refuses
    assert ops.gemm_nt(A[:, 4:4 + K], b, fb.EPI_BF16, out=Cb[:, :N], route_only=True) < 0
    assert ops.gemm_nt(a, b, fb.EPI_DGELU_BF16, out=Cb[:, :N], aux=X.view(-1)[:M * 124].view(M, 124)[:, :N], route_only=True) < 0
    assert ops.gemm_nt(a, b, fb.EPI_BF16, out=Cb[:, :N], route_only=True) == 0
    torch.cuda.synchronize()
    for why, fn in cases:
        with pytest.raises(_lib.LafsHipError, match=why):
            fn()
    torch.cuda.synchronize()
    for t in (Cb, C2, Cf, R):
        assert bool((t == SENTINEL).all()), "an output was written by a rejected call"
    # the same requests, aligned, run
    A.zero_(); B.zero_(); R.zero_(); X.zero_()
    ops.gemm_nt(a, b, fb.EPI_RESID_F32, out=Cf[:, :N], resid=R[:, 4:4 + N])
    ops.gemm_nt(a, b, fb.EPI_DGELU_BF16, out=Cb[:, 8:8 + N], aux=X[:, 8:8 + N])
    torch.cuda.synchronize()
    assert bool((Cf[:, :N] == 0).all()) and bool((Cb[:, 8:8 + N] == 0).all()) and bool((Cb[:, :8] == SENTINEL).all())
