"""lafs_attention_cls_fwd / lafs_attention_cls_bwd (csrc/attention.hip: the cls query alone, for the last block of a trunk that is read
through x[:, 0]) against a plain fp64 restatement on the same bf16 operands, element by element, and against the dense kernels.

The reference rounds to bf16 exactly where the kernels store 16 bits -- o_c in the forward, every dqkv value in the backward -- and
makes the register roundings the kernels make where they make them (the un-normalised P in front of P V in the forward; P and dS in the
backward -- the places where lafs_attention_fwd / _bwd round), each through `flip`: the reference holds the rounded value and a bound
that is 0 unless the kernel's fp32 value can reach another bf16 value.  (For the comparison with the dense kernels, whose reference
keeps the unrounded value and bounds these roundings by half an ulp each, `exact=False` does the same, so that both references owe the
same values.)  Bounds as in tests/fp64_bounds.py: `flip` at every bf16 rounding, `acc_factor` for the fp32 sums (64-term dot products, sums over the L keys; the kernels' summation trees are at most 8 + 3 resp. L / 8 + 3 additions deep,
inside acc_factor's 4 sqrt(K) for every K used here).  No bound is looser than the caps of the dense attention test (1.5e-2 of the
maximum forward, 3e-2 backward).

Every call covers the three MIDDLE sequences of a five-sequence buffer (cu_seqlens pointer advanced by one): rows of the first and the
last sequence, guard rows and guard columns must keep their bits; dQ rows other than the cls rows must be exact zeros; two calls give the
same bits.  The cross-check feeds lafs_attention_fwd / _bwd the same operands with a dO that is zero outside the cls rows (and the cls
backward the dense forward's out / lse of the cls rows, so both kernels owe the same fp64 values): the results agree within the sum of
the two references' bounds."""
import math

import pytest
import torch

pytestmark = pytest.mark.gpu

import fp64_bounds as FB  # noqa: E402
import test_gpu_attention as A  # noqa: E402
from lafs_cvpr2024_amd import _lib  # noqa: E402
from lafs_cvpr2024_amd.ops import _p  # noqa: E402

DEV = "cuda"
bf16, f32, f64 = torch.bfloat16, torch.float32, torch.float64
U = FB.U
SCALE = 64 ** -0.5
# three sequences per call, mixed lengths: every length of {1, 15, 16, 17, 37, 100, 197, 256} in some call and in several positions
CALLS = {"short": [1, 15, 16], "tiles": [17, 37, 100], "long": [197, 256, 1], "mixed": [256, 16, 37], "crops": [37, 197, 17], "edge": [15, 1, 100]}
OUTER = (5, 21)         # the sequences in front of and behind the call's three


def launch_cls_fwd(qkv, cud, n_seq, max_len, heads, scale, o_c, lse_c):
    _lib.call("lafs_attention_cls_fwd", _p(qkv), qkv.stride(0), _p(cud), n_seq, max_len, heads, scale, _p(o_c), o_c.stride(0), _p(lse_c))


def launch_cls_bwd(qkv, o_c, do_c, lse_c, cud, n_seq, max_len, heads, scale, dqkv):
    _lib.call("lafs_attention_cls_bwd", _p(qkv), qkv.stride(0), _p(o_c), o_c.stride(0), _p(do_c), do_c.stride(0), _p(lse_c), _p(cud), n_seq,
              max_len, heads, scale, _p(dqkv), dqkv.stride(0))


# ------------------------------------------------------------------------------------------------ fp64 reference with bounds
def cls_scores(q0, k, scale):
    """x = fl(scale) q0 . k_j (natural-log domain) and the bound on the kernel's fp32 value: 64 exact products summed in fp32, one product."""
    sc = A.f32c(scale)
    S, Sa = (k * q0).sum(-1), (k.abs() * q0.abs()).sum(-1)
    x = S * sc
    return x, FB.acc_factor(64) * U * sc * Sa + 2 * U * x.abs()


def cls_fwd_ref(q0, k, v, scale, exact=True):
    """q0 [H, 64], k, v [H, L, 64] (fp64 of the bf16 operands) -> o_c = bf16(softmax(scale q0 k^T) v) [H, 64], lse [H], with bounds.
    exact: P rounded to bf16 in the reference as in the kernel (else: unrounded, half an ulp of every p_j added to the bound)."""
    L = k.shape[-2]
    x, ex = cls_scores(q0.unsqueeze(-2), k, scale)                       # [H, L]
    m = x.max(-1, keepdim=True).values
    a = x - m
    e = torch.exp(a)
    # exp of an argument off by ex (the kernel's own maximum is a factor common to the row: it cancels), the subtraction and the
    # product with log2(e) inside __expf round (2 u |a|, 2x margin), v_exp_f32 is good to 1 ulp (2x margin)
    re = torch.expm1(ex + 4 * U * a.abs()) + 4 * U
    s = e.sum(-1, keepdim=True)
    rs = (e * re).sum(-1, keepdim=True) / s + FB.acc_factor(L) * U       # fp32 sum of L positive terms
    # each e_j off by re_j, then rounded to bf16 in registers, then accumulated in fp32; the normaliser sums the unrounded e
    eb, ebe = FB.flip(e, e * re) if exact else (e, e * re + A.R * A.top(e * (1 + re)))
    num, numa = (eb.unsqueeze(-1) * v).sum(-2), (eb.unsqueeze(-1) * v.abs()).sum(-2)
    enum = (ebe.unsqueeze(-1) * v.abs()).sum(-2) + FB.acc_factor(L) * U * numa
    o = num / s
    oe = (enum + num.abs() * (rs + 6 * U)) / s * (1 + 2 * rs)            # 1 / sum (a few ulp), the product
    ob, obe = FB.flip(o, oe)
    lse = (m + torch.log(s)).squeeze(-1)
    # log-sum-exp is 1-Lipschitz in the maximum norm of its arguments; the sum's relative error; __logf (log2, product with ln 2); the add
    lsee = (ex.max(-1).values + 4 * U * a.abs().max(-1).values + 1.01 * rs.squeeze(-1) + 16 * U + 4 * U * lse.abs())
    return ob, obe, lse, lsee


def cls_bwd_ref(q0, k, v, o, lse, do, scale, exact=True):
    """dq0 [H, 64], dk, dv [H, L, 64] (bf16) from the bf16 operands, the stored bf16 o [H, 64], fp32 lse [H] and dO [H, 64], with bounds.
    exact: P and dS rounded to bf16 in the reference as in the kernel (else: unrounded, half an ulp of each added to the bounds)."""
    L = k.shape[-2]
    sc = A.f32c(scale)
    x, ex = cls_scores(q0.unsqueeze(-2), k, scale)
    arg = x - lse.unsqueeze(-1)
    p = torch.exp(arg)
    ep = p * (torch.expm1(ex + 4 * U * arg.abs()) + 4 * U)
    # ... then rounded to bf16 in registers for dV; dS is formed from the unrounded P
    pr, ep_r = FB.flip(p, ep) if exact else (p, ep + A.R * A.top(p + ep))
    delta = (o * do).sum(-1, keepdim=True)                                # [H, 1]
    ed = FB.acc_factor(64) * U * (o * do).abs().sum(-1, keepdim=True)
    dp = (v * do.unsqueeze(-2)).sum(-1)                                   # [H, L]
    t = dp - delta
    et = FB.acc_factor(64) * U * (v.abs() * do.abs().unsqueeze(-2)).sum(-1) + ed + U * t.abs()
    ds = p * t * sc
    eds = sc * (ep * t.abs() + (p + ep) * et) + 3 * U * ds.abs()
    ds, eds = FB.flip(ds, eds) if exact else (ds, eds + A.R * A.top(ds.abs() + eds))       # dS rounded to bf16 in registers
    dv = pr.unsqueeze(-1) * do.unsqueeze(-2)
    dve = ep_r.unsqueeze(-1) * do.abs().unsqueeze(-2) + U * dv.abs()
    dk = ds.unsqueeze(-1) * q0.unsqueeze(-2)
    dke = eds.unsqueeze(-1) * q0.abs().unsqueeze(-2) + U * dk.abs()
    dq = (ds.unsqueeze(-1) * k).sum(-2)
    dqe = (eds.unsqueeze(-1) * k.abs()).sum(-2) + FB.acc_factor(L) * U * (ds.abs().unsqueeze(-1) * k.abs()).sum(-2)
    return FB.flip(dq, dqe) + FB.flip(dk, dke) + FB.flip(dv, dve)


# ------------------------------------------------------------------------------------------------ one call, run once per (lens, heads)
_CACHE = {}


def run(case, heads):
    """Forward, backward, a second pair of calls and the dense kernels on one set of operands; everything the tests look at, on the CPU."""
    key = (case, heads)
    if key in _CACHE:
        return _CACHE[key]
    lens = [OUTER[0]] + CALLS[case] + [OUTER[1]]
    T, inner = sum(lens), heads * 64
    cu = [0]
    for n in lens:
        cu.append(cu[-1] + n)
    qkv_c, do_all = A.make_inputs(lens, heads, SCALE, "normal", A._seed("cls", case, heads))
    cud = torch.tensor(cu, dtype=torch.int32, device=DEV)
    mid, max_len = cud[1:], max(CALLS[case])
    cls_rows = torch.tensor(cu[1:4])
    qkv, do_c = A.Buf(T, 3 * inner, bf16, 8, qkv_c), A.Buf(3, inner, bf16, 24, do_all[cls_rows])
    o_c, lse_c, dqkv = A.Buf(3, inner, bf16, 16), A.Buf(3, heads, f32, 0), A.Buf(T, 3 * inner, bf16, 40)
    launch_cls_fwd(qkv.v, mid, 3, max_len, heads, SCALE, o_c.v, lse_c.v)
    launch_cls_bwd(qkv.v, o_c.v, do_c.v, lse_c.v, mid, 3, max_len, heads, SCALE, dqkv.v)
    torch.cuda.synchronize()
    # a second pair of calls into fresh buffers
    o2, l2, d2 = A.Buf(3, inner, bf16, 16), A.Buf(3, heads, f32, 0), A.Buf(T, 3 * inner, bf16, 40)
    launch_cls_fwd(qkv.v, mid, 3, max_len, heads, SCALE, o2.v, l2.v)
    launch_cls_bwd(qkv.v, o2.v, do_c.v, l2.v, mid, 3, max_len, heads, SCALE, d2.v)
    # the dense kernels on the same three sequences, dO zero outside the cls rows; then the cls backward on THEIR out / lse of the cls rows
    do_dense = torch.zeros(T, inner, dtype=bf16)
    do_dense[cls_rows] = do_all[cls_rows]
    dod = A.Buf(T, inner, bf16, 24, do_dense)
    out_d, lse_d, dqkv_d = A.Buf(T, inner, bf16, 16), A.Buf(T, heads, f32, 0), A.Buf(T, 3 * inner, bf16, 40)
    A.launch_fwd(qkv.v, mid, 3, max_len, heads, SCALE, out_d.v, lse_d.v)
    A.launch_bwd(qkv.v, out_d.v, dod.v, lse_d.v, mid, 3, max_len, heads, SCALE, dqkv_d.v)
    rows_dev = cls_rows.to(DEV)
    o3, l3, d3 = A.Buf(3, inner, bf16, 16, out_d.v[rows_dev]), A.Buf(3, heads, f32, 0, lse_d.v[rows_dev]), A.Buf(T, 3 * inner, bf16, 40)
    launch_cls_bwd(qkv.v, o3.v, do_c.v, l3.v, mid, 3, max_len, heads, SCALE, d3.v)
    torch.cuda.synchronize()
    r = dict(lens=lens, cu=cu, heads=heads, qkv_c=qkv_c, do=do_all[cls_rows], bufs=dict(qkv=qkv, do_c=do_c, o_c=o_c, lse_c=lse_c, dqkv=dqkv),
             second=(o2, l2, d2), o_c=o_c.v.cpu(), lse_c=lse_c.v.cpu(), dqkv=dqkv.v.cpu(), out_d=out_d.v.cpu(), lse_d=lse_d.v.cpu(),
             dqkv_d=dqkv_d.v.cpu(), dqkv_3=d3.v.cpu())
    _CACHE[key] = r
    return r


def operands(r, i):
    """fp64 q0 [H, 64], k, v [H, L, 64] and dO [H, 64] of the call's sequence i (0..2)."""
    H, inner = r["heads"], r["heads"] * 64
    a, b = r["cu"][1 + i], r["cu"][2 + i]
    blk = r["qkv_c"][a:b].double()
    part = lambda j: blk[:, j * inner:(j + 1) * inner].view(b - a, H, 64).transpose(0, 1)
    return part(0)[:, 0], part(1), part(2), r["do"][i].double().view(H, 64)


def grads(r, t, i):
    """dq [L, H, 64] -> [H, L, 64], dk, dv of the call's sequence i from a dqkv image t."""
    H, inner = r["heads"], r["heads"] * 64
    a, b = r["cu"][1 + i], r["cu"][2 + i]
    return [t[a:b, j * inner:(j + 1) * inner].double().view(b - a, H, 64).transpose(0, 1) for j in range(3)]


GRID = [(c, h) for c in CALLS for h in (2, 6)]
IDS = [f"{c}-h{h}" for c, h in GRID]


@pytest.mark.parametrize("case,heads", GRID, ids=IDS)
def test_forward_against_fp64(case, heads):
    r = run(case, heads)
    st_o, st_l = [0.0, 0, 0, 0], [0.0, 0, 0, 0]
    for i, L in enumerate(CALLS[case]):
        q0, k, v, _ = operands(r, i)
        ob, obe, lse, lsee = cls_fwd_ref(q0, k, v, SCALE)
        if L >= 16:
            assert float(obe.max()) <= 1.5e-2 * float(ob.abs().max()), "forward bound looser than 1.5e-2 of the maximum"
        A.check(f"[cls fwd {case} h{heads}] o_c, length {L}", r["o_c"][i].view(heads, 64), ob, obe, st_o)
        A.check(f"[cls fwd {case} h{heads}] lse_c, length {L}", r["lse_c"][i].view(heads, 1), lse.unsqueeze(-1), lsee.unsqueeze(-1), st_l)
    print(f"[cls fwd {case} h{heads}] |error| / bound  o_c {st_o[0]:.3f}  lse_c {st_l[0]:.3f};  bound 0 (must be exact) {100.0 * st_o[1] / st_o[2]:.1f} %")
    for name in ("o_c", "lse_c"):
        r["bufs"][name].untouched(f"cls fwd {case}: {name}")


@pytest.mark.parametrize("case,heads", GRID, ids=IDS)
def test_backward_against_fp64(case, heads):
    r = run(case, heads)
    st = [0.0, 0, 0, 0]
    for i, L in enumerate(CALLS[case]):
        q0, k, v, do = operands(r, i)
        o = r["o_c"][i].double().view(heads, 64)
        dq, dqe, dk, dke, dv, dve = cls_bwd_ref(q0, k, v, o, r["lse_c"][i].double(), do, SCALE)
        if L >= 16:
            for name, ref, e in (("dq", dq, dqe), ("dk", dk, dke), ("dv", dv, dve)):
                assert float(e.max()) <= 3e-2 * float(ref.abs().max()), f"{name} bound looser than 3e-2 of the maximum"
        gq, gk, gv = grads(r, r["dqkv"], i)
        nm = f"[cls bwd {case} h{heads}] length {L}"
        A.check(f"{nm}: dq of the cls row", gq[:, 0], dq, dqe, st)
        A.check(f"{nm}: dk", gk, dk, dke, st)
        A.check(f"{nm}: dv", gv, dv, dve, st)
        raw = r["dqkv"][r["cu"][1 + i] + 1:r["cu"][2 + i], :heads * 64]
        assert int(raw.view(torch.int16).count_nonzero()) == 0, f"{nm}: dQ rows other than the cls row are not exact zeros"
    print(f"[cls bwd {case} h{heads}] |error| / bound {st[0]:.3f};  bound 0 (must be exact) {100.0 * st[1] / st[2]:.1f} %")


@pytest.mark.parametrize("case,heads", GRID, ids=IDS)
def test_rows_outside_the_call_and_inputs_keep_their_bits_and_two_calls_agree(case, heads):
    r = run(case, heads)
    b = r["bufs"]
    dq = b["dqkv"]
    dq.untouched(f"cls bwd {case}: dqkv")
    lo, hi = r["cu"][1], r["cu"][4]
    bits, before = dq.bits(dq.buf), dq.bits(dq.before)
    assert torch.equal(bits[:lo], before[:lo]) and torch.equal(bits[hi:], before[hi:]), "rows of sequences outside the call were written"
    assert not bool(torch.isnan(dq.v[lo:hi].float()).any()), "a value of the call's own dqkv range was not written"
    for name in ("qkv", "do_c"):
        b[name].untouched(f"cls {case}: {name}", whole=True)
    for name, x, y in zip(("o_c", "lse_c", "dqkv"), (b["o_c"], b["lse_c"], b["dqkv"]), r["second"]):
        assert torch.equal(x.bits(x.buf), y.bits(y.buf)), f"{name} differs between two calls on the same inputs"


@pytest.mark.parametrize("case,heads", GRID, ids=IDS)
def test_against_the_dense_kernels(case, heads):
    """lafs_attention_fwd's cls rows against o_c / lse_c, and lafs_attention_bwd under a dO that is zero outside the cls rows against
    the cls backward on the same out / lse: within the sum of the two references' bounds (both kernels owe the same fp64 values)."""
    r = run(case, heads)
    worst = 0.0
    for i, L in enumerate(CALLS[case]):
        q0, k, v, do = operands(r, i)
        a = r["cu"][1 + i]
        H = heads
        q_all = r["qkv_c"][a:a + L, :H * 64].double().view(L, H, 64).transpose(0, 1)
        ob_d, obe_d, lse_dr, lsee_d = A.attn_fwd_ref(q_all, k, v, SCALE)                      # dense reference, all rows
        ob_c, obe_c, lse_cr, lsee_c = cls_fwd_ref(q0, k, v, SCALE, exact=False)
        o_d, o_c = r["out_d"][a].double().view(H, 64), r["o_c"][i].double().view(H, 64)
        assert bool(((ob_d[:, 0] - ob_c).abs() <= obe_d[:, 0] + obe_c).all()), "the two forward references disagree"
        assert bool(((o_d - o_c).abs() <= obe_d[:, 0] + obe_c).all()), f"[cls x dense {case}] out, length {L}"
        l_d, l_c = r["lse_d"][a].double(), r["lse_c"][i].double()
        assert bool(((l_d - l_c).abs() <= lsee_d[:, 0] + lsee_c).all()), f"[cls x dense {case}] lse, length {L}"
        # backward: both on the dense forward's out / lse
        do_rows = torch.zeros(H, L, 64, dtype=f64)
        do_rows[:, 0] = do
        o_rows = r["out_d"][a:a + L].double().view(L, H, 64).transpose(0, 1)
        l_rows = r["lse_d"][a:a + L].double().transpose(0, 1)
        dq_d, dqe_d, dk_d, dke_d, dv_d, dve_d = A.attn_bwd_ref(q_all, k, v, o_rows, l_rows, do_rows, SCALE)
        dq_c, dqe_c, dk_c, dke_c, dv_c, dve_c = cls_bwd_ref(q0, k, v, o_d, l_d, do, SCALE, exact=False)
        gd, gc = grads(r, r["dqkv_d"], i), grads(r, r["dqkv_3"], i)
        for name, x, y, e in (("dq", gd[0], gc[0], dqe_d), ("dk", gd[1], gc[1], dke_d + dke_c), ("dv", gd[2], gc[2], dve_d + dve_c)):
            if name == "dq":
                e = e.clone()
                e[:, 0] += dqe_c
            err = (x - y).abs()
            assert bool((err <= e).all()), f"[cls x dense {case} h{heads}] {name}, length {L}: {float((err - e).max()):.3g} past the summed bounds"
            nz = e > 0
            worst = max(worst, float((err[nz] / e[nz]).max()) if bool(nz.any()) else 0.0)
    print(f"[cls x dense {case} h{heads}] backward |difference| / summed bounds {worst:.3f}")
