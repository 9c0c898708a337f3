"""lafs_attention_probs (csrc/attention.hip): the attention probabilities the fused forward never stores, against an fp64 softmax of
the same bf16 qkv, at the sequence mixes of test_attention_fwd_bwd, for all query rows (q_rows = 0) and for the cls query alone
(q_rows = 1)."""
import ctypes as C

import pytest
import torch

pytestmark = pytest.mark.gpu

from lafs_cvpr2024_amd import _lib, ops  # noqa: E402
from lafs_cvpr2024_amd.ops import _p  # noqa: E402

DEV = "cuda"
bf16 = torch.bfloat16
CASES = [([197, 197], 2), ([37] * 5, 3), ([16, 1, 37, 48, 33], 1), ([100, 77], 2), ([197, 150], 6), ([256, 200], 1), ([160, 130, 9], 3),
         ([197] * 90, 3)]
# Elementwise error against fp64: |p - ref| / max(ref, FLOOR) -- relative for entries above FLOOR = 1e-4 (a fiftieth of the uniform
# weight 1/197), absolute in units of FLOOR below it.
FLOOR = 1e-4
GATE_ELEM = 2.4e-6      # observed 1.21e-6 on MI355X (worst of the 16 cases: 90 x 197 tokens, all query rows); gate = 2x
ROW_SUM_TOL = 5e-5      # <= 256 fp32 terms + the normalisation: (n + a few) 2^-24 < 2e-5


def rnd_bf(*shape, seed=0):
    g = torch.Generator().manual_seed(seed)
    return torch.randn(*shape, generator=g).to(bf16)


def _ref_probs(qkv, cu, heads, scale, max_len):
    """fp64 softmax of the bf16 operands -> [n_seq, heads, max_len, max_len], zero outside each sequence."""
    inner = heads * 64
    out = torch.zeros(len(cu) - 1, heads, max_len, max_len, dtype=torch.float64)
    for s in range(len(cu) - 1):
        x = qkv[cu[s]:cu[s + 1]].double()
        n = x.shape[0]
        q, k = (x[:, i * inner:(i + 1) * inner].view(n, heads, 64).transpose(0, 1) for i in range(2))
        out[s, :, :n, :n] = (q @ k.transpose(-1, -2) * scale).softmax(-1)
    return out


def _setup(lens, heads):
    cu = [0]
    for n in lens:
        cu.append(cu[-1] + n)
    qkv = rnd_bf(cu[-1], 3 * heads * 64, seed=11)
    return cu, qkv, torch.tensor(cu, dtype=torch.int32, device=DEV)


@pytest.mark.parametrize("q_rows", [0, 1])
@pytest.mark.parametrize("lens,heads", CASES)
def test_attention_probs_against_fp64(lens, heads, q_rows):
    cu, qkv, cud = _setup(lens, heads)
    scale, L = 64 ** -0.5, max(lens)
    qd = qkv.to(DEV)
    # the kernel owes every element of the buffer, zeros included: hand it one full of NaN
    p = ops.attention_probs(qd, cud, L, heads, scale, q_rows)
    junk = torch.full_like(p, float("nan"))
    _lib.call("lafs_attention_probs", _p(qd), qd.stride(0), _p(cud), len(lens), L, heads, scale, q_rows, _p(junk))
    assert torch.equal(p, junk)
    nq = q_rows or L
    assert p.shape == (len(lens), heads, nq, L) and p.dtype == torch.float32
    p = p.cpu()
    ref = _ref_probs(qkv, cu, heads, scale, L)[:, :, :nq]
    worst_sum = 0.0
    for s, n in enumerate(lens):
        assert bool((p[s, :, :, n:] == 0).all()) and bool((p[s, :, n:, :] == 0).all()), "padding must be exact zeros"
        worst_sum = max(worst_sum, (p[s, :, :min(n, nq), :n].double().sum(-1) - 1).abs().max().item())
    err = ((p.double() - ref).abs() / ref.clamp_min(FLOOR)).max().item()
    print(f"[attention_probs] lens {lens[:3]}..x{len(lens)} heads {heads} q_rows {q_rows}: elementwise {err:.3e} (gate {GATE_ELEM:.1e}), "
          f"row sums off by {worst_sum:.3e}")
    assert worst_sum < ROW_SUM_TOL
    assert err < GATE_ELEM


@pytest.mark.parametrize("lens,heads", CASES)
def test_cls_form_is_row_zero_of_the_full_form(lens, heads):
    cu, qkv, cud = _setup(lens, heads)
    full = ops.attention_probs(qkv.to(DEV), cud, max(lens), heads, 64 ** -0.5)
    cls = ops.attention_probs(qkv.to(DEV), cud, max(lens), heads, 64 ** -0.5, q_rows=1)
    assert torch.equal(cls, full[:, :, :1])
    some = ops.attention_probs(qkv.to(DEV), cud, max(lens), heads, 64 ** -0.5, q_rows=min(21, max(lens)))
    assert torch.equal(some, full[:, :, :some.shape[2]])


@pytest.mark.parametrize("lens,heads", CASES)
def test_read_out_reproduces_the_forward(lens, heads):
    """P V in fp64 from the read-out's fp32 P and the bf16 v == what lafs_attention_fwd wrote, element by element.  Both kernels form
    the same fp32 scores, maximum and sum; the forward rounds its un-normalised weights e_j = p_j / max_j p_j to bf16 for its MFMA
    (half an ulp each: at most 2^-9 of the upper end of e_j's binade) and its output to bf16.  Where that leaves no bf16 rounding
    boundary within reach the two must agree exactly."""
    cu, qkv, cud = _setup(lens, heads)
    scale, inner = 64 ** -0.5, heads * 64
    qd = qkv.to(DEV)
    out, _ = ops.attention_fwd(qd, cud, max(lens), heads, scale)
    p = ops.attention_probs(qd, cud, max(lens), heads, scale)
    out, p = out.double().cpu(), p.double().cpu()
    rbf = lambda t: t.float().to(bf16).double()
    worst, exact, total = 0.0, 0, 0
    for s, n in enumerate(lens):
        v = qkv[cu[s]:cu[s + 1], 2 * inner:].double().view(n, heads, 64).transpose(0, 1)
        ps = p[s, :, :n, :n]
        pmax = ps.max(-1, keepdim=True).values
        e = ps / pmax
        # the read-out's own normalisation (v_rcp_f32 and a product: 3 roundings, so e is known to 2^-22); the bf16 rounding of e;
        # the forward's fp32 accumulation over the padded keys, its v_rcp_f32 and product
        top = torch.exp2(torch.floor(torch.log2(e * (1 + 2.0 ** -22))) + 1)
        pv, pva = ps @ v, ps @ v.abs()
        bound = (2.0 ** -9 * top * pmax) @ v.abs() + (n + 24) * 2.0 ** -24 * pva
        r = rbf(pv)
        bound = torch.maximum(rbf(pv + bound) - r, r - rbf(pv - bound))          # the output's bf16 flip
        got = out[cu[s]:cu[s + 1]].view(n, heads, 64).transpose(0, 1)
        err = (got - r).abs()
        assert bool((err <= bound).all()), f"sequence {s}: worst |error| / bound {float((err / bound.clamp_min(1e-300)).max()):.3g}"
        nz = bound > 0
        worst = max(worst, float((err[nz] / bound[nz]).max()) if bool(nz.any()) else 0.0)
        exact, total = exact + int((~nz).sum()), total + bound.numel()
    print(f"[attention_probs] P V vs forward: worst |error| / bound {worst:.3f}, exact (bound 0) {100.0 * exact / total:.1f} %")


def test_invalid_arguments_raise():
    cu, qkv, cud = _setup([37, 20], 2)
    qd = qkv.to(DEV)
    for kw in (dict(max_len=257), dict(heads=0), dict(heads=-2), dict(q_rows=-1), dict(q_rows=38)):
        a = dict(max_len=37, heads=2, q_rows=0); a.update(kw)
        with pytest.raises(_lib.LafsHipError):
            ops.attention_probs(qd, cud, a["max_len"], a["heads"], 0.125, a["q_rows"])
    out = torch.empty(2, 2, 37, 37, device=DEV)
    for args in ((None, _p(cud), _p(out)), (_p(qd), None, _p(out)), (_p(qd), _p(cud), None)):
        with pytest.raises(_lib.LafsHipError, match="null"):
            _lib.call("lafs_attention_probs", args[0], qd.stride(0), args[1], 2, 37, 2, 0.125, 0, args[2])
