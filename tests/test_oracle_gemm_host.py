"""What makes tests/test_gpu_gemm.py and tests/test_gpu_wgrad.py trustworthy without a GPU (tests/fp64_bounds.py is their oracle).

(a) Non-vacuity caps, as conditions on the oracle itself: for every case of the two GPU grids the bounds are computed here on the CPU
    (large-M cases on their first 512 rows).  For the zero-mean distributions at most 2 % of a case's 16-bit outputs may carry a bound
    wider than one 16-bit step of the reference value, and no fp32 output's bound may exceed 1e-4 (|A| |B|^T + |bias| + |resid|) at
    that element (same-sign distributions: K u times that sum).  The distributions of gemm_cases.operands were chosen to meet them.
    Only the GELU / GELU' forms on the `spread` distribution are not under the 2 % cap (gemm_cases.capped): their far-left tail gives
    outputs of 1e-6 whose bound is EPS_PHI |u| by construction.  The magnitude the fp32 cap multiplies is the one the epilogue forms:
    (|A| |B|^T + |bias|) times the DropPath scale and the dropout factor it applies to them, + |resid| (+ |pos| for the embed
    epilogue) -- looser than the unscaled sum by the dropout factor 1 / (1 - p) on kept elements, stricter (|resid| alone) where the
    scale or the factor is 0.
(b) Mutation self-test: a CPU emulation of the kernels (fp32 operands, k-blocks of 32 accumulated in fp32, fp32 epilogue, 16-bit
    rounding at the store) passes the oracle, and each seeded fault fails it -- on a bf16-output and on an fp32-output epilogue
    wherever the fault exists for both (DropPath scales exist only in the fp32 residual epilogue; a bf16 step and the tanh GELU only
    in bf16 outputs)."""
import math

import pytest
import torch

import fp64_bounds as fb
import gemm_cases as gc
from fp64_bounds import U, f32, f64, bf16

ROWS = 512


def _synthetic_drop(c, M, N):
    if not c["drop_p"] > 0:
        return None
    gen = torch.Generator()
    gen.manual_seed(gc.seed_of("drop", c["id"]))
    keep = torch.rand(M, N, generator=gen) >= c["drop_p"]
    return keep.double() * float(torch.tensor(1.0 / (1.0 - c["drop_p"]), dtype=f32))


def _magnitude(c, d, drop, k0=0, k1=None):
    """|A| |B|^T + |bias| (times the DropPath scale and dropout factor the epilogue applies to them) + |resid| (+ |pos|)."""
    A, B = d["A"][:, k0:k1].abs(), d["B"][:, k0:k1].abs()
    m = A @ B.t()
    if d.get("bias") is not None and c["epi"] not in (fb.EPI_DGELU_BF16, fb.EPI_ATOMIC_F32):
        m = m + d["bias"].abs()
    if drop is not None:
        m = m * drop
    if d.get("seq_scale") is not None:
        m = m * d["seq_scale"][d["row2seq"].long()][:, None].abs()
    if d.get("resid") is not None:
        m = m + d["resid"].abs()
    if d.get("pos") is not None:
        m = m + d["pos"][1 + torch.arange(A.shape[0]) % c["npatch"]].abs()
    return m


@pytest.mark.parametrize("c", gc.NT_CASES, ids=[c["id"] for c in gc.NT_CASES])
def test_nt_bounds_are_not_vacuous(c):
    d = gc.nt_inputs(c, rows=ROWS)
    M = d["A"].shape[0]
    drop = _synthetic_drop(c, M, c["N"])
    exp = gc.nt_expected(c, d, drop)
    slices = gc.nt_slices(c["K"], c["splits"])
    for name, (ref, bound, is16) in exp.items():
        assert bool(torch.isfinite(ref).all()) and bool(torch.isfinite(bound).all()) and bool((bound >= 0).all())
        if is16:
            if gc.capped(c):
                wide = (bound > fb.step16(ref, c["half"]) * (1 + 1e-9)).double().mean().item()
                assert wide <= 0.02, f"{c['id']} {name}: {100 * wide:.2f} % of the 16-bit outputs carry a bound wider than one step"
        else:
            k0, k1 = slices[int(name[2:-1])] if name.startswith("C[") else (0, None)
            K = (k1 or c["K"]) - k0
            cap = (K * U if c["dist"] == "positive" else 1e-4) * _magnitude(c, d, drop, k0, k1) * (1 + 1e-12)
            over = bound > cap
            assert not bool(over.any()), f"{c['id']} {name}: {int(over.sum())} fp32 bounds above the cap, worst ratio {float((bound / cap)[over].max()):.3g}"


@pytest.mark.parametrize("c", gc.TN_CASES, ids=[c["id"] for c in gc.TN_CASES])
def test_tn_bounds_are_not_vacuous(c):
    worst = c["dist"] == "positive"
    for (a, b, co, so), (n1, n2, acc, cs) in zip(gc.tn_inputs(c, rows=ROWS), gc.tn_items(c)):
        old = co if (acc or c["fn"] in ("tn_acc", "tn_part")) else None
        ref, bound = fb.gemm_tn(a, b, old, worst)
        mag = a.abs().t() @ b.abs() + (old.abs() if old is not None else 0)
        cap = (a.shape[0] * U if worst else 1e-4) * mag * (1 + 1e-12)
        assert bool(torch.isfinite(bound).all()) and not bool((bound > cap).any()), c["id"]
        sv, se = fb.colsum(a, so, worst)
        assert not bool((se > (a.shape[0] * U if worst else 1e-4) * (a.abs().sum(0) + so.abs()) * (1 + 1e-12)).any()), c["id"]


# ------------------------------------------------------------------------------------------------ the emulated kernels
FAULTS = {1: "last 32-wide k-block dropped", 2: "two k columns of A swapped", 3: "bias skipped on one column",
          4: "residual of the last partial column group taken from the previous group", 5: "dropout factors shifted by one column",
          6: "DropPath scale 1 for one sequence", 7: "one exact output moved by one bf16 step", 8: "one element between N and ldc written",
          9: "tanh GELU", 10: "TN: last M % 32 rows dropped", 11: "TN: one slice image added twice"}


def _acc(A, B, fault):
    A, B = A.float().clone(), B.float()
    K = A.shape[1]
    if fault == 2:
        A[:, [1, K - 2]] = A[:, [K - 2, 1]]
    acc = torch.zeros(A.shape[0], B.shape[0], dtype=f32)
    for k in range(0, K - (32 if fault == 1 else 0), 32):
        acc = acc + A[:, k:k + 32] @ B[:, k:k + 32].t()
    return acc


def _gelu32(x, tanh=False):
    if tanh:
        return 0.5 * x * (1 + torch.tanh(math.sqrt(2 / math.pi) * (x + 0.044715 * x ** 3)))
    return 0.5 * x * (1 + torch.erf(x * 0.70710678118654752))


def _stale_group(t, vpl, fault):
    """Fault 4: the last, partial group of `vpl` columns reads the group before it."""
    N = t.shape[1]
    t = t.float().clone()
    if fault == 4 and N % vpl and N > vpl:
        g0 = N - N % vpl
        t[:, g0:] = t[:, g0 - vpl:g0 - vpl + N % vpl]
    return t


def emulate_nt(c, d, drop, fault=0):
    """{name: tensor in the output's own dtype} of case c, as the kernel computes it, with seeded fault `fault`."""
    epi, N = c["epi"], c["N"]
    v = _acc(d["A"], d["B"], fault)
    if d.get("bias") is not None:
        b = d["bias"].float().clone()
        if fault == 3:
            b[N // 2] = 0
        v = v + b
    dr = None if drop is None else (torch.roll(drop, 1, 1) if fault == 5 else drop).float()
    if epi == fb.EPI_RESID_F32:
        if dr is not None:
            v = v * dr
        sc = d["seq_scale"].float().clone()
        if fault == 6:
            sc[4] = 1.0
        return {"C": _stale_group(d["resid"], 4, fault) + sc[d["row2seq"].long()][:, None] * v}
    if epi == fb.EPI_BF16_ACT:
        v = v + _stale_group(d["aux"], 8, fault)
        y = v * ((v + 3).clamp(0, 6) * (1.0 / 6)) if c["act"] == fb.ACT_HSWISH else v.clamp_min(0)
        return {"C": y.to(bf16)}
    if epi == fb.EPI_BF16_GELU:
        g = _gelu32(v, fault == 9)
        return {"C": v.to(bf16), "C2": (g if dr is None else g * dr).to(bf16)}
    if epi == fb.EPI_BF16:
        return {"C": v.to(bf16)}
    raise ValueError(epi)


def _judge(c, d, drop, got, guard=None):
    exp = gc.nt_expected(c, d, drop)
    for name, (ref, bound, is16) in exp.items():
        fb.check(f"{c['id']}: {name}", got[name], ref, bound, is16)
    if guard is not None:
        guard.intact(c["id"])


def _mut_case(tag):
    if tag == "act":      # bf16 output with bias and a 16-bit residual
        return gc.nt_case("mut-act", fb.EPI_BF16_ACT, 130, 100, 96, act=fb.ACT_HSWISH, aux=True)
    if tag == "gelu":     # bf16 outputs under dropout
        return gc.nt_case("mut-gelu", fb.EPI_BF16_GELU, 130, 100, 96, drop_p=0.5)
    if tag == "bf16":
        return gc.nt_case("mut-bf16", fb.EPI_BF16, 130, 100, 96, "onehot")
    return gc.nt_case("mut-resid", fb.EPI_RESID_F32, 130, 102, 96, drop_p=0.5)   # fp32 output: residual, DropPath, dropout


MUTATIONS = [("act", 1), ("resid", 1), ("act", 2), ("resid", 2), ("bf16", 2), ("act", 3), ("resid", 3), ("act", 4), ("resid", 4),
             ("gelu", 5), ("resid", 5), ("resid", 6), ("act", 7), ("bf16", 7), ("act", 8), ("resid", 8), ("gelu", 9)]


@pytest.mark.parametrize("tag", ["act", "gelu", "bf16", "resid"])
def test_the_emulated_kernel_passes(tag):
    c = _mut_case(tag)
    d = gc.nt_inputs(c)
    drop = _synthetic_drop(c, c["M"], c["N"])
    _judge(c, d, drop, emulate_nt(c, d, drop))


@pytest.mark.parametrize("tag,fault", MUTATIONS, ids=[f"{t}-fault{f}" for t, f in MUTATIONS])
def test_a_seeded_fault_fails(tag, fault):
    c = _mut_case(tag)
    d = gc.nt_inputs(c)
    drop = _synthetic_drop(c, c["M"], c["N"])
    got = emulate_nt(c, d, drop, fault if fault not in (7, 8) else 0)
    out = gc.Out(c["M"], c["N"], got["C"].dtype, "cpu").arm()
    out.v.copy_(got["C"])
    if fault == 7:
        ref, bound, _ = gc.nt_expected(c, d, drop)["C"]
        r, col = (((bound == 0) & (ref.abs() > 0.01)).nonzero()[7]).tolist()
        bits = out.v.view(torch.int16)
        bits[r, col] += 1
    if fault == 8:
        out.buf[0, 5, 8 + c["N"]] = 1.0                       # the first column behind the owned region
    got["C"] = out.v
    with pytest.raises(AssertionError):
        _judge(c, d, drop, got, out)
    print(f"rejected: {FAULTS[fault]} ({tag})")


def emulate_tn(a, b, slices=1, fault=0):
    M = a.shape[0]
    if fault == 10:
        M -= M % 32
    a, b = a.float(), b.float()
    step = -(-(-(-M // 32)) // slices) * 32
    imgs = []
    for m0 in range(0, M, step):
        acc = torch.zeros(a.shape[1], b.shape[1], dtype=f32)
        for m in range(m0, min(M, m0 + step), 32):
            e = min(M, m0 + step, m + 32)
            acc = acc + a[m:e].t() @ b[m:e]
        imgs.append(acc)
    if fault == 11:
        imgs.append(imgs[len(imgs) // 2])
    out = torch.zeros_like(imgs[0])
    for i in imgs:
        out = out + i
    return out


@pytest.mark.parametrize("dist", ["normal", "onehot", "positive"])
@pytest.mark.parametrize("fault", [0, 10, 11])
def test_tn_emulation_and_its_faults(dist, fault):
    c = gc.tn_case(f"mut-tn-{dist}", "wgrad", 777, 72, 200, dist, acc=False)
    (a, b, _, _), = gc.tn_inputs(c)
    ref, bound = fb.gemm_tn(a, b, None, dist == "positive")
    got = emulate_tn(a, b, slices=5, fault=fault)
    if fault == 0:
        fb.check(c["id"], got, ref, bound)
        return
    with pytest.raises(AssertionError):
        fb.check(c["id"], got, ref, bound)
    print(f"rejected: {FAULTS[fault]} ({dist})")
