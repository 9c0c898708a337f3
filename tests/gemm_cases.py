"""The case grids of tests/test_gpu_gemm.py and tests/test_gpu_wgrad.py, their seeded input distributions, what the oracle of
tests/fp64_bounds.py expects for a case, and the NaN-guarded buffers the operands and outputs live in.  Kept apart from the GPU modules
so that tests/test_oracle_gemm_host.py judges on the CPU exactly the cases the GPU runs."""
import math
import zlib

import torch

from fp64_bounds import (ACT_HSIGMOID, ACT_HSWISH, ACT_NONE, ACT_RELU, EPI_ATOMIC_F32, EPI_BF16, EPI_BF16_ACT, EPI_BF16_GELU,  # noqa: F401
                         EPI_DGELU_BF16, EPI_EMBED_F32, EPI_F32, EPI_RESID_F32, F32_EPIS, U, bf16, f16, f32, f64, nt_reference, rbf, rh)


def seed_of(*k):
    return zlib.crc32(repr(k).encode())


# ------------------------------------------------------------------------------------------------ input distributions
DISTS = ("normal", "cancel", "positive", "onehot", "ramp", "spread", "zeros")


def capped(c):
    """Whether the 2 % cap of test_oracle_gemm_host.py holds for the 16-bit outputs of NT case c: every distribution but the same-sign
    one (the cap is stated for zero-mean inputs), and but the GELU / GELU' forms on `spread` -- in the far left tail gelu(u) and
    gelu'(u) sink below EPS_PHI |u|, so a fifth of those outputs carry a wide bound whatever the operands are."""
    return c["dist"] != "positive" and not (c["dist"] == "spread" and c["epi"] in (EPI_BF16_GELU, EPI_DGELU_BF16))

NNZ = 128


def _thin(x, gen, keep):
    if keep >= 1.0:
        return x
    return x * (torch.rand(x.shape, generator=gen) < keep)


def operands(dist, R, C1, C2, gen, nnz=NNZ):
    """The two 16-bit operands of a contraction of length R (K of the NT product, M of the TN one), as fp64 [C1, R] and [C2, R] (the
    caller transposes for TN).
    normal:   zero-mean normal; products of variance 1 / R.  Beyond R = 128 each entry of the first operand is kept with probability
              128 / R: sum|terms| -- and with it the bound -- grows like the number of non-zero products while the output's own
              spread grows like its root, so a dense long reduction would put a rounding boundary within reach of a growing share of
              the 16-bit outputs (the 2 % cap of the host module); which entries are zero differs per row, so every k is still used
    cancel:   the same, plus three pairs of large terms per row that cancel exactly (+L b, -L b)
    positive: all-positive (the same-sign case: takes the worst-case bound)
    onehot:   rows of the first operand hold a single 1, every third row a second one: each output is exactly an element of the
              second operand, or a sum of two -- any permutation of k between the operands shows up as a wrong exact value
    ramp:     the second operand is a k-dependent ramp of small integers / 64 (exact in 16 bits)
    spread:   normal (the caller spreads the pre-activations with the bias)
    zeros:    a zero first operand"""
    rn = lambda *s: torch.randn(*s, generator=gen, dtype=f64)
    keep = min(1.0, nnz / R)
    if dist in ("normal", "spread", "cancel", "ramp"):
        a = _thin(rn(C1, R), gen, keep)
        b = rn(C2, R) / math.sqrt(min(R, nnz))
        if dist == "ramp":
            k, n = torch.arange(R)[None, :], torch.arange(C2)[:, None]
            b = (((k * 37 + n * 11) % 127) - 63).double() / 64
        if dist == "cancel" and R >= 8:
            for j in range(3):
                k1, k2 = (5 * j + 1) % R, (R - 1 - 3 * j) % R
                if k1 == k2:
                    continue
                L = 16.0 * (1 + torch.randint(0, 3, (C1,), generator=gen).double())
                a[:, k1], a[:, k2] = L, L
                b = rbf(b)
                b[:, k2] = -b[:, k1]
        return a, b
    if dist == "positive":
        return rn(C1, R).abs(), rn(C2, R).abs() / R
    if dist == "onehot":
        a = torch.zeros(C1, R, dtype=f64)
        r = torch.arange(C1)
        a[r, torch.randint(0, R, (C1,), generator=gen)] = 1.0
        a[r[::3], torch.randint(0, R, (r[::3].numel(),), generator=gen)] = 1.0
        return a, rn(C2, R)
    if dist == "zeros":
        return torch.zeros(C1, R, dtype=f64), rn(C2, R)
    raise ValueError(dist)


# ------------------------------------------------------------------------------------------------ the NT grid
SEQ_SCALE = [0.0, 1 / 0.9, 1.25, 0.0, 0.5, 1 / 0.9, 2.0]          # per-sequence DropPath scales, zeros included


def nt_case(cid, epi, M, N, K, dist="normal", **kw):
    """bias: None = wherever the epilogue takes one.  form: BF16_GELU 'u' / 'noC' / 'save', DGELU_BF16 'u' / 'save'.  seed: the id of
    the case whose operands this one shares (an A/B partner under another LAFS_OPT_* value); dense: no thinning of long reductions."""
    c = dict(id=cid, epi=epi, M=M, N=N, K=K, dist=dist, bias=None, half=False, act=0, aux=False, form="u", splits=1, scale="vec",
             alias=False, drop_p=0.0, drop_row0=0, drop_step=None, route=None, opts=None, npatch=0, seed=None, dense=False)
    c.update(kw)
    if c["bias"] is None:
        c["bias"] = epi not in (EPI_DGELU_BF16, EPI_ATOMIC_F32) and not (epi == EPI_F32 and c["splits"] > 1)
    if epi == EPI_EMBED_F32 and not c["npatch"]:
        c["npatch"] = next(p for p in (7, 5, 4, 3, 2, 1) if M % p == 0)
    return c


# every epilogue form the tiled kernel (route 0) accepts: (tag, epilogue, options)
FORMS = [
    ("bf16", EPI_BF16, {}), ("gelu_u", EPI_BF16_GELU, {}), ("gelu_noC", EPI_BF16_GELU, dict(form="noC")),
    ("gelu_save", EPI_BF16_GELU, dict(form="save")), ("resid", EPI_RESID_F32, {}), ("f32", EPI_F32, {}),
    ("dgelu_u", EPI_DGELU_BF16, {}), ("dgelu_save", EPI_DGELU_BF16, dict(form="save")), ("atomic", EPI_ATOMIC_F32, {}),
    ("embed", EPI_EMBED_F32, {}), ("act_hswish_aux", EPI_BF16_ACT, dict(act=ACT_HSWISH, aux=True)),
    ("act_relu", EPI_BF16_ACT, dict(act=ACT_RELU)),
]
ACT_NAME = {ACT_NONE: "none", ACT_RELU: "relu", ACT_HSWISH: "hswish", ACT_HSIGMOID: "hsigmoid"}
OPT_KRES_MASK, OPT_NT_WIDE, OPT_NT_TALL, OPT_NT_BIG = 2, 4, 5, 7          # LAFS_OPT_*


def _nt_grid():
    g = []
    add = lambda *a, **k: g.append(nt_case(*a, **k))
    # N % 8 != 0: the per-element tail branches exist per epilogue, so every such N runs every form (ldc padded to a multiple of 8)
    for N in (4, 12, 36, 100, 197, 1001):
        for tag, epi, o in FORMS:
            add(f"tail-N{N}-{tag}<2,32>", epi, 140 if epi == EPI_EMBED_F32 else 129, N, 64, route=0, **o)
    for M in (1, 15, 16, 17, 127, 128, 129, 159, 160, 161, 255, 257):
        add(f"rows-M{M}-bf16<2,32>", EPI_BF16, M, 200, 96, route=0)
        add(f"rows-M{M}-resid<2,32>", EPI_RESID_F32, M, 200, 96, route=0, scale="zeros" if M % 2 else "vec")
    # K: 1, 2, 3 stages (fewer than the ring depth); the bk64 threshold and K % 64 != 0 above it
    for K in (32, 64, 96, 608, 640, 672, 704):
        inst = "<2,64>" if K % 64 == 0 and K >= 640 else "<2,32>"
        add(f"depth-K{K}-bf16{inst}", EPI_BF16, 257, 136, K, route=0)
        add(f"depth-K{K}-f32{inst}", EPI_F32, 257, 132, K, route=0)
        add(f"depth-K{K}-gelu_save{inst}", EPI_BF16_GELU, 130, 264, K, route=0, form="save")
    # K splits: F32 images (704 + 640 on 64-deep stages, 64 + 32), atomics with 1, 2 and more slices than K / 32
    add("ksplit-f32-K1344x2<2,64>", EPI_F32, 200, 136, 1344, splits=2, route=0)
    add("ksplit-f32-K96x2<2,32>", EPI_F32, 200, 132, 96, splits=2, route=0)
    add("ksplit-f32-K672x3-N100<2,32>", EPI_F32, 130, 100, 672, splits=3, route=0)
    for sp in (1, 2, 1000):
        add(f"atomic-splits{sp}-K96<2,32>", EPI_ATOMIC_F32, 200, 136, 96, splits=sp, route=0)
    add("atomic-splits4-K1344<2,32>", EPI_ATOMIC_F32, 130, 100, 1344, splits=4, route=0)
    # 256x128 tiles (wm == 4: N >= 1024, M >= 4096, K < 640), with and without a K split
    add("wm4-bf16<4,32>", EPI_BF16, 4100, 1032, 96, route=0)
    add("wm4-resid-N1028<4,32>", EPI_RESID_F32, 4100, 1028, 160, route=0)
    add("wm4-gelu_u<4,32>", EPI_BF16_GELU, 4097, 1024, 64, route=0)
    add("wm4-ksplit-f32-K96x2<4,32>", EPI_F32, 4100, 1028, 96, splits=2, route=0)
    add("wm4-atomic-splits3<4,32>", EPI_ATOMIC_F32, 4100, 1024, 96, splits=3, route=0)
    # ... and on both sides of its thresholds (the route is 0 on either side: the values tell, and test_host_logic.py reads the plan)
    add("wm4-threshold-M4096-N1024<4,32>", EPI_BF16, 4096, 1024, 96, route=0)
    add("wm4-threshold-M4095-N1024<2,32>", EPI_BF16, 4095, 1024, 96, route=0)
    add("wm4-threshold-M4096-N1016<2,32>", EPI_BF16, 4096, 1016, 96, route=0)
    add("wm4-threshold-M4096-K608<4,32>", EPI_BF16, 4096, 1024, 608, route=0)
    # fp16 operands (operand_f16) at both stage depths
    for K, inst in ((96, "<2,32,2,true>"), (704, "<2,64,2,true>")):
        # (an fp16 step is 8x finer than a bf16 one: on the long reduction the K u |bias| term alone reaches it, so the 16-bit outputs
        # there run without a bias -- the activation case gets its pre-activations around +-3 from the residual -- and on 4 products
        # per output; the fp32 outputs keep the bias, one of them on dense operands, which is what pins this instantiation's fp32
        # accumulation over the whole K)
        add(f"f16-bf16-K{K}{inst}", EPI_BF16, 257, 136, K, half=True, route=0, bias=K < 640)
        add(f"f16-bf16-N100-K{K}{inst}", EPI_BF16, 130, 100, K, half=True, route=0, bias=K < 640)
        add(f"f16-f32-K{K}{inst}", EPI_F32, 130, 100, K, half=True, route=0)
        add(f"f16-f32-dense-K{K}{inst}", EPI_F32, 257, 136, K, half=True, dense=True, route=0)
        add(f"f16-act_hswish_aux-K{K}{inst}", EPI_BF16_ACT, 257, 132, K, "spread", half=True, act=ACT_HSWISH, aux=True, route=0, bias=K < 640)
    add("f16-onehot<2,32,2,true>", EPI_BF16, 130, 136, 96, "onehot", half=True, bias=False, route=0)
    # BF16_ACT: 4 activations x aux present / NULL x bf16 / fp16, pre-activations around the kinks at +-3
    for half in (False, True):
        for a in range(4):
            for aux in (False, True):
                # (fp16: K = 32 keeps K u |bias| under the finer step)
                add(f"act-{ACT_NAME[a]}-{'aux' if aux else 'noaux'}-{'f16<2,32,2,true>' if half else 'bf16<2,32>'}", EPI_BF16_ACT, 130, 100,
                    32 if half else 64, "spread", act=a, aux=aux, half=half, route=0)
    # route 3: 128x384 / 12 waves (N % 384 == 0, 160..256 tiles); LAFS_OPT_NT_WIDE = 0 is its A/B partner on the same operands (`seed`:
    # the GPU module also holds the two kernels' outputs against each other, within the sum of their bounds)
    for tag, epi in (("bf16", EPI_BF16), ("resid", EPI_RESID_F32)):
        add(f"route3-{tag}<2,64,6>", epi, 20500, 384, 768, route=3)
        add(f"route3-{tag}-NT_WIDE0<2,64>", epi, 20500, 384, 768, route=0, opts={OPT_NT_WIDE: 0}, seed=f"route3-{tag}<2,64,6>")
    # ... and its thresholds: 160 and 256 tiles of 128 rows are in, 159 and 257 are out
    for M, r in ((159 * 128, 0), (160 * 128, 3), (256 * 128, 3), (256 * 128 + 1, 0)):
        add(f"route3-threshold-M{M}-bf16{'<2,64,6>' if r else '<2,64>'}", EPI_BF16, M, 384, 640, route=r)
    add("route3-onehot-bf16<2,64,6>", EPI_BF16, 20500, 384, 640, "onehot", bias=False, route=3)
    # route 4: 160-row tiles (N = 500 keeps gemm_big.hip out); LAFS_OPT_NT_TALL = 0 is the partner
    for tag, epi, o in FORMS[:1] + FORMS[3:5] + FORMS[6:8] + FORMS[1:2]:
        add(f"route4-{tag}<2,64,2,false,5>", epi, 16400, 500, 640, route=4, **o)
    add("route4-bf16-NT_TALL0<2,64>", EPI_BF16, 16400, 500, 640, route=0, opts={OPT_NT_TALL: 0}, seed="route4-bf16<2,64,2,false,5>")
    # ... and its thresholds at 4 tile columns: 513 tiles of 128 rows spill into a second round (512 do not), 512 tiles of 160 rows
    # still fit one (516 do not)
    for M, r in ((16384, 0), (16385, 4), (20480, 4), (20481, 0)):
        add(f"route4-threshold-M{M}-bf16{'<2,64,2,false,5>' if r else '<2,64>'}", EPI_BF16, M, 500, 640, route=r)
    add("route4-onehot-resid<2,64,2,false,5>", EPI_RESID_F32, 16400, 500, 704, "onehot", route=4)
    # route 1: the K-resident kernel (K = 384), and the same operands with LAFS_OPT_KRES_MASK = 0 on the tiled kernel
    for tag, epi, o in FORMS[:5] + FORMS[6:8]:
        add(f"route1-{tag}", epi, 2100, 192, 384, route=1, **o)
        add(f"route1-{tag}-KRES_MASK0<2,32>", epi, 2100, 192, 384, route=0, opts={OPT_KRES_MASK: 0}, seed=f"route1-{tag}", **o)
    add("route1-onehot-bf16", EPI_BF16, 2177, 1536, 384, "onehot", bias=False, route=1)
    # ... and its thresholds: M >= 2048, 64 <= N <= 1536 in steps of 64
    for M, N, r in ((2047, 64, 0), (2048, 64, 1), (2048, 1536, 1), (2048, 1600, 0), (2048, 56, 0), (2048, 96, 0)):
        add(f"route1-threshold-M{M}-N{N}-bf16{'' if r else '<2,32>'}", EPI_BF16, M, N, 384, route=r)
    add("route1-dropout-falls-back-resid<2,32>", EPI_RESID_F32, 2100, 192, 384, drop_p=0.1, route=0)
    # route 5: gemm_big.hip, its default geometry choice and the three forced ones
    for big in (1, 2, 3, 4):
        for tag, epi, o in (FORMS[0], FORMS[3], FORMS[4], FORMS[7]):
            if big == 1:      # the default: eligible by its own fill rule (the residual epilogue only from three rounds of tiles on)
                add(f"route5-NT_BIG1-{tag}", epi, 26048 if epi == EPI_RESID_F32 else 8685, 1016, 1024, route=5, **o)
            else:
                add(f"route5-NT_BIG{big}-{tag}", epi, 12300, 776, 1024, route=5, opts={OPT_NT_BIG: big}, **o)
    add("route5-NT_BIG2-dgelu_u", EPI_DGELU_BF16, 8200, 520, 512, route=5, opts={OPT_NT_BIG: 2})
    add("route5-NT_BIG2-onehot-bf16", EPI_BF16, 8200, 520, 576, "onehot", bias=False, route=5, opts={OPT_NT_BIG: 2})
    add("route5-NT_BIG0-bf16<2,64>", EPI_BF16, 12300, 776, 1024, route=0, opts={OPT_NT_BIG: 0, OPT_NT_TALL: 0}, seed="route5-NT_BIG2-bf16")
    # ... and its thresholds (forced geometry: eligibility alone decides): M >= 8192, N >= 512, K >= 512
    for M, N, K, r in ((8191, 512, 512, 0), (8192, 512, 512, 5), (8192, 504, 512, 0), (8192, 512, 448, 0)):
        add(f"route5-threshold-M{M}-N{N}-K{K}-bf16{'' if r else '<2,32>'}", EPI_BF16, M, N, K, route=r, opts={OPT_NT_BIG: 2})
    # dropout: the factor matrix of lafs_debug_dropout_mask feeds the oracle
    for p in (0.1, 0.5):
        add(f"drop-p{p}-resid<2,32>", EPI_RESID_F32, 130, 100, 96, drop_p=p, route=0)
        add(f"drop-p{p}-gelu_u-C2only<2,32>", EPI_BF16_GELU, 130, 100, 96, drop_p=p, route=0)
        add(f"drop-p{p}-gelu_save<2,32>", EPI_BF16_GELU, 257, 136, 96, drop_p=p, form="save", route=0)
        add(f"drop-p{p}-dgelu_u<2,32>", EPI_DGELU_BF16, 130, 100, 96, drop_p=p, route=0)
        add(f"drop-p{p}-dgelu_save<2,64>", EPI_DGELU_BF16, 257, 136, 640, drop_p=p, form="save", route=0)
    add("drop-row0-resid<2,32>", EPI_RESID_F32, 130, 100, 96, drop_p=0.5, drop_row0=77, route=0)
    add("drop-row0-dgelu_u<2,32>", EPI_DGELU_BF16, 130, 136, 96, drop_p=0.1, drop_row0=300, route=0)
    add("drop-step-resid<2,32>", EPI_RESID_F32, 130, 100, 96, drop_p=0.5, drop_step=5, route=0)
    add("drop-step-row0-gelu_noC<2,32>", EPI_BF16_GELU, 130, 136, 96, drop_p=0.1, drop_step=3, drop_row0=40, form="noC", route=0)
    add("drop-route5-resid", EPI_RESID_F32, 8200, 520, 512, drop_p=0.1, route=5, opts={OPT_NT_BIG: 2})
    # residual forms
    add("resid-inplace<2,32>", EPI_RESID_F32, 257, 136, 96, alias=True, route=0)
    add("resid-inplace-N100<2,64>", EPI_RESID_F32, 257, 100, 640, alias=True, route=0)
    add("resid-noscale<2,32>", EPI_RESID_F32, 257, 100, 96, scale=None, route=0)
    add("resid-zeroscales<2,32>", EPI_RESID_F32, 257, 136, 96, scale="zeros", route=0)
    add("resid-nobias<2,32>", EPI_RESID_F32, 130, 100, 96, bias=False, route=0)
    add("embed-npatch49<2,32>", EPI_EMBED_F32, 490, 384, 192, npatch=49, route=0)
    # the input distributions, on a 16-bit and an fp32 output, short and long reductions
    for dist in DISTS:
        for K, inst in ((160, "<2,32>"), (704, "<2,64>")):
            nb = dict(bias=False) if dist in ("onehot", "zeros") else {}
            add(f"dist-{dist}-bf16-K{K}{inst}", EPI_BF16, 200, 136, K, dist, route=0, **nb)
            # (all-positive: the plain fp32 store -- the K u cap of the host module leaves no room for the residual epilogue's roundings)
            if dist == "positive":
                add(f"dist-{dist}-f32-K{K}{inst}", EPI_F32, 200, 100, K, dist, route=0)
            else:
                add(f"dist-{dist}-resid-K{K}{inst}", EPI_RESID_F32, 200, 100, K, dist, route=0)
    for tag, epi, o in FORMS[1:4] + FORMS[6:7]:
        add(f"dist-spread-{tag}<2,32>", epi, 257, 136, 96, "spread", route=0, **o)
    ids = [c["id"] for c in g]
    assert len(set(ids)) == len(ids)
    return g


NT_CASES = _nt_grid()


def nt_inputs(c, rows=None):
    """The operands of case c as fp64 CPU tensors holding exactly representable 16-bit / fp32 values, derived from a crc32 seed of the
    case id.  rows: keep only the first `rows` rows (the host module's view of a large-M case)."""
    gen = torch.Generator()
    gen.manual_seed(seed_of("nt", c["seed"] or c["id"]))
    M, N, K, epi, dist = c["M"], c["N"], c["K"], c["epi"], c["dist"]
    r16 = rh if c["half"] else rbf
    rn = lambda *s: torch.randn(*s, generator=gen, dtype=f64)
    rf = lambda v: v.to(f32).double()
    a, b = operands(dist, K, M, N, gen, nnz=K if c["dense"] else 4 if c["half"] and (K > 128 or dist == "spread") else NNZ)
    if dist == "spread":
        b = b * 1.5
    d = dict(A=r16(a), B=r16(b))
    sign = lambda n: torch.randint(0, 2, (n,), generator=gen).double() * 2 - 1
    if c["bias"]:
        # magnitudes in [0.75, 3]: sets the outputs apart from 0 (see `operands`) and, for the GELU / activation epilogues, spreads the
        # pre-activations over both tails and the kinks at +-3
        mag = 0.75 + 2.25 * torch.rand(N, generator=gen, dtype=f64)
        if dist == "spread":
            mag = 6 * torch.rand(N, generator=gen, dtype=f64)
            mag[::5] = 3.0
        # (GELU outside `spread`: positive biases keep u out of the far left tail, where gelu(u) ~ 1e-5 sits below EPS_PHI |u|)
        d["bias"] = rf(mag * (1.0 if dist == "positive" or (epi == EPI_BF16_GELU and dist != "spread") else sign(N)))
    if epi == EPI_RESID_F32:
        d["resid"] = rf(rn(M, N).abs() if dist == "positive" else rn(M, N))
        nseq = len(SEQ_SCALE)
        d["row2seq"] = torch.randint(0, nseq, (M,), generator=gen, dtype=torch.int32)
        if c["scale"] is not None:
            sc = torch.tensor(SEQ_SCALE, dtype=f64) if c["scale"] == "vec" else torch.zeros(nseq, dtype=f64)
            if c["scale"] == "zeros":
                sc[2] = 1.0
            d["seq_scale"] = rf(sc)
    if epi == EPI_DGELU_BF16:
        # the stored gelu'(u), or the pre-activation u: over [-6, 6] for `spread`, else over [-2.5, 4] (further left gelu'(u) sinks below
        # EPS_PHI and every output's bound would be wide); a tenth of them exactly 0
        lo, hi = (-6.0, 6.0) if dist == "spread" else (-2.5, 4.0)
        d["aux"] = rbf(torch.rand(M, N, generator=gen, dtype=f64) * 1.4 - 0.2) if c["form"] == "save" else \
            rbf((torch.rand(M, N, generator=gen, dtype=f64) * (hi - lo) + lo) * (torch.rand(M, N, generator=gen) < 0.9))
    if epi == EPI_BF16_ACT and c["aux"]:
        d["aux"] = r16(rn(M, N))
        if dist == "spread" and not c["bias"]:            # the 16-bit residual places the pre-activations: over [-6, 6], a fifth at +-3
            mag = 6 * torch.rand(M, N, generator=gen, dtype=f64)
            mag[:, ::5] = 3.0
            d["aux"] = r16(mag * (torch.randint(0, 2, (M, N), generator=gen).double() * 2 - 1))
    if epi == EPI_EMBED_F32:
        d["pos"] = rf(rn(c["npatch"] + 1, N))
    if rows is not None and rows < M:
        for k in ("A", "resid", "row2seq", "aux"):
            if k in d:
                d[k] = d[k][:rows]
    return d


def nt_slices(K, splits):
    """K slices of lafs_gemm_nt for `splits` (ksplit_len of gemm.hip restated: whole 32-deep stages, 64-deep ones for long slices of a
    K that is a multiple of 64) -- the GPU module checks the count against lafs_gemm_nt_slices."""
    ksteps = K // 32
    sp = max(1, min(splits, ksteps))
    klen = -(-ksteps // sp) * 32
    if K % 64 == 0 and klen >= 640:
        klen = (klen + 63) // 64 * 64
    return [(k0, min(K, k0 + klen)) for k0 in range(0, K, klen)]


def nt_expected(c, d, drop=None):
    """{name: (reference, bound, 16-bit?)} of case c for inputs d (fp64, any device); the K-split F32 form returns one entry per slice
    image ("C[i]") and "sum" for lafs_sum_slices."""
    epi = c["epi"]
    s = None
    if epi == EPI_RESID_F32 and d.get("seq_scale") is not None:
        s = d["seq_scale"][d["row2seq"].long()][:, None]
    pos_rows = None
    if epi == EPI_EMBED_F32:
        pos_rows = d["pos"][1 + torch.arange(d["A"].shape[0], device=d["A"].device) % c["npatch"]]
    kw = dict(bias=d.get("bias"), res=d.get("resid"), s=s, drop=drop, aux=d.get("aux"), pos_rows=pos_rows, act_kind=c["act"],
              save_grad=c["form"] == "save", half=c["half"], worst=c["dist"] == "positive")
    if epi == EPI_F32 and c["splits"] > 1:
        out, tot, tote = {}, 0, 0
        for i, (k0, k1) in enumerate(nt_slices(c["K"], c["splits"])):
            v, e, _ = nt_reference(epi, d["A"][:, k0:k1], d["B"][:, k0:k1], **kw)["C"]
            out[f"C[{i}]"] = (v, e, False)
            tot, tote = tot + v, tote + e
        out["sum"] = (tot, tote + len(out) * U * tot.abs(), False)
        return out
    if epi == EPI_ATOMIC_F32:
        kw["n_atomic"] = len(nt_slices(c["K"], c["splits"]))
    return nt_reference(epi, d["A"], d["B"], **kw)


# ------------------------------------------------------------------------------------------------ the TN grid
VIT_S, VIT_B = (384, 1152, 1536), (768, 2304, 2048)          # dim, qkv width, hidden width of the two ViTs' blocks


def block_shapes(vit):
    """(N1, N2) of the four weight gradients dY^T X of a block: proj, qkv, fc1, fc2."""
    d, q, h = vit
    return [(d, d), (q, d), (h, d), (d, h)]



def tn_case(cid, fn, M, N1, N2, dist="normal", **kw):
    c = dict(id=cid, fn=fn, M=M, N1=N1, N2=N2, dist=dist, splits=0, acc=True, colsum=False, half=False, items=1, wg=0, vit="s")
    c.update(kw)
    return c


def _tn_grid():
    g = []
    add = lambda *a, **k: g.append(tn_case(*a, **k))
    small = [(8, 8), (72, 200), (200, 72), (200, 200), (8, 200)]
    for M in (1, 31, 32, 33, 130, 777, 4099):
        for i, (n1, n2) in enumerate(small):
            if (M + i) % 2 == 0 or M in (33, 777):
                add(f"tn_acc-128x128-M{M}-{n1}x{n2}", "tn_acc", M, n1, n2, colsum=(i % 2 == 0))
                add(f"wgrad-M{M}-{n1}x{n2}-acc{i % 2}", "wgrad", M, n1, n2, acc=bool(i % 2), colsum=(i % 2 == 1))
    for sp in (0, 1, 3, 8, 16, 1000):
        add(f"tn_acc-128x128-splits{sp}", "tn_acc", 777, 200, 136, splits=sp, colsum=True)
    # the wide tiles: splits <= 0, M >= 8192, more than 768 tile-slices
    add("tn_acc-256x128-M8200-1152x768", "tn_acc", 8200, 1152, 768, colsum=True)
    add("tn_acc-128x256-M8200-768x1160", "tn_acc", 8200, 768, 1160)
    add("tn_acc-256x128-onehot", "tn_acc", 8195, 896, 776, "onehot")
    add("tn_acc-128x256-onehot", "tn_acc", 8195, 776, 896, "onehot", colsum=True)
    add("tn_acc-M44160-200x72", "tn_acc", 44160, 200, 72, colsum=True)
    # ... on both sides of the wide tiles' M >= 8192
    add("tn_acc-256x128-threshold-M8192", "tn_acc", 8192, 1152, 768, colsum=True)
    add("tn_acc-128x128-threshold-M8191", "tn_acc", 8191, 1152, 768, colsum=True)
    # the block shapes of both ViTs (ViT-B's qkv gradient, 2304 x 768, is the shape the 256x128 tile exists for)
    for name, vit in (("vit_s", VIT_S), ("vit_b", VIT_B)):
        for tag, (n1, n2) in zip(("proj", "qkv", "fc1", "fc2"), block_shapes(vit)):
            add(f"tn_acc-{name}-{tag}-M8200-{n1}x{n2}", "tn_acc", 8200, n1, n2, colsum=tag != "proj")
            if (name, tag) not in (("vit_s", "fc1"), ("vit_b", "proj")):
                add(f"wgrad-{name}-{tag}-M4099-{n1}x{n2}", "wgrad", 4099, n1, n2, acc=tag == "qkv", colsum=tag != "fc2")
    for dist in DISTS:
        if dist != "spread":
            add(f"tn_acc-dist-{dist}", "tn_acc", 777, 136, 200, dist, colsum=True)
            add(f"wgrad-dist-{dist}", "wgrad", 777, 136, 200, dist, colsum=True, acc=False)
            add(f"tn_part-dist-{dist}", "tn_part", 777, 136, 72, dist)
    for M in (1, 33, 4099):
        add(f"tn_part-M{M}-72x200", "tn_part", M, 72, 200, colsum=True)
    add("tn_part-splits16-M4099", "tn_part", 4099, 200, 200, splits=16)
    add("tn_part-M44160-384x384", "tn_part", 44160, 384, 384)
    for M in (31, 130, 4099):
        add(f"wgrad_f16-M{M}-72x200", "wgrad_f16", M, 72, 200, half=True, acc=(M == 130), colsum=(M != 31))
    add("wgrad_f16-onehot", "wgrad_f16", 777, 200, 136, "onehot", half=True, acc=False)
    add("wgrad-M44160-vit_s-fc1", "wgrad", 44160, 1536, 384, acc=False, colsum=True)
    add("wgrad-M4099-vit_b-proj", "wgrad", 4099, 768, 768, acc=True)
    # groups: 1, 2, 4, 8 items, the workgroup budgets, strided column slices of a fused qkv buffer
    for n, wg in ((1, 0), (2, 8), (4, 160), (8, 0), (4, 8)):
        add(f"group-{n}items-wg{wg}-M777", "group", 777, 0, 0, items=n, wg=wg)
    add("group-4items-wg160-vit_s-M4099", "group", 4099, 0, 0, items=4, wg=160)
    add("group-4items-wg160-vit_b-M4099", "group", 4099, 0, 0, items=4, wg=160, vit="b")
    add("group-4items-wg0-onehot-M130", "group", 130, 0, 0, "onehot", items=4)
    ids = [c["id"] for c in g]
    assert len(set(ids)) == len(ids)
    return g


TN_CASES = _tn_grid()
GROUP_SHAPES = block_shapes(VIT_S) + [(72, 200), (200, 8), (136, 136), (8, 72)]     # (N1, N2) of a group's items


def tn_items(c):
    """(N1, N2, accumulate, colsum) of every GEMM of case c."""
    if c["fn"] != "group":
        return [(c["N1"], c["N2"], c["acc"], c["colsum"])]
    sh = block_shapes(VIT_B) if c["vit"] == "b" else GROUP_SHAPES if c["items"] > 4 or c["M"] < 1000 else GROUP_SHAPES[:4]
    return [(n1, n2, i % 2 == 0, i % 3 != 1) for i, (n1, n2) in enumerate(sh[:c["items"]])]


def tn_inputs(c, rows=None):
    """[(A [M, N1], B [M, N2], C_old [N1, N2], colsum_old [N1])] per item, fp64 CPU tensors of exactly representable values."""
    gen = torch.Generator()
    gen.manual_seed(seed_of("tn", c["id"]))
    r16 = rh if c["half"] else rbf
    M = c["M"]
    out = []
    for n1, n2, acc, cs in tn_items(c):
        a, b = operands(c["dist"], M, n1, n2, gen)
        a, b = r16(a).t().contiguous(), r16(b).t().contiguous()
        if rows is not None and rows < M:
            a, b = a[:rows], b[:rows]
        co = torch.randn(n1, n2, generator=gen, dtype=f64).to(f32).double()
        so = torch.randn(n1, generator=gen, dtype=f64).to(f32).double()
        if c["dist"] == "positive":
            co, so = co.abs(), so.abs()
        out.append((a, b, co, so))
    return out


# ------------------------------------------------------------------------------------------------ buffers
GR = 16                 # guard rows past the last row of every buffer (a wave owns 16 rows)


def _bits(t):
    return t.view(torch.int32 if t.element_size() == 4 else torch.int16)


def inp(v, dtype, device, off=8, pad=8):
    """v as a column slice of a wider NaN-filled buffer with GR more rows: the row stride exceeds the logical width, and a read outside
    the slice poisons a checked value.  off / pad: columns in front / behind; the row stride is rounded up to a multiple of 8 elements."""
    if v.dim() == 1:
        return v.to(device=device, dtype=dtype)
    buf = torch.full((v.shape[0] + GR, (off + v.shape[1] + pad + 7) // 8 * 8), float("nan"), device=device, dtype=dtype)
    buf[:v.shape[0], off:off + v.shape[1]] = v.to(device=device, dtype=dtype)
    return buf[:v.shape[0], off:off + v.shape[1]]


class Out:
    """An output [rows, cols] as a column slice of a NaN-filled buffer with guard rows behind it and guard columns on both sides; the
    row stride is padded to a multiple of 8 elements.  arm() records the buffer (after the caller pre-filled what the kernel
    accumulates into); intact() demands everything outside the owned region bit-identical afterwards -- the owned region itself is
    judged by `check`, which refuses a NaN the kernel left standing."""

    def __init__(self, rows, cols, dtype, device, off=8, images=1):
        ld = (off + cols + 8 + 7) // 8 * 8
        self.buf = torch.full((images, rows + GR, ld), float("nan"), device=device, dtype=dtype)
        self.img = self.buf[:, :rows, off:off + cols]
        self.v = self.img[0]
        self.owned = torch.zeros(self.buf.shape, dtype=torch.bool, device=device)
        self.owned[:, :rows, off:off + cols] = True
        self.before = None

    def arm(self):
        self.before = _bits(self.buf).clone()
        return self

    def intact(self, name):
        now = _bits(self.buf)
        bad = (now != self.before) & ~self.owned
        if bool(bad.any()):
            i = bad.nonzero()[0].tolist()
            raise AssertionError(f"{name}: {int(bad.sum())} elements outside the owned region were written, first at [image, row, column] {i} "
                                 f"(owned: rows < {self.img.shape[1]}, columns {int(self.owned[0, 0].nonzero()[0])}..+{self.img.shape[2]})")
