"""lafs_attention_fwd / lafs_attention_bwd (csrc/attention.hip) against a plain fp64 restatement of the same operation on the same
bf16 operands: every tile count 1..16 (all eight dispatch classes and every count strictly inside one), ragged and exact lengths,
mixed lengths in one call, the pair counts that fill a workgroup partly and that make the streaming backward walk several pairs of
different lengths, 1 / 3 / 6 / 11 heads, both softmax scales, strided operands, and six input distributions.

The reference is evaluated in fp64 on the CPU and rounds to bf16 only where the kernels do (un-normalised P in the forward, P and dS
in the backward, the outputs).  Next to every value it carries a bound on how far the kernel's value may lie from it, element by
element (never normalised by a tensor's maximum); a bf16 output's bound is the distance to the neighbouring bf16 values its unrounded
value can reach, 0 where no rounding boundary lies within reach: those outputs must match the reference exactly.  The backward is fed
the kernel's own `out` and `lse` (as the engines do), which the forward check has just bounded, so its reference is what the backward
owes for exactly these operands.  Every output buffer is a column slice of a wider NaN-filled buffer with guard rows past T: the owned
region must be overwritten, everything else must be bit-identical afterwards.

Each case prints the worst |error| / bound over the elements with a non-zero bound and the share of bf16 outputs whose bound is 0."""
import math
import zlib

import pytest
import torch

pytestmark = pytest.mark.gpu

from lafs_cvpr2024_amd import _lib, ops  # noqa: E402
from lafs_cvpr2024_amd.ops import _p  # noqa: E402

DEV = "cuda"
bf16, f32, f64 = torch.bfloat16, torch.float32, torch.float64
U = 2.0 ** -24          # fp32 unit roundoff
R = 2.0 ** -9           # the bf16 rounding of P / dS in front of the second MFMA: half an ulp = 2^-9 of the binade's upper end, top()
TINY = 2.0 ** -120      # a flushed fp32 / bf16 denormal (absolute)
LOG2E = 1.4426950408889634
LN2 = 0.6931471805599453
GR = 16                 # guard rows past T in every buffer (a wave owns 16 rows)
SCALES = {"s64": 64 ** -0.5, "s768": 768 ** -0.5}      # ViT (head_dim^-0.5) and Part-fViT (dim^-0.5)
CHUNK = 3_000_000       # elements of one [batch, heads, L, L] fp64 matrix of the reference


def n_cu():
    return torch.cuda.get_device_properties(0).multi_processor_count     # what the streaming backward sizes its grid by


def _seed(*k):
    return zlib.crc32(repr(k).encode())


# ------------------------------------------------------------------------------------------------ fp64 reference with bounds
def rbf(v):
    return v.to(f32).to(bf16).to(f64)


def flip(v, e):
    """bf16 rounding of a value the kernel holds to within +-e before it rounds: the reference rbf(v) and the most the kernel's bf16
    value can differ from it (rounding is monotone: the kernel's result lies between rbf(v - e) and rbf(v + e))."""
    r = rbf(v)
    return r, torch.maximum(rbf(v + e) - r, r - rbf(v - e))


def f32c(x):
    return float(torch.tensor(x, dtype=f32))


def top(p):
    """The upper end of the binade of p >= 0 (0 for 0): round-to-nearest-even to bf16 moves a value by at most half an ulp, which is
    R top(p) -- between R p and 2 R p.  (R p itself is no bound: 1 + 2^-8 rounds to 1 or 1 + 2^-7, off by 2^-8 (1 - 2^-8) p.)"""
    return torch.exp2(torch.floor(torch.log2(p)) + 1)


def scores(q, k, scale):
    """x = scale log2(e) q k^T (the log2 domain the kernels work in) and a bound on the kernel's fp32 value of it."""
    S, Sa = q @ k.transpose(-1, -2), q.abs() @ k.abs().transpose(-1, -2)
    c = f32c(scale) * LOG2E
    x = S * c
    # fp32 accumulation of 64 exact bf16 products, worst case (all roundings of one sign); c2 = fl(fl(scale) fl(log2 e)) and the
    # product with it: three roundings
    return x, 64 * U * c * Sa + 3 * U * x.abs()


def attn_fwd_ref(q, k, v, scale):
    """q, k, v: fp64 [..., L, 64] of the bf16 operands.  Returns out = bf16(softmax(scale q k^T) v) and lse, each with its bound."""
    L = q.shape[-2]
    x, ex = scores(q, k, scale)
    m = x.max(-1, keepdim=True).values
    a = x - m
    e = torch.exp2(a)
    # exp2 of an argument off by ex (the kernel's own maximum is a factor common to the row: it cancels) and by the rounding of the
    # subtraction; v_exp_f32 itself is good to 1 ulp
    re = torch.expm1(LN2 * (ex + 2 * U * a.abs())) + 2 * U
    s = e.sum(-1, keepdim=True)
    # fp32 sum of <= L + 12 positive terms (the padded tail of the last tile and two shuffles)
    rs = (e * re).sum(-1, keepdim=True) / s + (L + 12) * U
    num, numa = e @ v, e @ v.abs()
    # each e_j off by re_j, then rounded to bf16 (2^-9 sum_j top(p_j) |v_j|), then accumulated in fp32 over the padded keys; flushed
    # denormals
    enum = (e * re + R * top(e * (1 + re))) @ v.abs() + (L + 16) * U * numa + TINY * v.abs().sum(-2, keepdim=True)
    o = num / s
    # the quotient: the sum's error, v_rcp_f32 (1 ulp), the product
    oe = (enum + num.abs() * (rs + 4 * U)) / s * (1 + 2 * rs)
    ob, obe = flip(o, oe)
    lse2 = m + torch.log2(s)
    # log-sum-exp is 1-Lipschitz in the maximum norm of its arguments; the sum's relative error; v_log_f32 (1 ulp of a value <= 8);
    # the addition; the product with fl(ln 2)
    lse2e = ex.max(-1, keepdim=True).values + 2 * U * a.abs().max(-1, keepdim=True).values + 1.01 * rs / LN2 + 16 * U + U * lse2.abs()
    lse = lse2 * LN2
    return ob, obe, lse.squeeze(-1), (LN2 * lse2e + 2 * U * lse.abs()).squeeze(-1)


def attn_bwd_ref(q, k, v, o, lse, do, scale):
    """dq, dk, dv (bf16) from the bf16 operands, the bf16 `o` and fp32 `lse` the forward kernel stored and dO, each with its bound."""
    L = q.shape[-2]
    sc = f32c(scale)
    x, ex = scores(q, k, scale)
    nl = -(lse * LOG2E).unsqueeze(-1)
    arg = x + nl
    p = torch.exp2(arg)
    # exp2(fma(s, c2, -lse log2 e)): the score's error, the rounded constant and product in nl, the fma's rounding; v_exp_f32
    rp = torch.expm1(LN2 * (ex + 2 * U * nl.abs() + U * arg.abs())) + 2 * U
    ep = p * rp
    del x, ex, arg, rp
    delta = (o * do).sum(-1, keepdim=True)
    # 64 exact products summed in fp32: 7 additions in a thread, three shuffles
    ed = 16 * U * (o * do).abs().sum(-1, keepdim=True)
    nd = -sc * delta
    dP = do @ v.transpose(-1, -2)
    # fp32 accumulation of 64 exact products; fma with fl(scale) and the rounded -scale delta
    t = dP * sc + nd
    et = sc * 64 * U * (do.abs() @ v.abs().transpose(-1, -2)) + sc * ed + U * nd.abs() + U * t.abs()
    del dP
    dS = p * t
    eds = ep * t.abs() + (p + ep) * et + U * dS.abs()
    del t, et
    # P and dS rounded to bf16 in front of the MFMAs (half an ulp each); flushed denormals
    eP = ep + R * top(p + ep) + TINY
    eD = eds + R * top(dS.abs() + eds) + TINY
    acc = (L + 16) * U                                        # fp32 accumulation over the padded rows of the other side
    pt, dst = p.transpose(-1, -2), dS.transpose(-1, -2)
    dv, dve = pt @ do, eP.transpose(-1, -2) @ do.abs() + acc * (pt @ do.abs())
    dk, dke = dst @ q, eD.transpose(-1, -2) @ q.abs() + acc * (dst.abs() @ q.abs())
    dq, dqe = dS @ k, eD @ k.abs() + acc * (dS.abs() @ k.abs())
    return flip(dq, dqe) + flip(dk, dke) + flip(dv, dve)


# ------------------------------------------------------------------------------------------------ inputs
def make_inputs(lens, heads, scale, dist, seed):
    """bf16 qkv [T, 3 heads 64] and dout [T, heads 64] on the CPU.
    normal: unit normal everywhere.  peaked: q scaled so that the logits have a standard deviation of about 8 (near one-hot rows).
    offset+: q and k share a component (k's random part is orthogonal to it) that puts +80 nat under every logit.  offset-: the same
    with -120 nat under every logit of the rows i % 3 == 0 and of each sequence's last row.  samekeys: all keys of a (sequence, head)
    identical (rows exactly uniform).  gradlike: dout ~ 1e-3, V rows of scale 0.02 / 1 / 20."""
    g = torch.Generator().manual_seed(seed)
    T = sum(lens)
    rn = lambda *s: torch.randn(*s, generator=g, dtype=f64)
    q, k, v, do = rn(T, heads, 64), rn(T, heads, 64), rn(T, heads, 64), rn(T, heads, 64)
    row = torch.cat([torch.arange(n) for n in lens]) if T else torch.zeros(0, dtype=torch.long)
    last = torch.cat([torch.arange(n) == n - 1 for n in lens]) if T else torch.zeros(0, dtype=torch.bool)
    u = torch.full((64,), 0.125, dtype=f64)                     # unit vector
    if dist == "peaked":
        q = q / scale
    elif dist in ("offset+", "offset-"):
        nat = 80.0 if dist == "offset+" else 120.0
        c = math.sqrt(nat / scale)
        k = k - (k @ u).unsqueeze(-1) * u + c * u
        if dist == "offset+":
            q = q + c * u
        else:
            sel = ((row % 3 == 0) | last).view(T, 1, 1)
            q = torch.where(sel, q - c * u, q)
    elif dist == "samekeys":
        k = k[torch.arange(T) - row]                              # every token takes the key of its sequence's first token
    elif dist == "gradlike":
        do = do * 1e-3
        v = v * torch.tensor([0.02, 1.0, 20.0], dtype=f64)[row % 3].view(T, 1, 1)
    else:
        assert dist == "normal", dist
    qkv = torch.cat([q.reshape(T, -1), k.reshape(T, -1), v.reshape(T, -1)], 1).to(bf16)
    return qkv, do.reshape(T, -1).to(bf16)


# ------------------------------------------------------------------------------------------------ buffers and checks
class Buf:
    """A [rows, cols] view into a NaN-filled buffer with `pad` more columns and GR more rows.  As an input: a read outside the view
    poisons a checked value.  As an output: `untouched` holds the kernel to the rows and columns it owns."""

    def __init__(self, rows, cols, dtype, pad, value=None):
        self.buf = torch.full((rows + GR, cols + pad), float("nan"), device=DEV, dtype=dtype)
        self.v = self.buf[:rows, :cols]
        if value is not None:
            self.v.copy_(value)
        self.before = self.buf.clone()

    def bits(self, t):
        return t.view(torch.int16 if t.element_size() == 2 else torch.int32)

    def untouched(self, name, whole=False):
        rows, cols = self.v.shape
        a, b = self.bits(self.buf), self.bits(self.before)
        if whole:
            assert torch.equal(a, b), f"{name}: written although it must not be"
        assert torch.equal(a[rows:], b[rows:]), f"{name}: rows past T were written"
        assert torch.equal(a[:rows, cols:], b[:rows, cols:]), f"{name}: columns past the logical width were written"


def check(name, got, ref, bound, stats):
    """Element by element: |got - ref| <= bound, exact where bound is 0.  stats collects (worst |error| / bound over the elements with
    a non-zero bound, elements with a zero bound, elements, elements that differ from the reference at all)."""
    got, ref, bound = got.double().reshape(-1, got.shape[-1]), ref.reshape(-1, ref.shape[-1]), bound.reshape(-1, bound.shape[-1])
    assert bool(torch.isfinite(ref).all()) and bool(torch.isfinite(bound).all()), f"{name}: the fp64 reference is not finite"
    fin = torch.isfinite(got)
    if not bool(fin.all()):
        rows = (~fin).any(1).nonzero().flatten()
        raise AssertionError(f"{name}: {int((~fin).sum())} non-finite values in {rows.numel()} rows, first rows {rows[:8].tolist()}")
    err = (got - ref).abs()
    nz = bound > 0
    stats[0] = max(stats[0], float((err[nz] / bound[nz]).max()) if bool(nz.any()) else 0.0)
    stats[1] += int((~nz).sum())
    stats[2] += bound.numel()
    stats[3] += int((err > 0).sum())
    bad = err > bound
    if bool(bad.any()):
        rows = bad.any(1).nonzero().flatten()
        r = int(rows[0])
        c = int(bad[r].nonzero()[0])
        raise AssertionError(f"{name}: {int(bad.sum())} values in {rows.numel()} rows out of bounds (first rows {rows[:8].tolist()}); "
                             f"[{r}, {c}]: kernel {float(got[r, c]):.7g}, fp64 reference {float(ref[r, c]):.7g}, bound {float(bound[r, c]):.3g}, "
                             f"|error| / bound {float(err[r, c] / bound[r, c]) if float(bound[r, c]) > 0 else float('inf'):.3g}")


def groups(lens, heads):
    """Sequences of equal length batched together, in chunks of at most CHUNK score-matrix elements: (length, [sequence indices])."""
    by = {}
    for s, n in enumerate(lens):
        if n > 0:
            by.setdefault(n, []).append(s)
    for n, idx in by.items():
        step = max(1, CHUNK // (heads * n * n))
        for i in range(0, len(idx), step):
            yield n, idx[i:i + step]


def launch_fwd(qkv, cud, n_seq, max_len, heads, scale, out, lse):
    _lib.call("lafs_attention_fwd", _p(qkv), qkv.stride(0), _p(cud), n_seq, max_len, heads, scale, _p(out), out.stride(0), _p(lse))


def launch_bwd(qkv, out, dout, lse, cud, n_seq, max_len, heads, scale, dqkv):
    _lib.call("lafs_attention_bwd", _p(qkv), qkv.stride(0), _p(out), out.stride(0), _p(dout), dout.stride(0), _p(lse), _p(cud), n_seq,
              max_len, heads, scale, _p(dqkv), dqkv.stride(0))


# ------------------------------------------------------------------------------------------------ one case
def run(lens, heads, scale, dist="normal", seed=0, max_len=None, repeat=False):
    """One forward and one backward launch over sequences of the lengths `lens`, every output against the fp64 reference."""
    max_len = max_len or max(lens)
    T, inner, n_seq = sum(lens), heads * 64, len(lens)
    cu = [0]
    for n in lens:
        cu.append(cu[-1] + n)
    qkv_c, do_c = make_inputs(lens, heads, scale, dist, seed)
    cud = torch.tensor(cu, dtype=torch.int32, device=DEV)
    # four strides, all larger than the minimum, all different, all multiples of 8
    qkv = Buf(T, 3 * inner, bf16, 8, qkv_c)
    dout = Buf(T, inner, bf16, 24, do_c)
    out, lse = Buf(T, inner, bf16, 16), Buf(T, heads, f32, 0)
    dqkv = Buf(T, 3 * inner, bf16, 40)
    assert len({qkv.v.stride(0), out.v.stride(0), dout.v.stride(0), dqkv.v.stride(0)}) == 4
    nm = f"[attention] {dist} lens {lens[:4]}{'..x%d' % n_seq if n_seq > 4 else ''} max_len {max_len} heads {heads} scale {scale:.4f}"

    launch_fwd(qkv.v, cud, n_seq, max_len, heads, scale, out.v, lse.v)
    torch.cuda.synchronize()
    out.untouched(f"{nm}: out")
    lse.untouched(f"{nm}: lse")
    out_k, lse_k = out.v.cpu(), lse.v.cpu()
    launch_bwd(qkv.v, out.v, dout.v, lse.v, cud, n_seq, max_len, heads, scale, dqkv.v)
    torch.cuda.synchronize()
    dqkv.untouched(f"{nm}: dqkv")
    qkv.untouched(f"{nm}: qkv", whole=True)
    dout.untouched(f"{nm}: dout", whole=True)
    assert torch.equal(out.v.cpu().view(torch.int16), out_k.view(torch.int16)) and torch.equal(lse.v.cpu(), lse_k), \
        f"{nm}: the backward wrote its inputs out / lse"
    dqkv_k = dqkv.v.cpu()
    if repeat:
        out2, lse2, dqkv2 = Buf(T, inner, bf16, 16), Buf(T, heads, f32, 0), Buf(T, 3 * inner, bf16, 40)
        launch_fwd(qkv.v, cud, n_seq, max_len, heads, scale, out2.v, lse2.v)
        launch_bwd(qkv.v, out2.v, dout.v, lse2.v, cud, n_seq, max_len, heads, scale, dqkv2.v)
        torch.cuda.synchronize()
        for name, a, b in (("out", out, out2), ("lse", lse, lse2), ("dqkv", dqkv, dqkv2)):
            assert torch.equal(a.bits(a.buf), b.bits(b.buf)), f"{nm}: {name} differs between two calls on the same inputs"

    sf, sl, sb = [0.0, 0, 0, 0], [0.0, 0, 0, 0], [0.0, 0, 0, 0]
    head = lambda t, rows, i: t[rows, i * inner:(i + 1) * inner].double().view(len(rows), heads, 64)
    first_error = None
    for n, idx in groups(lens, heads):
        rows = torch.cat([torch.arange(cu[s], cu[s] + n) for s in idx])
        pick = lambda t, i=0: head(t, rows, i).view(len(idx), n, heads, 64).transpose(1, 2)          # [batch, heads, n, 64]
        q, k, v = pick(qkv_c, 0), pick(qkv_c, 1), pick(qkv_c, 2)
        ob, obe, lr, lre = attn_fwd_ref(q, k, v, scale)
        o_k = pick(out_k)
        l_k = lse_k[rows].double().view(len(idx), n, heads).transpose(1, 2)
        dq, dqe, dk, dke, dv, dve = attn_bwd_ref(q, k, v, o_k, l_k, pick(do_c), scale)
        if dist == "samekeys":
            # exactly uniform rows: the reference output is V's column mean (to within the bound just derived)
            # (bf16's unit roundoff for the output's own rounding)
            mean = v.mean(-2, keepdim=True).expand_as(ob)
            assert bool(((o_k - mean).abs() <= obe + mean.abs() * 2.0 ** -8).all()), f"{nm}: out is not V's column mean"
        if dist == "normal" and n >= 16:
            # nowhere may a bound admit more than the max-normalised gates of test_attention_fwd_bwd did (a very short sequence's dq
            # and dk are differences near zero: no maximum to speak of)
            assert float(obe.max()) <= 1.5e-2 * float(ob.abs().max()), f"{nm}: forward bound looser than 1.5e-2 of the maximum"
            for name, r, e in (("dq", dq, dqe), ("dk", dk, dke), ("dv", dv, dve)):
                assert float(e.max()) <= 3e-2 * float(r.abs().max()), f"{nm}: {name} bound looser than 3e-2 of the maximum"
        try:
            check(f"{nm}: out (length {n})", o_k, ob, obe, sf)
            check(f"{nm}: lse (length {n})", l_k.unsqueeze(-1), lr.unsqueeze(-1), lre.unsqueeze(-1), sl)
            for i, (name, r, e) in enumerate((("dq", dq, dqe), ("dk", dk, dke), ("dv", dv, dve))):
                check(f"{nm}: {name} (length {n})", pick(dqkv_k, i), r, e, sb)
        except AssertionError as err:                          # (every group is measured before the first failure is raised)
            first_error = first_error or err
    sh = lambda s, i=1: 100.0 * s[i] / max(s[2], 1)
    print(f"{nm}: |error| / bound  out {sf[0]:.3f}  lse {sl[0]:.3f}  dqkv {sb[0]:.3f};  bound 0 (must be exact)  out {sh(sf):.1f} %  dqkv {sh(sb):.1f} %;"
          f"  off by a bf16 step  out {sh(sf, 3):.1f} %  dqkv {sh(sb, 3):.1f} %"
          + ("  FAILED" if first_error else ""))
    if first_error:
        raise first_error
    return sf, sl, sb


# ------------------------------------------------------------------------------------------------ the grids
HEADS = [1, 3, 6, 11]
# a ragged length in every tile count 1..16 (1, 15 / 17 next to the first boundary), three sequences per call
RAGGED = {1: 15, 2: 17, 3: 37, 4: 49, 5: 77, 6: 83, 7: 100, 8: 127, 9: 130, 10: 150, 11: 161, 12: 190, 13: 197, 14: 215, 15: 239, 16: 250}


@pytest.mark.parametrize("kind", ["ragged", "exact"])
@pytest.mark.parametrize("nt", list(range(1, 17)), ids=[f"nt{t}" for t in range(1, 17)])
def test_every_tile_count(nt, kind):
    """max_len of every tile count: all eight instantiations of both directions, and every count strictly inside a dispatch class
    (whole trailing tiles are padding for every sequence).  `exact` takes the forward's wave-uniform unmasked branch in every tile.
    Three sequences: 3 x heads pairs, not a multiple of the 4 / 2 pairs a workgroup takes for most head counts."""
    n = RAGGED[nt] if kind == "ragged" else 16 * nt
    heads = HEADS[(nt + (kind == "exact")) % 4]
    scale = list(SCALES.values())[(nt // 2) % 2]
    run([n] * 3, heads, scale, seed=_seed("t", nt, kind))


MIXED = {
    "nt1": ([1, 16, 0, 9, 15, 1], 3), "nt2": ([17, 1, 32, 0, 5, 30], 11), "nt3": ([37, 1, 0, 20, 16, 37, 3], 6), "nt4": ([64, 0, 1, 17, 48, 63], 1),
    "nt7": ([100, 0, 77, 1, 30, 97, 112], 3), "nt10": ([160, 3, 0, 100, 1, 150, 145], 6), "nt13": ([197, 5, 0, 150, 1, 37, 197], 3),
    "nt16": ([256, 200, 0, 1, 130, 33, 255], 1),
}


@pytest.mark.parametrize("case", list(MIXED))
def test_mixed_lengths_in_one_call(case):
    """Sequences shorter than a wave item's first tile (the item is skipped), a single-token sequence and an empty sequence between
    two others (it owns no row: nothing written, nothing disturbed), in every dispatch class."""
    lens, heads = MIXED[case]
    run(lens, heads, SCALES["s64"] if heads != 11 else SCALES["s768"], seed=_seed("x", case))


@pytest.mark.parametrize("length", [1, 16, 17, 64, 100, 197, 256])
def test_a_single_pair(length):
    run([length], 1, SCALES["s64"], seed=_seed("1", length))


STREAM = {"nt13": [197, 150, 5, 37, 180], "nt10": [160, 100, 3, 150, 20]}


@pytest.mark.parametrize("pairs", ["ncu+1", "2ncu+3"])
@pytest.mark.parametrize("cls", list(STREAM))
def test_streaming_backward_walks_pairs_of_different_lengths(cls, pairs):
    """The 10- and 13-tile classes run one workgroup per CU that walks the pairs b, b + grid, ...: with n_cu + 1 and 2 n_cu + 3 pairs
    of interleaved long and short sequences every workgroup that takes a second (third) pair stages it into the Q | dO buffer that
    just held another length: rows >= len of a buffer must be re-zeroed by every deposit."""
    n = n_cu() + 1 if pairs == "ncu+1" else 2 * n_cu() + 3
    period = next(p for p in (3, 4, 5) if n_cu() % p)         # one head: pair b + n_cu has another length than pair b
    pat = STREAM[cls][:period]
    run([pat[i % period] for i in range(n)], 1, SCALES["s64"], seed=_seed("s", cls, pairs), max_len=max(pat))


SHAPES = {"stream13": ([197, 150, 37, 197, 5], 3), "short3": ([37, 20, 1, 33, 37], 6), "long16": ([250, 129, 256], 1)}
DISTS = ["normal", "peaked", "offset+", "offset-", "samekeys", "gradlike"]
# each distribution in each backward form (fused short, streaming, fused long), the offsets at both scales
DIST_CASES = [(d, sh, "s768" if sh == "long16" else "s64") for d in DISTS for sh in SHAPES] + \
             [(d, sh, "s768") for d in ("offset+", "offset-") for sh in ("stream13", "short3")]


@pytest.mark.parametrize("dist,shape,scale", DIST_CASES, ids=["-".join(c) for c in DIST_CASES])
def test_input_distributions(dist, shape, scale):
    """Near one-hot rows, a large common logit offset of either sign (the maximum subtraction and the backward's exp2(s c2 - lse log2 e)
    at |lse| ~ 100; offset-: a padded key of a ragged last tile has score 0 = e^120 times the row's largest weight, which must not
    reach dQ), exactly uniform rows, gradient-like dout with V of mixed scale -- in each backward form."""
    lens, heads = SHAPES[shape]
    run(lens, heads, SCALES[scale], dist=dist, seed=_seed("d", dist, shape, scale))


@pytest.mark.parametrize("form", ["short3", "long7", "stream13", "long16"])
def test_two_calls_give_identical_bits(form):
    """Run-to-run reproducibility of out, lse and dqkv (guard regions included) in each kernel form."""
    lens, heads = {"short3": ([37, 20, 37, 1, 33], 3), "long7": ([100, 77, 97], 3), "stream13": ([197, 150, 5] * 30, 3),
                   "long16": ([256, 200, 250], 6)}[form]
    run(lens, heads, SCALES["s64"], seed=_seed("r", form), repeat=True)


# ------------------------------------------------------------------------------------------------ the accepted domain
def test_invalid_arguments_fail_loudly_and_launch_nothing():
    lens, heads, inner = [37, 20], 2, 128
    T = sum(lens)
    qkv = torch.zeros(T, 3 * inner + 8, device=DEV, dtype=bf16)
    dout = torch.zeros(T, inner + 8, device=DEV, dtype=bf16)
    cud = torch.tensor([0, 37, 57], dtype=torch.int32, device=DEV)
    nan = float("nan")
    out, lse = torch.full((T, inner + 8), nan, device=DEV, dtype=bf16), torch.full((T, heads), nan, device=DEV)
    dqkv = torch.full((T, 3 * inner + 8), nan, device=DEV, dtype=bf16)

    def fwd(**kw):
        a = dict(qkv=_p(qkv), ldqkv=3 * inner + 8, cu=_p(cud), n_seq=2, max_len=37, heads=heads, out=_p(out), ldo=inner + 8, lse=_p(lse))
        a.update(kw)
        _lib.call("lafs_attention_fwd", a["qkv"], a["ldqkv"], a["cu"], a["n_seq"], a["max_len"], a["heads"], 0.125, a["out"], a["ldo"], a["lse"])

    def bwd(**kw):
        a = dict(qkv=_p(qkv), ldqkv=3 * inner + 8, out=_p(out), ldo=inner + 8, dout=_p(dout), lddo=inner + 8, lse=_p(lse), cu=_p(cud), n_seq=2,
                 max_len=37, heads=heads, dqkv=_p(dqkv), lddqkv=3 * inner + 8)
        a.update(kw)
        _lib.call("lafs_attention_bwd", a["qkv"], a["ldqkv"], a["out"], a["ldo"], a["dout"], a["lddo"], a["lse"], a["cu"], a["n_seq"],
                  a["max_len"], a["heads"], 0.125, a["dqkv"], a["lddqkv"])

    torch.cuda.synchronize()
    for name in ("qkv", "cu", "out", "lse"):
        with pytest.raises(_lib.LafsHipError, match="null operand"):
            fwd(**{name: None})
    for name in ("qkv", "out", "dout", "lse", "cu", "dqkv"):
        with pytest.raises(_lib.LafsHipError, match="null operand"):
            bwd(**{name: None})
    for f in (fwd, bwd):
        for kw in (dict(max_len=0), dict(max_len=257), dict(heads=0), dict(n_seq=0)):
            with pytest.raises(_lib.LafsHipError, match="1..256"):
                f(**kw)
    for f, names in ((fwd, ("ldqkv", "ldo")), (bwd, ("ldqkv", "ldo", "lddo", "lddqkv"))):
        for name in names:
            with pytest.raises(_lib.LafsHipError, match="multiples of 8"):
                f(**{name: (3 * inner if "qkv" in name else inner) + 4})
    torch.cuda.synchronize()
    for name, t in (("out", out), ("lse", lse), ("dqkv", dqkv)):
        assert bool(torch.isnan(t).all()), f"{name} written by a rejected call"
    # the same arguments with nothing wrong run (the cases above fail for the one reason each names): all-zero operands give
    # uniform rows, zero outputs, lse = log(len) and zero gradients
    fwd()
    bwd()
    torch.cuda.synchronize()
    assert bool((out[:, :inner] == 0).all()) and bool(torch.isnan(out[:, inner:].float()).all())
    assert torch.allclose(lse[:37], torch.full((37, heads), math.log(37.0), device=DEV), atol=1e-5)
    assert bool((dqkv[:, :3 * inner] == 0).all()) and bool(torch.isnan(dqkv[:, 3 * inner:].float()).all())
