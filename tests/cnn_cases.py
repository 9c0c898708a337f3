"""The case grids of tests/test_gpu_cnn_kernels.py (the landmark CNN's kernels, csrc/landmark_cnn.hip and csrc/landmark_train.hip, plus
lafs_landmark_theta of csrc/finetune.hip), their seeded inputs and one fp64 restatement per entry point that returns, per output,
(reference, bound, 16-bit output?) in the style of tests/fp64_bounds.py.  Kept apart from the GPU module so that
tests/test_oracle_cnn_host.py judges on the CPU exactly the cases the GPU runs.

Every input value is exactly representable in the format the kernel reads it in (bf16 activations on the inference plan, fp16 on the
training plan, fp32 weights and statistics).  The references round to 16 bits exactly where the kernel stores 16 bits (fb.flip with
fb.rbf / fb.rh), so most 16-bit outputs must match bit for bit.  The reach before the rounding is the kernel's own operation count:
  * a k x k depthwise window or the 27-tap stem is a chain of K fmas that starts from the bias: fb.acc_factor(K, worst) u (sum |x w| +
    |b|), plus K u |b| for the bias the chain starts from (as fb.gemm);
  * a pooling / statistics / gate-gradient sum is a per-thread sequence followed by a binary tree over the lanes: fb.tree_depth
    additions per term, depth u sum |terms| whatever the signs are;
  * a product of two 16-bit values is exact in fp32 (16 resp. 22 significant bits), so the squeeze-excite rescale and its backward
    recompute their pre-activation z gate exactly: no element of those kernels is on a knife edge of act', and the side taken AT a
    kink is the source's (z <= -3 -> 0, z >= 3 -> 1, relu' (0) = 0, h-sigmoid' (+-3) = 0), which the `kink` cases assert;
  * the activations and their derivatives are fb.act / fb.act_grad.
Bounds that turned out too tight on the device would be corrected here, with the reason; none has been."""
import math

import torch

import fp64_bounds as fb
from fp64_bounds import U, f32, f64, rbf, rh
from gemm_cases import seed_of

DISTS = ("normal", "offset", "positive")


def _gen(*key):
    g = torch.Generator()
    g.manual_seed(seed_of("cnn", *key))
    return g


def _rn(gen, *s):
    return torch.randn(*s, generator=gen, dtype=f64)


def r32(v):
    return v.to(f32).double()


def _ids(cases):
    ids = [c["id"] for c in cases]
    assert len(set(ids)) == len(ids), "duplicate case ids"
    return cases


def group_block(ld):
    """group_block of landmark_train.hip: channel groups (of 8) per workgroup."""
    g = ld // 8
    return 4 if g <= 4 else 8 if g <= 8 else 16 if g <= 16 else 32


def rows_per_block(R):
    return (max(256, -(-R // 1024)) + 63) // 64 * 64


def coded_image(N, S):
    """value = (((n 3 + c) S + y) S + x + 1) / 64: a wrong tap shows as another pixel's code (exact in fp32 and, up to 2048 codes, in
    fp16)."""
    return (torch.arange(N * 3 * S * S, dtype=f64) + 1).view(N, 3, S, S) / 64


# ================================================================================================ inference plan (bf16 NHWC)
# ------------------------------------------------------------------------------------------------ lafs_cnn_stem
STEM_PLANES = [(1, 2), (2, 6), (3, 20)]          # 3 x 10 x 10 = 300 outputs: a second, partly filled workgroup


def _stem_grid():
    g = []
    for i, (N, S) in enumerate(STEM_PLANES):
        for act in (0, 1, 2):
            g.append(dict(id=f"stem-{N}x{S}-ldy{(16, 24, 32)[(i + act) % 3]}-act{act}", N=N, S=S, ldy=(16, 24, 32)[(i + act) % 3], act=act, coded=False))
        g.append(dict(id=f"stem-{N}x{S}-ldy{(32, 16, 24)[i]}-coded", N=N, S=S, ldy=(32, 16, 24)[i], act=0, coded=True))
    return _ids(g)


STEM_CASES = _stem_grid()


def stem_inputs(c):
    gen = _gen(c["id"])
    x = coded_image(c["N"], c["S"]) if c["coded"] else r32(_rn(gen, c["N"], 3, c["S"], c["S"]))
    return dict(x=x, w=r32(0.3 * _rn(gen, 27, 16)), b=r32(0.5 * _rn(gen, 16)))


def stem_conv(d):
    """The 3 x 3 stride-2 pad-1 convolution 3 -> 16 channels of the stem as (value, sum |terms|) [N, So, So, 16]; w [27, 16] holds tap
    (c, ky, kx) of output channel o at [c 9 + ky 3 + kx, o]."""
    x, w = d["x"], d["w"]
    N, _, S, _ = x.shape
    So = S // 2
    xp = torch.zeros(N, 3, S + 2, S + 2, dtype=f64)
    xp[:, :, 1:S + 1, 1:S + 1] = x
    v = torch.zeros(N, So, So, 16, dtype=f64)
    s = torch.zeros_like(v)
    for ch in range(3):
        for ky in range(3):
            for kx in range(3):
                t = xp[:, ch, ky:ky + 2 * (So - 1) + 1:2, kx:kx + 2 * (So - 1) + 1:2][..., None] * w[ch * 9 + ky * 3 + kx]
                v, s = v + t, s + t.abs()
    return v, s


def stem_expected(c, d, r16=rbf):
    v, s = stem_conv(d)
    b = d["b"]
    v, s = v + b, s + b.abs()
    e = fb.acc_factor(27, c["coded"]) * U * s + 27 * U * b.abs()
    y, ye = fb.flip(*fb.act(v, e, c["act"]), r16)
    pad = torch.zeros(*v.shape[:3], c["ldy"] - 16, dtype=f64)
    return {"y": (torch.cat([y, pad], 3), torch.cat([ye, pad], 3), True), "mag": s}


# ------------------------------------------------------------------------------------------------ depthwise convolutions (both plans)
DW_PLANES = [(1, 1), (2, 3), (4, 4), (7, 7), (5, 8), (9, 6)]      # smaller than the kernel, odd with stride 2, non-square


def _dw_grid():
    g, i = [], 0
    for k in (3, 5):
        for stride in (1, 2):
            for H, W in DW_PLANES:
                C, N, act = (8, 24, 40)[i % 3], (1, 3)[(i // 3) % 2], (-1, 0, 1, 2)[i % 4]
                g.append(dict(id=f"dw-k{k}s{stride}-{H}x{W}-C{C}-N{N}-act{act}", k=k, stride=stride, H=H, W=W, C=C, N=N, act=act, dist="normal"))
                i += 1
    g.append(dict(id="dw-k3s1-7x7-C40-N3-positive", k=3, stride=1, H=7, W=7, C=40, N=3, act=2, dist="positive"))     # 735 threads: 3 workgroups
    g.append(dict(id="dw-k5s2-9x6-C24-N3-positive", k=5, stride=2, H=9, W=6, C=24, N=3, act=1, dist="positive"))
    return _ids(g)


DW_CASES = _dw_grid()


def dw_inputs(c):
    gen = _gen(c["id"])
    x = _rn(gen, c["N"], c["H"], c["W"], c["C"])
    w = 0.4 * _rn(gen, c["k"] ** 2, c["C"])
    if c["dist"] == "positive":
        x, w = x.abs(), w.abs()
    return dict(x=rbf(x), w=r32(w), b=r32(0.5 * _rn(gen, c["C"])))


def dw_expected(c, d):
    K = c["k"] ** 2
    v, s = fb.dwconv(d["x"], d["w"], c["k"], c["stride"])
    b = d["b"]
    v, s = v + b, s + b.abs()
    e = fb.acc_factor(K, c["dist"] == "positive") * U * s + K * U * b.abs()
    return {"y": fb.flip(*fb.act(v, e, max(c["act"], 0)), rbf) + (True,), "mag": s}


# ------------------------------------------------------------------------------------------------ lafs_cnn_pool
def _pool_grid():
    g = []
    for HW in (1, 15, 16, 17, 49, 196):          # 1, 15: one thread per (image, 8 channels);  16..: one workgroup per image
        for C in (8, 24, 96, 2048):              # C / 8 = 3: 85 pixel rows and one idle thread;  C / 8 = 256: a single pixel row
            g.append(dict(id=f"pool-HW{HW}-C{C}", HW=HW, C=C, N=2 if C == 2048 else 3, ldo=C + 8 * (HW % 2), dist=DISTS[(HW + C // 8) % 3]))
    g.append(dict(id="pool-HW16-C2056-back-on-the-thread-kernel", HW=16, C=2056, N=2, ldo=2064, dist="normal"))
    return _ids(g)


POOL_CASES = _pool_grid()


def pool_route(c):
    return "wg" if c["C"] // 8 <= 256 and c["HW"] >= 16 else "thread"


def _dist(gen, dist, *shape, shift=0.0):
    """normal: randn (+ shift);  offset: |mean| = 30 std;  positive: |randn|.  The pooling cases shift their `normal` inputs by 0.5: the
    mean of 196 zero-mean values is ~0.07 of their magnitude, so the sum's allowance (depth u mean|x|) is a larger share of the
    16-bit step at the MEAN and 2.2 % of the outputs of one case carried a bound of two steps, above the 2 % cap."""
    v = _rn(gen, *shape)
    return 30 + v if dist == "offset" else v.abs() if dist == "positive" else v + shift


def pool_inputs(c):
    return dict(x=rbf(_dist(_gen(c["id"]), c["dist"], c["N"], c["HW"], c["C"], shift=0.5)))


def pool_expected(c, d):
    HW = c["HW"]
    parts = 256 // (c["C"] // 8)
    # (the LDS partials are added in sequence; those of pixel rows past HW are exact zeros, which add without a rounding)
    depth = HW if pool_route(c) == "thread" else -(-HW // parts) + min(parts, HW)
    return {"out": fb.col_mean(d["x"], depth, rbf) + (True,)}


# ------------------------------------------------------------------------------------------------ lafs_cnn_scale_act (in place)
def _scale_act_grid(tag):
    g = []
    for act in (0, 1, 2, 3):
        g.append(dict(id=f"{tag}-1x3x24-act{act}", N=1, HW=3, C=24, act=act, lds=24 + 8 * (act % 2)))             # 9 threads
        g.append(dict(id=f"{tag}-3x49x40-act{act}", N=3, HW=49, C=40, act=act, lds=40 + 8 * ((act + 1) % 2)))    # 735 threads: 3 workgroups
    return _ids(g)


SCALE_ACT_CASES = _scale_act_grid("scale_act")


def scale_inputs(c, r16=rbf):
    """x spread over the kinks of the activations (std 3), gates in (0, 1) as a h-sigmoid leaves them."""
    gen = _gen(c["id"])
    return dict(x=r16(3 * _rn(gen, c["N"], c["HW"], c["C"])), s=r16(torch.rand(c["N"], c["C"], generator=gen, dtype=f64)))


def scale_expected(c, d, r16=rbf):
    p = d["x"] * d["s"][:, None]                          # exact in fp32
    return {"y": fb.flip(*fb.act(p, torch.zeros_like(p), c["act"]), r16) + (True,)}


# ================================================================================================ training plan (fp16 NHWC)
IM2COL_CASES = _ids([dict(id=f"im2col-{N}x{S}-{'coded' if coded else 'random'}", N=N, S=S, coded=coded) for N, S in STEM_PLANES for coded in (False, True)])


def im2col_inputs(c):
    return dict(x=coded_image(c["N"], c["S"]) if c["coded"] else r32(_rn(_gen(c["id"]), c["N"], 3, c["S"], c["S"])))


def im2col_expected(c, d):
    """Rows (n, oy, ox), columns (c, ky, kx) of the 3 x 3 stride-2 pad-1 window, 27..31 zero: values moved and rounded once -- exact."""
    x = d["x"]
    N, _, S, _ = x.shape
    So = S // 2
    xp = torch.zeros(N, 3, S + 2, S + 2, dtype=f64)
    xp[:, :, 1:S + 1, 1:S + 1] = x
    P = torch.zeros(N, So, So, 32, dtype=f64)
    for ch in range(3):
        for ky in range(3):
            for kx in range(3):
                P[..., ch * 9 + ky * 3 + kx] = xp[:, ch, ky:ky + 2 * (So - 1) + 1:2, kx:kx + 2 * (So - 1) + 1:2]
    return {"P": (rh(P).view(-1, 32), torch.zeros(N * So * So, 32, dtype=f64), True)}


# ------------------------------------------------------------------------------------------------ lafs_cnn_bn_stats
BN_SHAPES = [(8, 8), (16, 16), (20, 32), (40, 40), (72, 72), (136, 136), (264, 264)]      # every group_block, idle groups, C % 8 != 0, grid.y = 2


def _stats_grid():
    g, i = [], 0
    for R in (1, 3, 255, 256, 257, 1000):        # with 64, 32, 16 and 8 row lanes these leave 0, 1, 2 and 3 rows to the tail loop
        for C, ld in BN_SHAPES:
            g.append(dict(id=f"stats-R{R}-C{C}-ld{ld}-{DISTS[i % 3]}", R=R, C=C, ld=ld, dist=DISTS[i % 3]))
            i += 1
    g.append(dict(id="stats-R263169-C8-ld8-rows_per_block-320", R=263169, C=8, ld=8, dist="offset"))
    return _ids(g)


STATS_CASES = _stats_grid()


def stats_inputs(c):
    gen = _gen(c["id"])
    x = torch.zeros(c["R"], c["ld"], dtype=f64)
    x[:, :c["C"]] = rh(_dist(gen, c["dist"], c["R"], c["C"]))
    return dict(x=x, old=10 * _rn(gen, 2 * c["C"]))


def stats_expected(c, d):
    """sums[c] += sum x, sums[C + c] += sum x^2 in fp64: per workgroup an fp32 partial (a lane's rows in sequence -- x^2 is exact and
    enters by fma, one rounding per addition --, then the tree over the lanes), one fp64 atomic per workgroup."""
    R, C = c["R"], c["C"]
    x = d["x"][:, :C]
    rpb = rows_per_block(R)
    nblk = -(-R // rpb)
    depth = fb.tree_depth(min(R, rpb), 256 // group_block(c["ld"]))
    s = torch.cat([x.abs().sum(0), (x * x).sum(0)])
    ref = d["old"] + torch.cat([x.sum(0), (x * x).sum(0)])
    return {"sums": (ref, depth * U * s + (nblk + 1) * 2.0 ** -52 * (s + d["old"].abs()), False), "mag": s + d["old"].abs()}


# ------------------------------------------------------------------------------------------------ pooling, squeeze-excite (training plan)
def _se_grid(tag):
    g, i = [], 0
    for HW in (1, 3, 49, 196):                   # against 256 / GB = 64, 32, 16, 8 lanes: fewer pixels than lanes, and several trips
        for ld in (8, 24, 72, 136, 264):
            g.append(dict(id=f"{tag}-HW{HW}-ld{ld}-act{i % 3}", HW=HW, ld=ld, N=3 if HW < 49 else 2, act=i % 3, wide=8 * (1 + i % 2), dist=DISTS[i % 3]))
            i += 1
    return _ids(g)


POOL_TRAIN_CASES = _se_grid("pool_train")
SE_CASES = _se_grid("se")


def pool_train_inputs(c):
    gen = _gen(c["id"])
    return dict(x=rh(_dist(gen, c["dist"], c["N"], c["HW"], c["ld"], shift=0.5)), dfeat=rh(_rn(gen, c["N"], c["ld"])))


def pool_train_expected(c, d):
    HW = c["HW"]
    g = d["dfeat"] / HW                              # the rounded reciprocal and the product: 2 u
    dx = fb.flip(g, 2 * U * g.abs(), rh)
    return {"out": fb.col_mean(d["x"], fb.tree_depth(HW, 256 // group_block(c["ld"])), rh) + (True,),
            "dx": (dx[0][:, None].expand(-1, HW, -1), dx[1][:, None].expand(-1, HW, -1), True)}


def se_inputs(c, kink=False):
    gen = _gen(c["id"], kink)
    N, HW, ld = c["N"], c["HW"], c["ld"]
    z, gate = rh(3 * _rn(gen, N, HW, ld)), rh(torch.rand(N, ld, generator=gen, dtype=f64))
    if kink:                                     # z gate exactly on -3, 0, 3 (gate a power of two)
        gate = torch.full((N, ld), 0.5, dtype=f64)
        z = torch.tensor([-6.0, 0.0, 6.0, 1.0], dtype=f64)[torch.arange(N * HW * ld) % 4].view(N, HW, ld)
    return dict(z=z, gate=gate, dout=rh(_rn(gen, N, HW, ld)))


def se_expected(c, d):
    """out = act(z gate);  ds = dout act'(z gate), dz = ds gate (fp16), dgate[n, c] = sum_p ds z (fp32).  z gate is exact."""
    z, g, do = d["z"], d["gate"][:, None], d["dout"]
    HW = c["HW"]
    p = z * g
    a, ae, knife = fb.act_grad(p, torch.zeros_like(p), c["act"])
    ds = do * a
    dse = do.abs() * ae + (U * ds.abs() if c["act"] == 2 else 0)
    dz = ds * g
    t = ds * z
    depth = fb.tree_depth(HW, 256 // group_block(c["ld"]))
    return {"out": fb.flip(*fb.act(p, torch.zeros_like(p), c["act"]), rh) + (True,),
            "dz": fb.flip(dz, dse * g.abs() + U * dz.abs(), rh) + (True,),
            "dgate": (t.sum(1), (dse * z.abs()).sum(1) + depth * U * t.abs().sum(1), False), "mag": t.abs().sum(1), "knife": int(knife.sum())}


# ------------------------------------------------------------------------------------------------ lafs_cnn_act_bwd_post
ACT_POST_CASES = _ids([dict(id=f"act_post-act{act}-{'f32' if f else 'f16-in-place'}", act=act, f32=f, n=1000) for act in (0, 1, 3) for f in (True, False)])


def act_post_inputs(c):
    gen = _gen(c["id"])
    n = c["n"]
    y = rh(torch.rand(n, generator=gen, dtype=f64) * 1.5 - 0.25).clamp(0, 1)      # a fifth each exactly 0 and exactly 1
    y[-1], y[-2] = 0.0, 1.0
    dy = _rn(gen, n)
    return dict(y=y, dy=r32(dy) if c["f32"] else rh(dy))


def act_post_expected(c, d):
    """dy act'(.) from the post-activation value: relu y > 0; h-sigmoid 0 < y < 1 -> the rounded 1 / 6 (u) times dy (u); else 0."""
    y, dy = d["y"], d["dy"]
    if c["act"] == 0:
        v, e = dy, torch.zeros_like(dy)
    elif c["act"] == 1:
        v, e = dy * (y > 0), torch.zeros_like(dy)
    else:
        v = dy * ((y > 0) & (y < 1)) / 6
        e = 2 * U * v.abs()
    return {"out": fb.flip(v, e, rh) + (True,)}


# ------------------------------------------------------------------------------------------------ casts
CAST_CASES = _ids([dict(id=f"cast-{r}x{cl}-ld{ld}-scale-{s}", rows=r, cols=cl, ld=ld, scale=s)
                   for r, cl, ld in ((5, 7, 8), (3, 136, 136), (37, 20, 32)) for s in (None, 64.0, 1.7)])


def cast_inputs(c):
    return dict(src=r32(_rn(_gen(c["id"]), c["rows"], c["cols"])))


def cast_expected(c, d):
    s = 1.0 if c["scale"] is None else fb.f32c(c["scale"])
    v = torch.zeros(c["rows"], c["ld"], dtype=f64)
    v[:, :c["cols"]] = d["src"] * s
    e = U * v.abs() if c["scale"] == 1.7 else torch.zeros_like(v)          # (a power of two scales exactly)
    return {"dst": fb.flip(v, e, rh) + (True,)}


# ------------------------------------------------------------------------------------------------ depthwise convolution, training plan
def _dwt_grid():
    g, i = [], 0
    shapes = [(8, 8), (24, 32), (20, 32)]
    for k in (3, 5):
        for stride in (1, 2):
            for H, W in DW_PLANES:
                C, ld = shapes[i % 3]
                g.append(dict(id=f"dwt-k{k}s{stride}-{H}x{W}-C{C}-ld{ld}-N{(1, 3)[(i // 3) % 2]}", k=k, stride=stride, H=H, W=W, C=C, ld=ld, N=(1, 3)[(i // 3) % 2],
                              dist="normal", onehot=False))
                i += 1
    # N Ho Wo = 2548 / 2600: three slabs of pix_per_block = 1024
    g.append(dict(id="dwt-k3s1-7x7-C20-ld32-N52-three-slabs", k=3, stride=1, H=7, W=7, C=20, ld=32, N=52, dist="normal", onehot=False))
    g.append(dict(id="dwt-k5s2-9x6-C24-ld32-N174-three-slabs-positive", k=5, stride=2, H=9, W=6, C=24, ld=32, N=174, dist="positive", onehot=False))
    for k, stride, H, W in ((3, 1, 7, 7), (5, 2, 9, 6), (5, 1, 5, 8), (3, 2, 7, 7)):
        g.append(dict(id=f"dwt-k{k}s{stride}-{H}x{W}-onehot", k=k, stride=stride, H=H, W=W, C=20, ld=32, N=2, dist="normal", onehot=True))
    return _ids(g)


DWT_CASES = _dwt_grid()


def dwt_inputs(c):
    gen = _gen(c["id"])
    N, H, W, C, ld, K = c["N"], c["H"], c["W"], c["C"], c["ld"], c["k"] ** 2
    Ho, Wo = -(-H // c["stride"]), -(-W // c["stride"])
    pad = lambda v: torch.cat([v, torch.zeros(*v.shape[:-1], ld - C, dtype=f64)], -1)
    x, dy, w = _rn(gen, N, H, W, C), _rn(gen, N, Ho, Wo, C), 0.4 * _rn(gen, K, C)
    if c["dist"] == "positive":
        x, dy, w = x.abs(), dy.abs(), w.abs()
    if c["onehot"]:
        # a single 1 per channel at a coded position (channel ch: image ch % N, pixel (3 ch) % (Ho Wo)); x holds pixel codes
        dy = torch.zeros(N, Ho * Wo, C, dtype=f64)
        ch = torch.arange(C)
        dy[ch % N, (3 * ch) % (Ho * Wo), ch] = 1.0
        dy = dy.view(N, Ho, Wo, C)
        x = ((torch.arange(N * H * W, dtype=f64) + 1).view(N, H, W, 1) + torch.arange(C, dtype=f64) / 8) / 4
    return dict(x=pad(rh(x)), dy=pad(rh(dy)), w=pad(r32(w)), dw_old=pad(r32(_rn(gen, K, C))))


def dwt_expected(c, d):
    """y, dx fp16: chains of <= k k fmas without a bias.  dw [k k, ld] fp32 accumulates: a thread adds its pixels of a slab in
    sequence (ceil(pix_per_block / 256) fmas of exact products), a 64-lane butterfly (6), the four waves (3), then one fp32 atomic per
    slab on top of the old value."""
    k, stride, C, K = c["k"], c["stride"], c["C"], c["k"] ** 2
    worst = c["dist"] == "positive"
    f = fb.acc_factor(K, worst) * U
    v, s = fb.dwconv(d["x"], d["w"], k, stride)
    (dx, dxs), (dw, dws) = fb.dwconv_bwd(d["x"], d["dy"], d["w"], k, stride)
    npix = d["dy"].shape[0] * d["dy"].shape[1] * d["dy"].shape[2]
    ppb = max(1024, -(-npix // 256))
    nslab = -(-npix // ppb)
    depth = -(-min(npix, ppb) // 256) + 6 + 3 + nslab
    old = d["dw_old"]
    return {"y": fb.flip(v, f * s, rh) + (True,), "dx": fb.flip(dx, f * dxs, rh) + (True,),
            "dw": (old + dw, depth * U * (dws + old.abs()), False), "mag_dw": dws + old.abs()}


# ------------------------------------------------------------------------------------------------ lafs_landmark_theta (+ backward)
def _theta_grid():
    g = []
    for B in (1, 3):
        for n_full in (2, 36, 196, 300):         # 2 n_full across 256 and 512
            g.append(dict(id=f"theta-B{B}-n{n_full}-plain", B=B, n_full=n_full, noise=False, sel=False, n_out=n_full))
            g.append(dict(id=f"theta-B{B}-n{n_full}-noise-sel", B=B, n_full=n_full, noise=True, sel=True, n_out=(3, 36, 36, 301)[(2, 36, 196, 300).index(n_full)]))
    return _ids(g)


THETA_CASES = _theta_grid()
THETA_BWD_KINDS = ("random", "twice", "ends", "ends-swapped", "same-lane")


def theta_inputs(c):
    gen = _gen(c["id"])
    B, n = c["B"], c["n_full"]
    d = dict(t=r32(_rn(gen, B, 2 * n)), noise=r32(_rn(gen, B, 2 * n)), dtheta=r32(_rn(gen, B, 2 * n)))
    d["sel"] = torch.randint(0, n, (B, c["n_out"]), generator=gen).int()
    d["sel"][:, -1] = d["sel"][:, 0]              # a repeat
    return d


def theta_structured(c, kind):
    """The raw landmarks of case c with the extrema placed: `twice` -- the minimum and the maximum occur twice each (the first
    occurrence takes the gradient, as torch.min / torch.max select); `ends` -- arg-min at 0, arg-max at n - 1 (and swapped);
    `same-lane` -- both extrema in one 256-stride lane."""
    d = theta_inputs(c)
    t = d["t"]
    n = t.shape[1]
    if kind == "random" or n < 4:
        return d
    lo, hi = -8.0, 8.0
    if kind == "twice":
        t[:, n // 3], t[:, n - 1], t[:, 1], t[:, n // 2] = lo, lo, hi, hi
    elif kind == "ends":
        t[:, 0], t[:, n - 1] = lo, hi
    elif kind == "ends-swapped":
        t[:, 0], t[:, n - 1] = hi, lo
    elif kind == "same-lane":
        t[:, 3], t[:, 3 + 256 * ((n - 4) // 256)] = hi, lo
        if n <= 260:
            t[:, 2] = lo                         # (short rows: neighbours, and the minimum twice)
    return d


NOISE_SCALE = 5.0


def theta_expected(c, d):
    """theta = (t - min) / (max - min) 111 (+ noise_scale noise), selected landmarks (x, y) pairs: the difference, the range, the
    division (1 ulp), the product, the noise product and the sum round once each."""
    t = d["t"]
    mn, mx = t.min(1, keepdim=True).values, t.max(1, keepdim=True).values
    q = (t - mn) / (mx - mn) * 111
    e = (3 * U + fb.ULP1) * q
    v = q
    if c["noise"]:
        v = q + fb.f32c(NOISE_SCALE) * d["noise"]
        e = e + U * (NOISE_SCALE * d["noise"]).abs() + U * v.abs()
    if c["sel"]:
        idx = (2 * d["sel"].long()[:, :, None] + torch.arange(2)).view(t.shape[0], -1)
        v, e = v.gather(1, idx), e.gather(1, idx)
    else:
        v, e = v[:, :2 * c["n_out"]], e[:, :2 * c["n_out"]]
    return {"theta": (v, e, False)}


def theta_bwd_expected(c, d):
    """dt = dtheta k with k = 111 / r, plus d/dmin = sum_j dtheta_j 111 (t_j - max) / r^2 at the FIRST arg-min and d/dmax = -sum_j
    dtheta_j 111 (t_j - min) / r^2 at the first arg-max.  r rounds (1), k = 111 / r (1 ulp), k2 = 111 / (r r) (1 + 1 ulp on top of
    2 x r's), each term g k2 (t - ext) three more; the sums: a thread's ceil(n / 256) terms in sequence, then an 8-level tree."""
    t, g = d["t"], d["dtheta"]
    n = t.shape[1]
    mn, imn = t.min(1, keepdim=True)
    mx, imx = t.max(1, keepdim=True)
    first = lambda m: (t == m).double().argmax(1, keepdim=True)
    imn, imx = first(mn), first(mx)
    r = mx - mn
    k, k2 = 111 / r, 111 / (r * r)
    dt = g * k
    e = (2 * U + fb.ULP1) * dt.abs()
    ta, tb = g * k2 * (t - mx), -g * k2 * (t - mn)
    depth = -(-n // 256) + 8
    rel = (3 * U + fb.ULP1 + 3 * U + depth * U)
    a, ae = ta.sum(1, keepdim=True), rel * ta.abs().sum(1, keepdim=True)
    b, be = tb.sum(1, keepdim=True), rel * tb.abs().sum(1, keepdim=True)
    add = torch.zeros_like(dt).scatter_add_(1, imn, a).scatter_add_(1, imx, b)
    adde = torch.zeros_like(dt).scatter_add_(1, imn, ae).scatter_add_(1, imx, be)
    out = dt + add
    return {"dt": (out, e + adde + U * out.abs() * (adde > 0), False),
            "mag": dt.abs() + torch.zeros_like(dt).scatter_add_(1, imn, ta.abs().sum(1, keepdim=True)).scatter_add_(1, imx, tb.abs().sum(1, keepdim=True))}


# ------------------------------------------------------------------------------------------------ lafs_cnn_grad_scale, lafs_cnn_grad_guard
P2 = lambda k: 2.0 ** k
SCALE_SLACK = 2.0 ** -20
"""scale[0] <= (target / m) (1 + SCALE_SLACK): the issue's reading of "brings max |g| to ~target" -- log2f of an fp32 neighbour below a
power of two may round to the integer itself, and floorf then keeps the larger power.  Not a measured value; a device that lands
outside it is a finding."""


def _nb(v, up):
    t = torch.tensor(v, dtype=f32)
    return float(torch.nextafter(t, torch.tensor(float("inf") if up else 0.0, dtype=f32)))


def _gs_grid():
    g = []
    for e in (-20, -3, 0, 1, 10):
        for nb in (None, False, True):
            m = P2(e) if nb is None else _nb(P2(e), nb)
            g.append(dict(id=f"gs-max-2^{e}{'' if nb is None else '-above' if nb else '-below'}", m=m, target=1024.0, state_target=0.0, kind="max"))
    g.append(dict(id="gs-max-3.7-state-target-256", m=3.7, target=1024.0, state_target=256.0, kind="max"))
    g.append(dict(id="gs-all-zero", m=0.0, target=1024.0, state_target=0.0, kind="max"))
    g.append(dict(id="gs-clamp-2^24", m=P2(-30), target=1024.0, state_target=0.0, kind="max"))
    g.append(dict(id="gs-clamp-2^-24", m=P2(40), target=1024.0, state_target=0.0, kind="max"))
    g.append(dict(id="gs-inf-in-the-last-element", m=2.0, target=1024.0, state_target=0.0, kind="inf"))
    g.append(dict(id="gs-nan-in-the-last-element", m=2.0, target=1024.0, state_target=0.0, kind="nan"))
    return _ids(g)


GS_CASES = _gs_grid()
GS_N = 257


def gs_inputs(c):
    """g [257]: |g| <= m with m itself at index 200 (negative); inf / NaN alone in the last element."""
    gen = _gen(c["id"])
    g = r32((torch.rand(GS_N, generator=gen, dtype=f64) - 0.5) * c["m"])
    g[200] = -c["m"]
    if c["kind"] == "inf":
        g[-1] = float("inf")
    if c["kind"] == "nan":
        g[-1] = float("nan")
    return dict(g=g)


def gs_contract(c, scale, inv, found):
    """The asserted contract of lafs_cnn_grad_scale (state machine of the comment in landmark_train.hip)."""
    target = c["state_target"] if c["state_target"] > 0 else c["target"]
    assert scale > 0 and math.frexp(scale)[0] == 0.5, f"{c['id']}: scale {scale} is not a power of two"
    assert scale * inv == 1.0, f"{c['id']}: scale x 1 / scale = {scale * inv!r}"
    assert P2(-24) <= scale <= P2(24), f"{c['id']}: scale {scale} outside [2^-24, 2^24]"
    assert found == (1.0 if c["kind"] != "max" else 0.0), f"{c['id']}: found_inf {found}"
    m = c["m"]
    if m == 0.0:
        assert scale == 1.0, f"{c['id']}: scale {scale} for an all-zero gradient"
        return
    ideal = target / m
    if ideal >= P2(24):
        assert scale == P2(24), f"{c['id']}: scale {scale}, expected the clamp 2^24"
    elif ideal <= P2(-24):
        assert scale == P2(-24), f"{c['id']}: scale {scale}, expected the clamp 2^-24"
    else:
        assert ideal / 2 < scale <= ideal * (1 + SCALE_SLACK), f"{c['id']}: scale {scale} for target / max|g| = {ideal!r}"


def guard_ref(state, target_max):
    """lafs_cnn_grad_guard on state [8] (a list of floats): (new state, whether the gradient range is zeroed)."""
    s = list(state)
    found = s[3] != 0.0
    t = s[2] if s[2] > 0 else target_max
    if found:
        t = max(t * 0.5, 1.0)
        s[4] += 1.0
        s[5] = 0.0
    else:
        s[5] += 1.0
        if s[5] >= 2000.0:
            t = min(t * 2, target_max)
            s[5] = 0.0
    s[2] = t
    return s, found


GUARD_CASES = _ids([
    dict(id="guard-found-halves", state=[8.0, 0.125, 1024.0, 1.0, 3.0, 17.0, 0.0, 0.0], target_max=4096.0, poison=None),
    dict(id="guard-found-floor-1", state=[8.0, 0.125, 1.5, 1.0, 0.0, 0.0, 0.0, 0.0], target_max=4096.0, poison=None),
    dict(id="guard-clean-counts", state=[8.0, 0.125, 1024.0, 0.0, 3.0, 17.0, 0.0, 0.0], target_max=4096.0, poison=None),
    dict(id="guard-clean-2000th-doubles", state=[8.0, 0.125, 1024.0, 0.0, 3.0, 1999.0, 0.0, 0.0], target_max=4096.0, poison=None),
    dict(id="guard-clean-2000th-capped", state=[8.0, 0.125, 4096.0, 0.0, 0.0, 1999.0, 0.0, 0.0], target_max=4096.0, poison=None),
    dict(id="guard-unset-target-takes-target_max", state=[8.0, 0.125, 0.0, 0.0, 0.0, 5.0, 0.0, 0.0], target_max=512.0, poison=None),
    dict(id="guard-inf-in-the-range", state=[8.0, 0.125, 1024.0, 0.0, 0.0, 100.0, 0.0, 0.0], target_max=4096.0, poison=float("inf")),
    dict(id="guard-nan-in-the-range", state=[8.0, 0.125, 1024.0, 0.0, 0.0, 100.0, 0.0, 0.0], target_max=4096.0, poison=float("nan")),
])
GUARD_N = 300000                                 # past one sweep of 1024 workgroups x 256 threads


# ================================================================================================ BatchNorm of the training plan
EPS52 = 2.0 ** -52
BN_EPS = 1e-5


def _bn_grid():
    """The (R, C, ld) set of the statistics cases, thinned: every (C, ld) once per R class, acts 0-2, residual, distributions and the
    momentum rotating over them; then the cases that need a shape of their own."""
    g, i = [], 0
    # (R = 7 stands in for the R = 3 of the statistics cases: with three rows dx keeps one degree of freedom of dz's three, a cancellation
    # that left 2.3 % of two cases' dx with a bound of two fp16 steps)
    for R in (1, 7, 257, 1000):
        for C, ld in BN_SHAPES:
            if (i + R) % 2 and R in (7, 257):
                i += 1
                continue
            g.append(dict(id=f"bn-R{R}-C{C}-ld{ld}-act{i % 3}-{DISTS[i % 3]}", R=R, C=C, ld=ld, act=i % 3, dist=DISTS[i % 3], resid=i % 2 == 0,
                          mom=(0.1, 1.0)[(i // 2) % 2], run=i % 4 != 3, HW=(None, 1, 4, 49)[i % 4] if R == 1000 or R == 1 else None,
                          gs=(None, 64.0)[i % 2], affine=i % 5 != 4, const=R >= 257))
            i += 1
    # 263 169 x 64 / 8 = 2 105 352 > 8192 x 256: the grid-stride loops of both apply kernels take a second trip
    g.append(dict(id="bn-R263169-C64-ld64-second-trip", R=263169, C=64, ld=64, act=2, dist="normal", resid=False, mom=0.1, run=True, HW=None,
                  gs=None, affine=True, const=False))
    g.append(dict(id="bn-R980-C40-ld40-HW49-dsums-old", R=980, C=40, ld=40, act=2, dist="normal", resid=True, mom=0.1, run=True, HW=49, gs=64.0,
                  affine=True, const=True))
    for c in g:
        if c["HW"] is not None and c["R"] % c["HW"]:
            c["HW"] = 1 if c["R"] == 1 else 4 if c["R"] % 4 == 0 else None
    return _ids(g)


BN_CASES = _bn_grid()


def bn_bwd_modes(c):
    """(entry point, frozen) pairs a case runs the backward with.  At R = 1 the training-mode dx is zero by total cancellation (dz minus
    its own mean): there is no 16-bit step to hold a bound against, so those cases -- which exist for the R - 1 -> 1 branch of the
    running variance, in the apply kernel -- run the eval-mode backward only."""
    return ([("lafs_cnn_bn_bwd", False)] if c["R"] > 1 else []) + ([("lafs_cnn_bn_bwd_eval", True)] if c["R"] < 100000 else [])


def bn_inputs(c, exact_z=False):
    """x fp16 [R, ld] with zero pad channels; sums: the fp64 column sums of x itself (an operand of lafs_cnn_bn_apply); `const`: column
    1 is exactly constant at 2^-10 (variance 0: rstd = eps^-1/2 multiplies the mean's allowance; a small constant keeps the bound under
    the cap, as for the LayerNorm cases).  dy = 0.5 + randn: with a zero-mean dy the batch mean of dz is a cancelling sum, the dx of the
    elements relu switches off (-gamma rstd (mean dz + xhat mean(dz xhat))) is ~R^-1/2 of the terms' size, and 2.2-2.9 % of three cases'
    dx carried a bound of two fp16 steps, above the 2 % cap.  exact_z: statistics (0, 1), gamma 1, beta 0 and x on the kinks -- z = x exactly."""
    gen = _gen(c["id"], exact_z)
    R, C, ld = c["R"], c["C"], c["ld"]
    pad = lambda v: torch.cat([v, torch.zeros(*v.shape[:-1], ld - C, dtype=f64)], -1)
    x = rh(_dist(gen, c["dist"], R, C) * (2.0 ** -10 if R == 1 else 1.0))          # (R = 1: every column is constant -- small values, as below)
    if c["const"]:
        x[:, 1] = 2.0 ** -10
    if exact_z:
        x = torch.tensor([-3.0, 0.0, 3.0, 1.5, -1.0, 4.0], dtype=f64)[torch.arange(R * C) % 6].view(R, C)
    d = dict(x=pad(x), gamma=r32(1 + 0.5 * _rn(gen, C)), beta=r32(0.5 * _rn(gen, C)), resid=pad(rh(_rn(gen, R, C))), dy=pad(rh(0.5 + _rn(gen, R, C))),
             rm=r32(_rn(gen, C)), rv=r32(0.5 + torch.rand(C, generator=gen, dtype=f64)), dgamma_old=r32(_rn(gen, C)), dbeta_old=r32(_rn(gen, C)))
    if exact_z:
        d["gamma"], d["beta"] = torch.ones(C, dtype=f64), torch.zeros(C, dtype=f64)
    d["sums"] = torch.cat([x.sum(0), (x * x).sum(0)])
    if c["const"]:
        d["sums"][1], d["sums"][C + 1] = R * 2.0 ** -10, R * 2.0 ** -20
    if c["HW"]:
        d["add"] = pad(rh(_rn(gen, R // c["HW"], C)))
    return d


def bn_stat(c, d):
    """mean, biased variance and rstd as the apply kernel forms them in fp64 from the sums it is handed, with what the fp64 arithmetic
    can be off by (a few 2^-52 of the terms: E[x^2] - mean^2 cancels in double, not in float)."""
    R, C = c["R"], c["C"]
    s1, s2 = d["sums"][:C], d["sums"][C:]
    m = s1 / R
    me = 2 * EPS52 * m.abs()
    ex2 = s2 / R
    var = (ex2 - m * m).clamp_min(0)
    vare = 4 * EPS52 * (ex2 + m * m)
    eps = fb.f32c(BN_EPS)
    rs = 1 / (var + eps).sqrt()
    rse = rs * vare / (2 * (var + eps)) + 4 * EPS52 * rs
    return (m, me), (var, vare), (rs, rse)


def bn_apply_expected(c, d, r32=r32, rh=rh):
    """y = act(x scale + shift) (+ resid) with scale = rstd gamma, shift = beta - mean scale in fp32 from the fp32 roundings of the fp64
    statistics: scale rounds (1), shift twice, the fma once, the residual add once.  stat = the fp32 roundings themselves.  (r32, rh:
    the two roundings, replaced by the identity for the semantics tie of tests/test_oracle_cnn_host.py.)  Running
    statistics: (1 - momentum) rounds, each product and the sum round; the unbiased factor (float) R / (float) (R - 1) is a division
    (1 ulp) and one more product."""
    R, C, ld = c["R"], c["C"], c["ld"]
    (m, me), (var, vare), (rs, rse) = bn_stat(c, d)
    m32, m32e = fb.flip(m, me, r32)
    rs32, rs32e = fb.flip(rs, rse, r32)
    v32, v32e = fb.flip(var, vare, r32)
    g, b, x = d["gamma"], d["beta"], d["x"][:, :C]
    scale = rs32 * g
    scale_e = rs32e * g.abs() + U * scale.abs()
    shift = b - m32 * scale
    # (an error of scale moves x scale and -mean scale together: it enters as |x - mean| scale_e, not once per term)
    shift_e = m32e * scale.abs() + U * (m32 * scale).abs() + U * shift.abs()
    z = x * scale + shift
    ze = (x - m32).abs() * scale_e + shift_e + U * z.abs()
    a, ae = fb.act(z, ze, c["act"])
    if c["resid"]:
        a = a + d["resid"][:, :C]
        ae = ae + U * a.abs()
    y, ye = fb.flip(a, ae, rh)
    zpad = torch.zeros(R, ld - C, dtype=f64, device=x.device)
    out = {"y": (torch.cat([y, zpad], 1), torch.cat([ye, zpad], 1), True), "stat": (torch.cat([m32, rs32]), torch.cat([m32e, rs32e]), False),
           "mag_stat": torch.cat([m32.abs(), rs32]), "mag_y": g.abs() * rs * (x.abs() + m.abs()) + b.abs()}
    if c["run"]:
        mom = fb.f32c(c["mom"])
        om = fb.f32c(1.0) - mom
        a1, b1 = om * d["rm"], mom * m32
        rm = a1 + b1
        rme = 2 * U * a1.abs() + U * b1.abs() + mom * m32e + U * rm.abs()
        fac = R / max(R - 1, 1)
        a2, b2 = om * d["rv"], mom * v32 * fac
        rv = a2 + b2
        rve = 2 * U * a2.abs() + (2 * U + fb.ULP1) * b2.abs() + mom * fac * v32e + U * rv.abs()
        out["rm"], out["rv"] = (rm, rme, False), (rv, rve, False)
        out["mag_rm"], out["mag_rv"] = a1.abs() + b1.abs(), a2.abs() + mom * fac * (d["sums"][C:] / R + m * m)      # (var is formed from E[x^2] and mean^2)
    return out


def bn_bwd_expected(c, d, stat, frozen=False, dsums_old=None, exact_z=False, rh=rh):
    """lafs_cnn_bn_bwd (frozen: _eval) on the fp32 statistics it is handed (stat [2 C], widened).  d' = dy + add / HW: one fma with the
    rounded reciprocal; xhat = (x - mean) rstd rounds twice; z = fma(xhat, gamma, beta) once more; act' by fb.act_grad with its knife
    edges; dz = d' act' rounds.  dsums (fp64): per workgroup an fp32 partial of depth fb.tree_depth, then fp64 atomics.  dx = gamma rstd
    (dz - sum dz / R - xhat sum(dz xhat) / R): the kernel's own sums (within their bound) rounded to fp32, three roundings inside, two
    outside.  dgamma / dbeta += the sums x 1 / scale, rounded to fp32, added in fp32.  exact_z: every operation up to z is exact."""
    R, C, ld = c["R"], c["C"], c["ld"]
    x, dy, g, b = d["x"][:, :C], d["dy"][:, :C], d["gamma"], d["beta"]
    m, rs = stat[:C], stat[C:]
    dd, dde = dy, torch.zeros_like(dy)
    if c["HW"]:
        a = d["add"][:, :C].repeat_interleave(c["HW"], 0) / c["HW"]
        dd = dy + a
        dde = U * a.abs() + U * dd.abs()
    xh = (x - m) * rs
    xhe = torch.zeros_like(xh) if exact_z else 2 * U * xh.abs()
    z = xh * g + b
    ze = torch.zeros_like(z) if exact_z else xhe * g.abs() + U * z.abs()
    ad, ade, knife = fb.act_grad(z, ze, c["act"])
    dz = dd * ad
    dze = dde * ad.abs() + dd.abs() * ade + U * dz.abs()
    t2 = dz * xh
    t2e = dze * xh.abs() + dz.abs() * xhe
    rpb = rows_per_block(R)
    depth = fb.tree_depth(min(R, rpb), 256 // group_block(ld))
    nblk = -(-R // rpb)
    old = torch.zeros(2 * C, dtype=f64, device=x.device) if dsums_old is None else dsums_old
    s = torch.cat([dz.sum(0), t2.sum(0)]) + old
    sabs = torch.cat([dz.abs().sum(0), t2.abs().sum(0)])
    se = torch.cat([dze.sum(0), t2e.sum(0)]) + depth * U * sabs + (nblk + 1) * EPS52 * (sabs + old.abs())
    knife_share = torch.cat([(dd.abs() * ade * knife).sum(0), (dd.abs() * ade * knife * xh.abs()).sum(0)])
    out = {"dsums": (s, se, False), "mag_dsums": sabs + old.abs(), "knife": int(knife.sum()), "knife_share": knife_share}
    c4, c5 = (torch.zeros(C, dtype=f64, device=x.device),) * 2 if frozen else (s[:C] / R, s[C:] / R)
    c4e, c5e = (torch.zeros_like(c4),) * 2 if frozen else (se[:C] / R + U * c4.abs(), se[C:] / R + U * c5.abs())
    gr = g * rs
    inner = dz - c4 - xh * c5
    ie = dze + c4e + xh.abs() * c5e + xhe * c5.abs() + 3 * U * (dz.abs() + c4.abs() + (xh * c5).abs())
    dx = gr * inner
    dxe = gr.abs() * ie + 2 * U * dx.abs()
    zpad = torch.zeros(R, ld - C, dtype=f64, device=x.device)
    dxr, dxb = fb.flip(dx, dxe, rh)
    out["dx"] = (torch.cat([dxr, zpad], 1), torch.cat([dxb, zpad], 1), True)
    if c["affine"]:
        inv = 1.0 if c["gs"] is None else 1.0 / c["gs"]
        for name, k, oldv in (("dbeta", 0, d["dbeta_old"]), ("dgamma", 1, d["dgamma_old"])):
            add = s[k * C:(k + 1) * C] * inv
            v = oldv + add
            out[name] = (v, se[k * C:(k + 1) * C] * inv + U * add.abs() + U * v.abs(), False)
            out["mag_" + name] = sabs[k * C:(k + 1) * C] * inv + oldv.abs()
    return out


def bn_eval_sums_expected(rm, rv, R):
    """sums[c] = R mean, sums[C + c] = R (var + mean^2) in fp64: exact up to 2 roundings (3 for the second)."""
    s = torch.cat([R * rm, R * (rv + rm * rm)])
    return {"sums": (s, 3 * EPS52 * s.abs(), False)}


# ================================================================================================ the three tables
def table_entries():
    """A small arena and the entries landmark_train._Tables builds for it: ragged [5, 7] into [32, 32] plain and [40, 16] transposed, a
    depthwise C = 20, k k = 25, ld = 32, and images of exactly 1024 and of 1025 elements."""
    from lafs_cvpr2024_amd.landmark_train import _Tables
    T = _Tables()
    arena = {}
    off = 0
    for name, n in (("a", 5 * 7), ("gap0", 13), ("dw", 20 * 25), ("b", 32 * 32), ("gap1", 7), ("c", 25 * 41)):
        arena[name] = (off, n)
        off += n
    spec = dict(arena=arena, size=off, T=T)
    a, dwo, bo, co = arena["a"][0], arena["dw"][0], arena["b"][0], arena["c"][0]
    spec["cast"] = [("a", 5, 7, 32, 32, False, T.operand(a, 5, 7, 32, 32, False)), ("a", 5, 7, 40, 16, True, T.operand(a, 5, 7, 40, 16, True)),
                    ("b", 32, 32, 32, 32, False, T.operand(bo, 32, 32, 32, 32, False)), ("c", 25, 41, 25, 41, False, T.operand(co, 25, 41, 25, 41, False)),
                    ("c", 25, 41, 32, 48, True, T.operand(co, 25, 41, 32, 48, True))]
    spec["dwl"] = [("dw", 20, 25, 32) + T.depthwise(dwo, 20, 25, 32)]
    spec["grad"] = [("a", 5, 7, 32, 32, T.gradient(5, 7, 32, 32, a)), ("b", 32, 32, 32, 32, T.gradient(32, 32, 32, 32, bo)),
                    ("c", 25, 41, 32, 48, T.gradient(25, 41, 32, 48, co))]
    return spec


def table_inputs(spec):
    gen = _gen("tables")
    T = spec["T"]
    return dict(master=r32(_rn(gen, spec["size"])), padded=r32(_rn(gen, T.grad_size)), grad_old=r32(_rn(gen, spec["size"])))


SENT16 = 777.0          # what the destination images hold before the launch (exact in fp16)


def tables_expected(spec, d, gscale_inv=1.0, ignore_transpose=False):
    """The operand images (fp16, one rounding, zero padding, the 64-element gaps between images left alone), the tap-major depthwise
    image (fp32 moves) and the gradient fold grad += padded corner x 1 / scale (the product and the sum round; arena elements no entry
    covers are left alone)."""
    T, arena, m = spec["T"], spec["arena"], d["master"]
    cast = torch.full((T.cast_size,), SENT16, dtype=f64)
    for name, rows, cols, prow, pcol, tr, off in spec["cast"]:
        src = m[arena[name][0]:arena[name][0] + rows * cols].view(rows, cols)
        img = torch.zeros(prow, pcol, dtype=f64)
        img[:rows, :cols] = src
        img = img.t() if tr else img
        cast[off:off + img.numel()] = rh(img.reshape(-1))
    dwl = torch.full((T.dw_size,), SENT16, dtype=f64)
    for name, C, kk, ld, off, goff in spec["dwl"]:
        img = torch.zeros(kk, ld, dtype=f64)
        img[:, :C] = m[arena[name][0]:arena[name][0] + C * kk].view(C, kk).t()
        dwl[off:off + kk * ld] = img.reshape(-1)
    grad, ge = d["grad_old"].clone(), torch.zeros(spec["size"], dtype=f64)
    for name, rows, cols, prow, pcol, off in spec["grad"]:
        add = d["padded"][off:off + prow * pcol].view(prow, pcol)[:rows, :cols].reshape(-1) * gscale_inv
        sl = slice(arena[name][0], arena[name][0] + rows * cols)
        grad[sl] += add
        ge[sl] = U * grad[sl].abs()                       # (1 / scale is a power of two: the product is exact)
    for name, C, kk, ld, off, goff in spec["dwl"]:
        img = d["padded"][goff:goff + kk * ld].view(kk, ld)[:, :C]
        add = (img.reshape(-1)[:C * kk].view(C, kk) if ignore_transpose else img.t()).reshape(-1) * gscale_inv
        sl = slice(arena[name][0], arena[name][0] + C * kk)
        grad[sl] += add
        ge[sl] = U * grad[sl].abs()
    z = lambda t: torch.zeros_like(t)
    return {"cast": (cast, z(cast), True), "dwl": (dwl, z(dwl), False), "grad": (grad, ge, False)}
