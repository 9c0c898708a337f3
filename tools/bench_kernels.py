#!/usr/bin/env python3
"""Micro-benchmarks of the hot kernels at the C2 shapes (ViT-S, B=64: 44160 student tokens).  GPU box only.
usage: python tools/bench_kernels.py [nt] [tn] [wg] [wgg] [tnsplits] [tnpart] [augment] [facetensor] [verify] [ijb] [ln] [dzn] [attn]
       (default: nt tn attn)"""
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch
from lafs_cvpr2024_amd import _lib, ops

dev, bf, T = "cuda", torch.bfloat16, 44160
which = set(sys.argv[1:]) or {"nt", "tn", "attn"}


def timeit(fn, iters=20):
    for _ in range(3):
        fn()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda.synchronize(); e0.record()
    for _ in range(iters):
        fn()
    e1.record(); torch.cuda.synchronize()
    return e0.elapsed_time(e1) / iters * 1e-3


def nt(M, N, K, epi, name):
    A = torch.randn(M, K, device=dev).to(bf); B = (torch.randn(N, K, device=dev) * .02).to(bf)
    bias = torch.zeros(N, device=dev)
    kw = {}
    f32 = epi in (_lib.EPI_RESID_F32, _lib.EPI_F32)
    out = torch.empty(M, N, device=dev, dtype=torch.float32 if f32 else bf)
    byts = (M * K + N * K) * 2 + M * N * (4 if f32 else 2)
    if epi == _lib.EPI_BF16_GELU:
        kw["out2"] = torch.empty(M, N, device=dev, dtype=bf); byts += M * N * 2
    if epi == _lib.EPI_RESID_F32:
        kw["resid"] = torch.randn(M, N, device=dev); byts += M * N * 4
    if epi == _lib.EPI_DGELU_BF16:
        kw["aux"] = torch.randn(M, N, device=dev).to(bf); byts += M * N * 2
    t = timeit(lambda: ops.gemm_nt(A, B, epi, bias=None if epi == _lib.EPI_DGELU_BF16 else bias, out=out, **kw))
    print(f"NT {name:24s} M={M:6d} N={N:6d} K={K:5d}: {t*1e6:8.1f} us  {2*M*N*K/t/1e12:7.1f} TF/s  {byts/t/1e9:7.0f} GB/s")


def tn(M, N1, N2, name, splits=0):
    A = torch.randn(M, N1, device=dev).to(bf); B = torch.randn(M, N2, device=dev).to(bf)
    C = torch.zeros(N1, N2, device=dev)
    t = timeit(lambda: ops.gemm_tn_acc(A, B, C, splits=splits))
    print(f"TN {name:24s} M={M:6d} N1={N1:6d} N2={N2:5d}: {t*1e6:8.1f} us  {2*M*N1*N2/t/1e12:7.1f} TF/s  {(M*(N1+N2)*2)/t/1e9:7.0f} GB/s")


def wg(M, N1, N2, name):
    A = torch.randn(M, N1, device=dev).to(bf); B = torch.randn(M, N2, device=dev).to(bf)
    C = torch.zeros(N1, N2, device=dev); ws = ops.wgrad_workspace(M, N1, N2, dev); cs = torch.zeros(N1, device=dev)
    t = timeit(lambda: ops.wgrad(A, B, C, accumulate=False, colsum=cs, workspace=ws))
    err = ((C - A.float().t() @ B.float()).abs().max() / C.abs().max()).item()
    print(f"WG {name:24s} M={M:6d} N1={N1:6d} N2={N2:5d}: {t*1e6:8.1f} us  {2*M*N1*N2/t/1e12:7.1f} TF/s  {(M*(N1+N2)*2)/t/1e9:7.0f} GB/s  "
          f"ws {ws.numel()*4/1e6:6.1f} MB  relerr {err:.1e}")


SHAPES = [(T, 1152, 384, _lib.EPI_BF16, "qkv fwd"), (T, 384, 384, _lib.EPI_RESID_F32, "proj fwd"),
          (T, 1536, 384, _lib.EPI_BF16_GELU, "fc1 fwd"), (T, 384, 1536, _lib.EPI_RESID_F32, "fc2 fwd"),
          (T, 1536, 384, _lib.EPI_DGELU_BF16, "fc2 dgrad"), (T, 384, 1536, _lib.EPI_BF16, "fc1 dgrad"),
          (T, 384, 384, _lib.EPI_BF16, "proj dgrad"), (T, 384, 1152, _lib.EPI_BF16, "qkv dgrad"),
          (640, 100096, 256, _lib.EPI_F32, "last layer"), (4096, 4096, 4096, _lib.EPI_BF16, "square 4k")]

if "nt" in which:
    for M, N, K, e, n in SHAPES:
        nt(M, N, K, e, n)
if "tn" in which:
    tn(T, 384, 1536, "fc2 wgrad"); tn(T, 1536, 384, "fc1 wgrad"); tn(T, 384, 384, "proj wgrad"); tn(T, 1152, 384, "qkv wgrad")
    tn(640, 100096, 256, "last wgrad")
    TB = 25216                                                          # ViT-B fine-tune: 128 x 197 tokens
    tn(TB, 768, 2048, "B fc2 wgrad"); tn(TB, 2048, 768, "B fc1 wgrad"); tn(TB, 2112, 768, "B qkv wgrad"); tn(TB, 768, 704, "B proj wgrad")
if "wg" in which:
    print("--- wide-tile weight gradient (lafs_wgrad) vs the round-1 kernel (lafs_gemm_tn_acc)")
    TB = 25216
    for (M, N1, N2, name) in ((T, 384, 1536, "fc2 wgrad"), (T, 1536, 384, "fc1 wgrad"), (T, 384, 384, "proj wgrad"), (T, 1152, 384, "qkv wgrad"),
                              (TB, 768, 2048, "B fc2 wgrad"), (TB, 2048, 768, "B fc1 wgrad"), (TB, 2112, 768, "B qkv wgrad"),
                              (TB, 768, 704, "B proj wgrad"), (8192, 4096, 4096, "square")):
        wg(M, N1, N2, name); tn(M, N1, N2, name)
if "wgg" in which:
    print("--- the four weight gradients of one block: 4 x round-1 kernel | 4 x lafs_wgrad | ONE lafs_wgrad_group")
    for (Mx, D, I, H, name) in ((T, 384, 384, 1536, "ViT-S student"), (25216, 384, 384, 1536, "ViT-S teacher-size"), (25216, 768, 704, 2048, "ViT-B fine-tune")):
        mk = lambda r, c: torch.randn(r, c, device=dev).to(bf)
        gbm, a, du, h2, gba, o, dqkv, h1 = mk(Mx, D), mk(Mx, H), mk(Mx, H), mk(Mx, D), mk(Mx, D), mk(Mx, I), mk(Mx, 3 * I), mk(Mx, D)
        pairs = [(gbm, a), (du, h2), (gba, o), (dqkv, h1)]
        Cs = [torch.zeros(x.shape[1], y.shape[1], device=dev) for x, y in pairs]
        bs = [torch.zeros(x.shape[1], device=dev) for x, _ in pairs]
        t0 = timeit(lambda: [ops.gemm_tn_acc(x, y, c, colsum=b) for (x, y), c, b in zip(pairs, Cs, bs)])
        wss = [ops.wgrad_workspace(Mx, x.shape[1], y.shape[1], dev) for x, y in pairs]
        t1 = timeit(lambda: [ops.wgrad(x, y, c, accumulate=True, colsum=b, workspace=w) for (x, y), c, b, w in zip(pairs, Cs, bs, wss)])
        probs = [(x, y, c, True, b) for (x, y), c, b in zip(pairs, Cs, bs)]
        ws = ops.wgrad_group(probs)
        t2 = timeit(lambda: ops.wgrad_group(probs, workspace=ws))
        fl = sum(2 * Mx * x.shape[1] * y.shape[1] for x, y in pairs)
        print(f"   {name:20s} M={Mx}: round-1 {t0*1e6:7.1f} us | 4 x wgrad {t1*1e6:7.1f} us | group {t2*1e6:7.1f} us = {fl/t2/1e12:6.1f} TF/s  (ws {ws.numel()*4/1e6:.1f} MB)")
if "tnsplits" in which:
    print("--- TN wgrad vs number of M-slices (0 = library default)")
    for sp in (0, 8, 16, 24, 32):
        tn(T, 384, 1536, f"fc2 wgrad s{sp}", splits=sp); tn(T, 1536, 384, f"fc1 wgrad s{sp}", splits=sp)
        tn(T, 384, 384, f"proj wgrad s{sp}", splits=sp); tn(T, 1152, 384, f"qkv wgrad s{sp}", splits=sp)
if "tnpart" in which:
    print("--- TN wgrad: device atomics vs per-XCD partial images (+ fold)")
    for (M, N1, N2, name) in ((T, 384, 1536, "fc2 wgrad"), (T, 1536, 384, "fc1 wgrad"), (T, 384, 384, "proj wgrad"), (T, 1152, 384, "qkv wgrad")):
        A = torch.randn(M, N1, device=dev).to(bf); B = torch.randn(M, N2, device=dev).to(bf)
        Cd = torch.zeros(N1, N2, device=dev); part = torch.zeros(8, N1, N2, device=dev)
        ops.gemm_tn_acc(A, B, Cd)
        ops.gemm_tn_part(A, B, part); Cp = ops.reduce_partials(part, torch.zeros(N1, N2, device=dev))
        ref = A.float().t() @ B.float()
        print(f"   {name}: max|atomics-ref| {float((Cd-ref).abs().max()):.3e}  max|partials-ref| {float((Cp-ref).abs().max()):.3e}  (|ref| {float(ref.abs().max()):.1f})"
              f"  images left zero: {float(part.abs().max()) == 0.0}")
        t0 = timeit(lambda: ops.gemm_tn_acc(A, B, Cd))
        t1 = timeit(lambda: ops.gemm_tn_part(A, B, part))
        out = torch.zeros(N1, N2, device=dev)
        t2 = timeit(lambda: ops.reduce_partials(part, out))
        print(f"   {name}: atomics {t0*1e6:7.1f} us | partial {t1*1e6:7.1f} us + fold {t2*1e6:6.1f} us")
if "augment" in which:
    from lafs_cvpr2024_amd.augment import DeviceAugmenter
    da = DeviceAugmenter(64, n_local=8, device=dev, seed=0)
    u8 = torch.randint(0, 256, (64, 3, 112, 112), device=dev, dtype=torch.uint8)
    t = timeit(lambda: da(u8), iters=20)                     # vectorised host sampling + parameter upload + one launch
    from lafs_cvpr2024_amd.ops import _p, call
    tk = timeit(lambda: call("lafs_augment_views", _p(u8), _p(da.params_dev), _p(da.table), 64, 10, _p(da.views)), iters=20)
    print(f"--- device augmentation: 64 images -> 1280 views: {t*1e6:8.1f} us per batch end to end, kernel alone {tk*1e6:8.1f} us "
          f"({1280/tk/1e6:.2f} M views/s)")
if "facetensor" in which:
    import time
    import numpy as np
    from lafs_cvpr2024_amd.face_tensor_aug import FaceTensorAug, RECORD
    from lafs_cvpr2024_amd.ops import _p, call
    aug = FaceTensorAug(0)
    t0 = time.perf_counter(); recs = aug.sample(128); th = time.perf_counter() - t0      # host draws, one CPU thread
    u8 = torch.randint(0, 256, (128, 3, 112, 112), device=dev, dtype=torch.uint8)
    out = torch.empty_like(u8)
    rdev = torch.from_numpy(recs.view(np.uint8).reshape(128, RECORD.itemsize)).to(dev)
    te = timeit(lambda: aug(u8, records=recs, out=out), iters=50)                   # record validation + upload + one launch
    tk = timeit(lambda: call("lafs_face_tensor_aug", _p(u8), _p(out), _p(rdev), 128, 112, 112, 112), iters=50)
    print(f"--- torchvision tensor chain (RandomResizedCrop / ColorJitter / RandomErasing), 128 x 3 x 112^2 uint8: kernel {tk*1e6:7.1f} us "
          f"({2 * u8.numel() / tk / 1e9:.0f} GB/s), end to end with given records {te*1e6:7.1f} us, host sampling {th*1e3:.1f} ms per batch")
if "ln" in which:
    print("--- LayerNorm forward / backward at the student shape (44160 x 384); distinct buffers per call (no cache residency)")
    L = 6
    xs = [torch.randn(T, 384, device=dev) for _ in range(L)]; dys = [torch.randn(T, 384, device=dev).to(bf) for _ in range(L)]
    gs = [torch.randn(T, 384, device=dev) for _ in range(L)]; gbs = [torch.empty(T, 384, device=dev, dtype=bf) for _ in range(L)]
    gam = torch.ones(384, device=dev); bet = torch.zeros(384, device=dev); dgam = torch.zeros(384, device=dev); dbet = torch.zeros(384, device=dev)
    outs = [ops.layernorm_fwd(x, gam, bet, 1e-6) for x in xs]
    tf = timeit(lambda: [ops.layernorm_fwd(x, gam, bet, 1e-6) for x in xs]) / L
    tb = timeit(lambda: [ops.layernorm_bwd(dys[i], xs[i], outs[i][2], gam, gs[i], dgam, dbet, accumulate=True, gb_out=gbs[i]) for i in range(L)]) / L
    print(f"   fwd {tf*1e6:6.1f} us ({T*384*6/tf/1e9:6.0f} GB/s)   bwd {tb*1e6:6.1f} us ({T*384*16/tb/1e9:6.0f} GB/s)")
if "dzn" in which:
    print("--- head backward dzn = dlogits Wn (M=640, N=256, K=100096): split-K atomics vs slice images + fold")
    from lafs_cvpr2024_amd.ops import _p, call
    A = torch.randn(640, 100096, device=dev).to(bf); B = torch.randn(256, 100096, device=dev).to(bf)
    for sp in (16, 32, 64, 96):
        ta = timeit(lambda: ops.gemm_nt(A, B, _lib.EPI_ATOMIC_F32, splits=sp))
        ns = _lib.lib().lafs_gemm_nt_slices(100096, sp)
        part = torch.empty(ns, 640, 256, device=dev); out = torch.empty(640, 256, device=dev)
        def f():
            ops.gemm_nt(A, B, _lib.EPI_F32, splits=sp, out=part.view(-1, 256), out_rows=ns * 640)
            call("lafs_sum_slices", _p(part), 640 * 256, ns, 640 * 256, _p(out))
        tb = timeit(f)
        ref = ops.gemm_nt(A, B, _lib.EPI_ATOMIC_F32, splits=sp)
        print(f"   splits {sp:3d}: atomics {ta*1e6:6.1f} us | images + fold {tb*1e6:6.1f} us   max diff {float((ref - out).abs().max()):.2e} (|ref| {float(ref.abs().max()):.1f})")
if "attn" in which:
    print("--- attention (student shapes: 128 seqs x 197 and 512 x 37, 6 heads)")
    for nseq, n in ((128, 197), (512, 37)):
        heads = 6
        cu = torch.arange(0, (nseq + 1) * n, n, dtype=torch.int32, device=dev)
        qkv = torch.randn(nseq * n, 3 * heads * 64, device=dev).to(bf)
        out, lse = ops.attention_fwd(qkv, cu, n, heads, 0.125)
        dout = torch.randn(nseq * n, heads * 64, device=dev).to(bf)
        tf = timeit(lambda: ops.attention_fwd(qkv, cu, n, heads, 0.125))
        tb = timeit(lambda: ops.attention_bwd(qkv, out, dout, lse, cu, n, heads, 0.125))
        fl = 4 * nseq * heads * n * n * 64
        print(f"   {nseq:4d} x {n:3d}: fwd {tf*1e6:7.1f} us ({fl/tf/1e12:6.1f} TF/s)   bwd {tb*1e6:7.1f} us ({2.5*fl/tb/1e12:6.1f} TF/s)")

if "verify" in which:
    # verification (verification.py): extraction rate of the flip test at batch 128 on Part-fViT ViT-B with / without the landmark
    # branch, the host metric at P = 6000, and a whole 6000-pair set against the module path + the reference-style numpy sweep
    import time
    import numpy as np
    from lafs_cvpr2024_amd import verification as V
    from lafs_cvpr2024_amd.face_pre_pro.ViT_face import ViT_face_landmark_patch8
    from lafs_cvpr2024_amd.vision_transformer import attach_arena
    P = 6000
    x = torch.randint(0, 256, (2 * P, 3, 112, 112), dtype=torch.uint8)
    issame = np.arange(P) % 2 == 0
    for land in (True, False):
        torch.manual_seed(0)
        m = ViT_face_landmark_patch8(loss_type="None", GPU_ID=None, num_class=10, image_size=112, patch_size=8, dim=768, depth=12,
                                     heads=11, mlp_dim=2048, dropout=0.1, emb_dropout=0.1, with_land=land)
        attach_arena(m, dev)
        ev = V.VerificationEvaluator(m, 128, dev)
        ev(x[:1024], issame[:512])                                     # warm-up (code objects, plans)
        torch.cuda.synchronize(); t0 = time.perf_counter()
        ev(x, issame)
        torch.cuda.synchronize(); tv = time.perf_counter() - t0
        print(f"verify with_land={int(land)}: {P} pairs ({2 * P} images, x2 flip) in {tv:.2f} s = {2 * P / tv:.0f} images/s "
              f"({4 * P / tv:.0f} embeddings/s) at batch 128")
        if land:
            # module path: backbone.eval() forward per copy (MIOpen landmark branch) + perform_val's numpy host math
            m.eval()
            t0 = time.perf_counter()
            embs = []
            with torch.no_grad():
                for flip in (False, True):
                    e = np.zeros((2 * P, 768))
                    for i in range(0, 2 * P, 128):
                        b = (x[i:i + 128].float() / 255.0 - 0.5).to(dev)
                        e[i:i + 128] = m(b.flip(3) if flip else b).cpu().numpy()
                    embs.append(e)
            t_emb = time.perf_counter() - t0
            e = embs[0] + embs[1]
            e = e / np.linalg.norm(e, axis=1, keepdims=True)
            dist = np.sum(np.square(e[0::2] - e[1::2]), 1)
            t1 = time.perf_counter()
            from sklearn.model_selection import KFold
            for train, test in KFold(10, shuffle=False).split(np.arange(P)):
                for t in V.THRESHOLDS:
                    for sel in (train, test):
                        pred = dist[sel] < t
                        _ = (np.sum(pred & issame[sel]), np.sum(pred & ~issame[sel]), np.sum(~pred & ~issame[sel]), np.sum(~pred & issame[sel]))
            t_sweep = time.perf_counter() - t1
            print(f"module path: {P} pairs: forward {t_emb:.2f} s + numpy sweep {t_sweep:.2f} s = {t_emb + t_sweep:.2f} s")
    h = V.hist_from_dist(np.random.RandomState(0).uniform(0, 4, P), issame)
    t0 = time.perf_counter()
    for _ in range(10):
        V.metrics_from_hist(h)
    print(f"host metric from the histogram at P = {P}: {(time.perf_counter() - t0) / 10 * 1e3:.2f} ms")

if "ijb" in which:
    # IJB-C sized protocol (ijb_evaluation.py): N = 469 375 images, T = 23 124 templates, P = 15 658 489 pairs, D = 768, and the
    # alignment kernel at the reference's batch of 360 loose crops; beside it the numpy oracle of tests/ijb_oracle.py on this host
    import time
    import numpy as np
    from lafs_cvpr2024_amd import ijb_evaluation as J
    from lafs_cvpr2024_amd.ops import _p, call
    sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "tests"))
    import ijb_oracle as IO
    N, Tn, P, D, B = 469375, 23124, 15658489, 768, 360
    rng = np.random.RandomState(0)
    # alignment
    hw = np.stack([rng.randint(120, 201, B), rng.randint(120, 201, B)], 1).astype(np.int32)
    sizes = hw[:, 0].astype(np.int64) * hw[:, 1] * 3
    offs = np.r_[0, np.cumsum(sizes)]
    src = torch.randint(0, 256, (int(offs[-1]),), dtype=torch.uint8, device=dev)
    th = rng.uniform(-0.3, 0.3, B); z = rng.uniform(0.9, 1.5, B)
    maps = np.stack([z * np.cos(th), -z * np.sin(th), rng.uniform(0, 20, B), z * np.sin(th), z * np.cos(th), rng.uniform(0, 20, B)], 1)
    d_off, d_hw = torch.from_numpy(offs[:B].copy()).to(dev), torch.from_numpy(hw).to(dev)
    d_map = torch.from_numpy(maps.astype(np.float32)).to(dev)
    x = torch.empty(2 * B, 3, 112, 112, device=dev); al = torch.empty(B, 3, 112, 112, device=dev, dtype=torch.uint8)
    t = timeit(lambda: call("lafs_ijb_align_flip_normalize", _p(src), int(offs[-1]), _p(d_off), _p(d_hw), _p(d_map), B, 112, 255.0, 1.0,
                            -0.5, _p(x), _p(al)), iters=50)
    by = int(offs[-1]) + x.numel() * 4 + al.numel()
    print(f"ijb align B={B}: {t*1e6:8.1f} us   {by/1e6:.1f} MB (whole crops counted) -> {by/t/1e12:.3f} TB/s = {by/t/8e12*100:.1f}% of 8 TB/s")
    del src, x, al
    # template pooling: skewed template sizes, as IJB's are
    w = rng.lognormal(0.0, 1.2, Tn); cnt = np.maximum(1, np.floor(w / w.sum() * (N - Tn)).astype(np.int64) + 1)
    cnt[0] += N - cnt.sum()
    tids = rng.permutation(Tn * 4)[:Tn]
    templates = np.repeat(tids, cnt)
    medias = np.concatenate([rng.randint(0, c // 3 + 1, c) for c in cnt])
    perm = rng.permutation(N); templates, medias = templates[perm], medias[perm]
    print(f"ijb templates: {Tn} of {cnt.min()}..{cnt.max()} images (median {int(np.median(cnt))})")
    feats = torch.randn(N, 2 * D, device=dev); fac = torch.rand(N, device=dev)
    t0 = time.perf_counter()
    order, ms, ts, uq = J.build_csr(templates, medias)
    t_csr = time.perf_counter() - t0
    d = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(dev)
    d_order, d_ms, d_ts = d(order), d(ms), d(ts)
    sums = torch.empty(Tn, D, device=dev); unit = torch.empty(Tn, D, device=dev, dtype=torch.float64)
    t = timeit(lambda: call("lafs_ijb_template_pool", _p(feats), 2 * D, _p(fac), N, _p(d_order), _p(d_ms), len(ms) - 1, _p(d_ts), Tn, D, 1, 1,
                            _p(sums), _p(unit)), iters=10)
    by = feats.numel() * 4 + N * 8 + Tn * D * 12
    print(f"ijb pool N={N} T={Tn} D={D}: {t*1e6:9.1f} us   {by/1e9:.2f} GB -> {by/t/1e12:.3f} TB/s = {by/t/8e12*100:.1f}% of 8 TB/s   (host CSR {t_csr:.2f} s)")
    # pair scores: random pairs, and the same pairs sorted by their first template
    i1 = rng.randint(0, Tn, P).astype(np.int32); i2 = rng.randint(0, Tn, P).astype(np.int32)
    sc = torch.empty(P, device=dev, dtype=torch.float64)
    for tag, (a, b) in (("random order", (i1, i2)), ("sorted by idx1", (np.sort(i1), i2))):
        da, db = d(a), d(b)
        t = timeit(lambda: call("lafs_ijb_pair_scores", _p(unit), Tn, D, _p(da), _p(db), P, _p(sc)), iters=5)
        print(f"ijb pairs P={P} ({tag}): {t*1e3:8.2f} ms   {P/t/1e6:.1f} M pairs/s   gathered {P*2*D*8/t/1e12:.2f} TB/s "
              f"(table {Tn*D*8/1e6:.0f} MB; 8 TB/s HBM would give {P*2*D*8/8e12*1e3:.1f} ms)")
    # the whole protocol through the public function (host CSR, H2D of the index lists, both kernels, D2H of the scores)
    p1, p2 = uq[i1], uq[i2]
    fac_h = fac.cpu().numpy()
    J.protocol(feats[:1000], fac_h[:1000], templates[:1000], medias[:1000], templates[:10], templates[10:20])
    torch.cuda.synchronize(); t0 = time.perf_counter()
    scores, _, _ = J.protocol(feats, fac_h, templates, medias, p1, p2)
    t_dev = time.perf_counter() - t0
    t0 = time.perf_counter(); fpr, tpr = J.roc_points(rng.randint(0, 2, P), scores); cells = J.tar_at_far(fpr, tpr)[2]
    t_roc = time.perf_counter() - t0
    print(f"ijb protocol wall: {t_dev:.2f} s on the device path + {t_roc:.2f} s host ROC / table ({len(fpr)} points)")
    # numpy oracle on this host: all template sums, and the pair scores of the first 1 000 000 pairs scaled to P
    fh = feats.cpu().numpy()
    t0 = time.perf_counter(); o_sums, o_uq = IO.template_sums(fh, fac_h, templates, medias); t_sum = time.perf_counter() - t0
    un = IO.unit_rows(o_sums)
    t0 = time.perf_counter(); o_sc = IO.pair_scores(un, o_uq, p1[:1000000], p2[:1000000]); t_pair = time.perf_counter() - t0
    print(f"numpy oracle on this host: template sums {t_sum:.1f} s, pair scores {t_pair:.1f} s per 1e6 pairs = {t_pair * P / 1e6:.0f} s for all "
          f"(extrapolated)   sums bit-equal to the device's: {np.array_equal(o_sums, sums.cpu().numpy())}, "
          f"scores max abs diff {float(np.abs(o_sc - scores[:1000000]).max()):.1e}")
