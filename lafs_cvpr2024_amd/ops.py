"""Tensor-level wrappers over the C ABI (torch is only the owner of device memory and streams here).

Every function launches hand-written HIP kernels from liblafs_hip.so on torch's current stream; nothing in this
module computes on the host or falls back to ATen math.
"""
import ctypes as C

import torch

from . import _lib
from ._lib import call

bf16 = torch.bfloat16


def _p(t):
    return None if t is None else C.c_void_p(t.data_ptr())


def _chk(t, dtype, name):
    if t is None:
        return
    if not t.is_cuda:
        raise _lib.LafsHipError(f"{name}: expected a device tensor (the HIP path has no CPU fallback)")
    if t.dtype != dtype:
        raise _lib.LafsHipError(f"{name}: expected dtype {dtype}, got {t.dtype}")
    if t.dim() >= 2 and t.stride(-1) != 1:
        raise _lib.LafsHipError(f"{name}: last dimension must be contiguous")


def _ld(t):
    return t.stride(0) if t.dim() >= 2 else t.numel()


def zero_(t):
    """t.zero_() as a lafs_fill_zero launch (keeps the captured step free of at::native kernels)."""
    if t.numel():
        call("lafs_fill_zero", _p(t), t.numel() * t.element_size())
    return t


def zeros(*shape, device, dtype=torch.float32):
    return zero_(torch.empty(*shape, device=device, dtype=dtype))


def gemm_nt(A, B, epilogue=_lib.EPI_BF16, bias=None, out=None, out2=None, resid=None, seq_scale=None, row2seq=None,
            aux=None, pos=None, npatch=0, splits=1, n_cols=None, out_rows=None, drop_p=0.0, drop_seed=0, act=0, skip_pre=False, drop_step=None, drop_row0=0,
            route_only=False, ctx=None):
    """out[M,N] = A[M,K] @ B[N,K]^T with a fused epilogue (see lafs_hip.h LAFS_EPI_*).  skip_pre (BF16_GELU): write only
    GELU(u), as the forward-only teacher pass does; route_only: return lafs_gemm_nt_route for this request instead of running it."""
    # 16-bit operand format: bf16 everywhere except the trainable landmark CNN's plan, which runs on fp16 (operand_f16)
    h16 = torch.float16 if A.dtype == torch.float16 else bf16
    _chk(A, h16, "A"); _chk(B, h16, "B")
    M, K = A.shape
    N = B.shape[0] if n_cols is None else n_cols
    f32_out = epilogue in (_lib.EPI_RESID_F32, _lib.EPI_F32, _lib.EPI_ATOMIC_F32, _lib.EPI_EMBED_F32)
    if out is None:
        rows = M if out_rows is None else out_rows
        out = torch.empty(rows, N, device=A.device, dtype=torch.float32 if f32_out else h16)
        if epilogue == _lib.EPI_ATOMIC_F32:
            zero_(out)
    _chk(out, torch.float32 if f32_out else h16, "out")
    if epilogue == _lib.EPI_BF16_GELU and out2 is None:
        out2 = torch.empty(M, N, device=A.device, dtype=bf16)
    a = _lib.GemmNTArgs()
    a.A, a.lda, a.B, a.ldb = A.data_ptr(), _ld(A), B.data_ptr(), _ld(B)
    a.M, a.N, a.K, a.epilogue = M, N, K, epilogue
    a.drop_p, a.drop_seed = float(drop_p), int(drop_seed) & 0xFFFFFFFF
    a.drop_step, a.drop_row0 = (drop_step.data_ptr() if drop_step is not None else None), int(drop_row0)
    a.act = int(act)
    a.operand_f16 = 1 if h16 == torch.float16 else 0
    a.C, a.ldc = out.data_ptr(), _ld(out)
    if out2 is not None:
        _chk(out2, bf16, "out2"); a.C2, a.ldc2 = out2.data_ptr(), _ld(out2)
    if bias is not None:
        _chk(bias, torch.float32, "bias"); a.bias = bias.data_ptr()
    if resid is not None:
        _chk(resid, torch.float32, "resid"); a.resid, a.ldr = resid.data_ptr(), _ld(resid)
    if seq_scale is not None:
        _chk(seq_scale, torch.float32, "seq_scale"); _chk(row2seq, torch.int32, "row2seq")
        a.seq_scale, a.row2seq = seq_scale.data_ptr(), row2seq.data_ptr()
    if aux is not None:
        _chk(aux, h16, "aux"); a.aux, a.ldaux = aux.data_ptr(), _ld(aux)
    if pos is not None:
        _chk(pos, torch.float32, "pos"); a.pos, a.npatch = pos.data_ptr(), npatch
    a.splits = splits
    a.ctx = (ctx or _lib.default_ctx(A.device)).handle
    if skip_pre and epilogue == _lib.EPI_BF16_GELU:
        a.C = None
    if route_only:
        return int(_lib.lib().lafs_gemm_nt_route(C.byref(a)))
    call("lafs_gemm_nt", C.byref(a))
    return (out, out2) if epilogue == _lib.EPI_BF16_GELU else out


def mlp_fused(X, Wa, Wb, mode, bias_a=None, bias_b=None, resid=None, seq_scale=None, row2seq=None, out=None, save_grad=None, save_act=None, ctx=None,
              ln=None, ln_stats=None, ln_out=None, ln_bwd=None, next_ln=None, proj=None):
    """The fused MLP of a ViT-S block (lafs_mlp_fused, csrc/mlp_fused.hip; vision_transformer.py:59-65,112).
    MLP_FWD / MLP_FWD_SAVE: out(f32) = resid + seq_scale[row2seq] * (gelu(X Wa^T + bias_a) Wb^T + bias_b), the saving form also
    writes save_grad = gelu'(u) and save_act = gelu(u); MLP_BWD: save_act = du = (X Wa^T) * save_grad, out(bf16) = du Wb^T."""
    _chk(Wa, bf16, "Wa"); _chk(Wb, bf16, "Wb")
    if ln is None:
        _chk(X, bf16, "X")
    else:
        X = resid                                        # ln = (gamma, beta, eps): the operand is LayerNorm(resid), formed in the kernel
    M, H = X.shape[0], Wa.shape[0]
    fwd = mode != _lib.MLP_BWD
    if out is None:
        out = torch.empty(M, X.shape[1], device=X.device, dtype=torch.float32 if fwd else bf16)
    _chk(out, torch.float32 if fwd else bf16, "out")
    if mode == _lib.MLP_FWD_SAVE and save_grad is None:
        save_grad = torch.empty(M, H, device=X.device, dtype=bf16)
    if mode != _lib.MLP_FWD and save_act is None:
        save_act = torch.empty(M, H, device=X.device, dtype=bf16)
    a = _lib.MlpArgs()
    a.X, a.ldx, a.Wa, a.ldwa, a.Wb, a.ldwb = (X.data_ptr() if ln is None else None), _ld(X), Wa.data_ptr(), _ld(Wa), Wb.data_ptr(), _ld(Wb)
    a.M, a.H, a.mode = M, H, int(mode)
    if ln is not None:
        _chk(ln[0], torch.float32, "ln gamma"); _chk(ln[1], torch.float32, "ln beta")
        a.ln_gamma, a.ln_beta, a.ln_eps = ln[0].data_ptr(), ln[1].data_ptr(), float(ln[2])
        if ln_stats is not None:
            _chk(ln_stats, torch.float32, "ln_stats"); a.ln_stats = ln_stats.data_ptr()
        if ln_out is not None:
            _chk(ln_out, bf16, "ln_out"); a.ln_out, a.ldln = ln_out.data_ptr(), _ld(ln_out)
    if bias_a is not None:
        _chk(bias_a, torch.float32, "bias_a"); a.bias_a = bias_a.data_ptr()
    if bias_b is not None:
        _chk(bias_b, torch.float32, "bias_b"); a.bias_b = bias_b.data_ptr()
    if resid is not None:
        _chk(resid, torch.float32, "resid"); a.resid, a.ldr = resid.data_ptr(), _ld(resid)
    if seq_scale is not None:
        _chk(seq_scale, torch.float32, "seq_scale"); _chk(row2seq, torch.int32, "row2seq")
        a.seq_scale, a.row2seq = seq_scale.data_ptr(), row2seq.data_ptr()
    a.out, a.ldo = out.data_ptr(), _ld(out)
    if save_grad is not None:
        _chk(save_grad, bf16, "save_grad"); a.save_grad, a.ldsg = save_grad.data_ptr(), _ld(save_grad)
    if save_act is not None:
        _chk(save_act, bf16, "save_act"); a.save_act, a.ldsa = save_act.data_ptr(), _ld(save_act)
    if next_ln is not None:                              # forward modes: (gamma, beta, eps, out bf16, stats or None) -- the next block's LayerNorm 1
        ng, nb, ne, no_, ns = next_ln
        _chk(ng, torch.float32, "next gamma"); _chk(nb, torch.float32, "next beta"); _chk(no_, bf16, "next_ln out")
        a.next_ln_gamma, a.next_ln_beta, a.next_ln_eps, a.next_ln_out, a.ldnln_next = ng.data_ptr(), nb.data_ptr(), float(ne), no_.data_ptr(), _ld(no_)
        if ns is not None:
            _chk(ns, torch.float32, "next_ln stats"); a.next_ln_stats = ns.data_ptr()
    if proj is not None:                                 # forward modes with ln: (o bf16, Wp bf16 [384, 384], bias or None, resid0 f32, scale or None) -- resid is WRITTEN
        po, pw, pb, pr, ps = proj
        _chk(po, bf16, "proj o"); _chk(pw, bf16, "proj W"); _chk(pr, torch.float32, "proj resid")
        a.proj_x, a.ldpx, a.proj_w, a.ldpw, a.proj_resid, a.ldpr = po.data_ptr(), _ld(po), pw.data_ptr(), _ld(pw), pr.data_ptr(), _ld(pr)
        if pb is not None:
            _chk(pb, torch.float32, "proj bias"); a.proj_bias = pb.data_ptr()
        if ps is not None:
            _chk(ps, torch.float32, "proj scale"); a.proj_scale = ps.data_ptr()
    if ln_bwd is not None:                               # MLP_BWD: (x, stats, gamma, g_io, gb_out, part_out) -- LayerNorm backward in the epilogue
        x_, st_, gam_, gio_, gbo_, part_ = ln_bwd
        _chk(x_, torch.float32, "x"); _chk(st_, torch.float32, "stats"); _chk(gam_, torch.float32, "gamma"); _chk(gio_, torch.float32, "g_io")
        _chk(gbo_, bf16, "gb_out"); _chk(part_, torch.float32, "part_out")
        a.resid, a.ldr, a.ln_stats, a.ln_gamma = x_.data_ptr(), _ld(x_), st_.data_ptr(), gam_.data_ptr()
        a.ln_g_io, a.ldgio, a.ln_gb_out, a.ldgb, a.ln_part_out = gio_.data_ptr(), _ld(gio_), gbo_.data_ptr(), _ld(gbo_), part_.data_ptr()
    a.ctx = (ctx or _lib.default_ctx(X.device)).handle
    call("lafs_mlp_fused", C.byref(a))
    return out, save_grad, save_act


def gemm_tn_acc(A, B, Cacc, splits=0, colsum=None):
    """Cacc[N1,N2] (f32) += A[M,N1]^T @ B[M,N2]; optional colsum[N1] (f32) += column sums of A (bias gradient)."""
    _chk(A, bf16, "A"); _chk(B, bf16, "B"); _chk(Cacc, torch.float32, "C")
    M, N1 = A.shape
    N2 = B.shape[1]
    call("lafs_gemm_tn_acc", _p(A), _ld(A), _p(B), _ld(B), _p(Cacc), _ld(Cacc), M, N1, N2, splits, _p(colsum))
    return Cacc


def wgrad_workspace(M, N1, N2, device):
    n = int(_lib.lib().lafs_wgrad_workspace_bytes(M, N1, N2))
    if n < 0:
        raise _lib.LafsHipError("lafs_wgrad_workspace_bytes: bad shape")
    return torch.empty(max(n, 16) // 4, device=device, dtype=torch.float32)


def wgrad(A, B, C, accumulate=True, colsum=None, workspace=None):
    """C[N1,N2] (f32) = (accumulate ? C : 0) + A[M,N1]^T @ B[M,N2] on the wide-tile kernel (csrc/wgrad.hip)."""
    h16 = torch.float16 if A.dtype == torch.float16 else bf16
    _chk(A, h16, "A"); _chk(B, h16, "B"); _chk(C, torch.float32, "C")
    M, N1 = A.shape
    N2 = B.shape[1]
    if workspace is None:
        workspace = wgrad_workspace(M, N1, N2, A.device)
    call("lafs_wgrad_f16" if h16 == torch.float16 else "lafs_wgrad", _p(A), _ld(A), _p(B), _ld(B), _p(C), _ld(C), M, N1, N2, int(bool(accumulate)), _p(colsum),
         _p(workspace), workspace.numel() * workspace.element_size())
    return C


def _wgrad_items(problems):
    items = (_lib.WgradItem * len(problems))()
    M = problems[0][0].shape[0]
    for it, (A, B, Cacc, accumulate, colsum) in zip(items, problems):
        _chk(A, bf16, "A"); _chk(B, bf16, "B"); _chk(Cacc, torch.float32, "C")
        if A.shape[0] != M or B.shape[0] != M:
            raise _lib.LafsHipError("wgrad_group: all GEMMs of a group share the token count M")
        it.A, it.lda, it.B, it.ldb, it.C, it.ldc = A.data_ptr(), _ld(A), B.data_ptr(), _ld(B), Cacc.data_ptr(), _ld(Cacc)
        it.N1, it.N2, it.accumulate = A.shape[1], B.shape[1], int(bool(accumulate))
        it.colsum_a = None if colsum is None else colsum.data_ptr()
    return items, M


def wgrad_group(problems, workspace=None, max_workgroups=0):
    """problems: list of (A[M,N1] bf16, B[M,N2] bf16, C[N1,N2] f32, accumulate, colsum or None); one launch + one fold."""
    items, M = _wgrad_items(problems)
    if workspace is None:
        n = int(_lib.lib().lafs_wgrad_group_workspace_bytes(items, len(problems), M, max_workgroups))
        workspace = torch.empty(max(n, 16) // 4, device=problems[0][0].device, dtype=torch.float32)
    call("lafs_wgrad_group", items, len(problems), M, max_workgroups, _p(workspace), workspace.numel() * workspace.element_size())
    return workspace


def gemm_tn_part(A, B, part, splits=0, colsum=None):
    """part[x] += (A^T @ B restricted to the rows handled by XCD x); part f32 [N_XCD, N1, N2] (zero-initialised)."""
    _chk(A, bf16, "A"); _chk(B, bf16, "B"); _chk(part, torch.float32, "part")
    M, N1 = A.shape
    N2 = B.shape[1]
    call("lafs_gemm_tn_part", _p(A), _ld(A), _p(B), _ld(B), _p(part), part.stride(1), part.stride(0), M, N1, N2, splits, _p(colsum))
    return part


def reduce_partials(part, out):
    """out += part.sum(0); part = 0."""
    call("lafs_reduce_partials", _p(part), part.stride(0), part.shape[0], out.numel(), _p(out))
    return out


def colsum_bf16_acc(X, out):
    _chk(X, bf16, "X"); _chk(out, torch.float32, "out")
    call("lafs_colsum_bf16_acc", _p(X), _ld(X), X.shape[0], X.shape[1], _p(out))
    return out


def layernorm_fwd(x, gamma, beta, eps, want_bf16=True, want_f32=False):
    _chk(x, torch.float32, "x")
    rows, D = x.shape
    y = torch.empty(rows, D, device=x.device, dtype=bf16) if want_bf16 else None
    yf = torch.empty(rows, D, device=x.device, dtype=torch.float32) if want_f32 else None
    stats = torch.empty(rows, 2, device=x.device, dtype=torch.float32)
    call("lafs_layernorm_fwd", _p(x), _ld(x), _p(gamma), _p(beta), eps, _p(y), D, _p(yf), D, _p(stats), rows, D)
    return y, yf, stats


def layernorm_bwd(dy, x, stats, gamma, g_io, dgamma, dbeta, accumulate=True, gb_out=None, seq_scale=None, row2seq=None,
                  drop_p=0.0, drop_seed=0, drop_step=None, drop_row0=0):
    """dy: bf16 or f32 [rows, D].  g_io (f32) receives (accumulates) dx; returns g_io.  dgamma / dbeta += the parameter gradients,
    deterministically: the launch stores per-workgroup sums (part_out) and lafs_layernorm_bwd_fold adds them in a fixed order."""
    rows, D = x.shape
    dy_b = dy if dy.dtype == bf16 else None
    dy_f = dy if dy.dtype == torch.float32 else None
    n_parts = int(_lib.lib().lafs_layernorm_bwd_parts(rows, D))
    part = torch.empty(n_parts * 2 * D, device=x.device, dtype=torch.float32)
    call("lafs_layernorm_bwd", _p(dy_b), D if dy_b is None else _ld(dy_b), _p(dy_f), D if dy_f is None else _ld(dy_f),
         _p(x), _ld(x), _p(stats), _p(gamma), _p(g_io), _ld(g_io), 1 if accumulate else 0,
         _p(gb_out), D if gb_out is None else _ld(gb_out), _p(seq_scale), _p(row2seq), _p(dgamma), _p(dbeta), rows, D,
         float(drop_p), int(drop_seed) & 0xFFFFFFFF, _p(drop_step), int(drop_row0), _p(part))
    item = (_lib.LnFoldItem * 1)()
    item[0].part[0], item[0].n_parts[0] = part.data_ptr(), n_parts
    item[0].dgamma, item[0].dbeta = dgamma.data_ptr(), dbeta.data_ptr()
    call("lafs_layernorm_bwd_fold", item, 1, D)
    return g_io


def scale_cast_bf16(g, seq_scale=None, row2seq=None, out=None, drop_p=0.0, drop_seed=0, drop_step=None, drop_row0=0):
    rows, D = g.shape
    if out is None:
        out = torch.empty(rows, D, device=g.device, dtype=bf16)
    call("lafs_scale_cast_bf16", _p(g), _ld(g), _p(out), _ld(out), _p(seq_scale), _p(row2seq), rows, D,
         float(drop_p), int(drop_seed) & 0xFFFFFFFF, _p(drop_step), int(drop_row0))
    return out


def dropout_mask(rows, cols, p, seed, device="cuda"):
    """The factor matrix (0 or 1/(1-p)) the kernels apply for (seed, rows x cols) -- test/debug helper."""
    out = torch.empty(rows, cols, device=device, dtype=torch.float32)
    call("lafs_debug_dropout_mask", rows, cols, float(p), int(seed) & 0xFFFFFFFF, _p(out))
    return out


def attention_fwd(qkv, cu_seqlens, max_len, heads, scale):
    _chk(qkv, bf16, "qkv"); _chk(cu_seqlens, torch.int32, "cu_seqlens")
    T = qkv.shape[0]
    inner = heads * 64
    out = torch.empty(T, inner, device=qkv.device, dtype=bf16)
    lse = torch.empty(T, heads, device=qkv.device, dtype=torch.float32)
    call("lafs_attention_fwd", _p(qkv), _ld(qkv), _p(cu_seqlens), cu_seqlens.numel() - 1, max_len, heads, scale,
         _p(out), inner, _p(lse))
    return out, lse


def attention_bwd(qkv, out, dout, lse, cu_seqlens, max_len, heads, scale):
    _chk(dout, bf16, "dout")
    dqkv = torch.empty_like(qkv)
    call("lafs_attention_bwd", _p(qkv), _ld(qkv), _p(out), _ld(out), _p(dout), _ld(dout), _p(lse),
         _p(cu_seqlens), cu_seqlens.numel() - 1, max_len, heads, scale, _p(dqkv), _ld(dqkv))
    return dqkv


def attention_probs(qkv, cu_seqlens, max_len, heads, scale, q_rows=0):
    """softmax(scale q k^T) itself, f32 [n_seq, heads, nq, max_len] with nq = q_rows or max_len (lafs_attention_probs): what
    attention_fwd used, for inspection.  Padding rows / columns of shorter sequences are zeros."""
    _chk(qkv, bf16, "qkv"); _chk(cu_seqlens, torch.int32, "cu_seqlens")
    n_seq = cu_seqlens.numel() - 1
    nq = q_rows if q_rows > 0 else max_len
    # (a bad argument is the entry point's to refuse, with its reason: the buffer only has to exist)
    probs = torch.empty(max(n_seq, 1), max(heads, 1), max(nq, 1), max(max_len, 1), device=qkv.device, dtype=torch.float32)
    call("lafs_attention_probs", _p(qkv), _ld(qkv), _p(cu_seqlens), n_seq, max_len, heads, scale, q_rows, _p(probs))
    return probs


def patchify(img, order=_lib.PATCH_ORDER_CHW):
    _chk(img, torch.float32, "img")
    B, _, S, _ = img.shape
    out = torch.empty(B * (S // 8) ** 2, 192, device=img.device, dtype=bf16)
    call("lafs_patchify", _p(img.contiguous()), B, S, order, _p(out))
    return out


def unfold_windows(S, k, stride, pad):
    """Windows per side of nn.Unfold(kernel_size=k, stride=stride, padding=pad) on an S x S image."""
    return (S + 2 * pad - k) // stride + 1


def unfold_ld(k):
    """Row stride of the window vectors: 3 k^2 rounded up to the K granule (32) of lafs_gemm_nt."""
    return (3 * k * k + 31) // 32 * 32


def unfold(img, k, stride, pad, out=None, ldp=None):
    """nn.Unfold + transpose as bf16 rows [B n n, ldp] (lafs_unfold_bf16); columns >= 3 k^2 are zero."""
    _chk(img, torch.float32, "img")
    B, _, S, _ = img.shape
    n = unfold_windows(S, k, stride, pad)
    ldp = unfold_ld(k) if ldp is None else ldp
    if out is None:
        out = torch.empty(B * max(n, 0) ** 2, ldp, device=img.device, dtype=bf16)
    call("lafs_unfold_bf16", _p(img.contiguous()), B, S, k, stride, pad, _p(out), ldp)
    return out


def fold(dpatches, B, S, k, stride, pad):
    """The adjoint of `unfold` on f32 rows [B n n, ld] -> f32 [B, 3, S, S] (lafs_fold_f32: gather form, deterministic)."""
    _chk(dpatches, torch.float32, "dpatches")
    out = torch.empty(B, 3, S, S, device=dpatches.device, dtype=torch.float32)
    call("lafs_fold_f32", _p(dpatches), _ld(dpatches), B, S, k, stride, pad, _p(out))
    return out


def pad_cast_bf16(src, ldd):
    """f32 [rows, cols] -> bf16 [rows, ldd] with a zero tail (lafs_pad_cast_bf16)."""
    _chk(src, torch.float32, "src")
    rows, cols = src.shape
    out = torch.empty(rows, ldd, device=src.device, dtype=bf16)
    call("lafs_pad_cast_bf16", _p(src), _ld(src), rows, cols, _p(out), ldd)
    return out


def add_cols(src, dst, accumulate=True):
    """dst[:, :cols] (+)= src[:, :cols], cols = dst.shape[1] (lafs_add_cols_f32)."""
    _chk(src, torch.float32, "src"); _chk(dst, torch.float32, "dst")
    rows, cols = dst.shape
    call("lafs_add_cols_f32", _p(src), _ld(src), rows, cols, _p(dst), _ld(dst), 1 if accumulate else 0)
    return dst


def bn1d_fwd(x, gamma, beta, eps, momentum, training, running_mean, running_var):
    """nn.BatchNorm1d on f32 [n, D] (lafs_bn1d_fwd).  Returns (y, save_mean, save_rstd); training updates the running buffers in place."""
    _chk(x, torch.float32, "x")
    n, D = x.shape
    y = torch.empty(n, D, device=x.device, dtype=torch.float32)
    mean = torch.empty(D, device=x.device, dtype=torch.float32)
    rstd = torch.empty(D, device=x.device, dtype=torch.float32)
    call("lafs_bn1d_fwd", _p(x), _ld(x), n, D, _p(gamma), _p(beta), float(eps), float(momentum), 1 if training else 0,
         _p(running_mean), _p(running_var), _p(y), D, _p(mean), _p(rstd))
    return y, mean, rstd


def bn1d_bwd(dy, x, mean, rstd, gamma, training, dgamma, dbeta, accumulate=True):
    """Backward of bn1d_fwd (lafs_bn1d_bwd): returns dx; dgamma / dbeta are accumulated into or overwritten."""
    _chk(dy, torch.float32, "dy"); _chk(x, torch.float32, "x")
    n, D = x.shape
    dx = torch.empty(n, D, device=x.device, dtype=torch.float32)
    call("lafs_bn1d_bwd", _p(dy), _ld(dy), _p(x), _ld(x), n, D, _p(mean), _p(rstd), _p(gamma), 1 if training else 0, _p(dx), D,
         _p(dgamma), _p(dbeta), 1 if accumulate else 0)
    return dx


def bn1d_gelu_fwd(u, gamma, beta, eps, momentum, training, running_mean, running_var, out=None):
    """a = bf16(gelu(BatchNorm1d(u))) on f32 [n, D] (lafs_bn1d_gelu_fwd; the BatchNorm output is never stored).  Returns
    (a bf16 [n, D], save_mean, save_rstd); training updates the running buffers in place.  `out`: a bf16 [n, D] view to write into."""
    _chk(u, torch.float32, "u")
    n, D = u.shape
    a = out if out is not None else torch.empty(n, D, device=u.device, dtype=bf16)
    _chk(a, bf16, "out")
    if a.shape != u.shape:
        raise _lib.LafsHipError(f"bn1d_gelu_fwd: out {tuple(a.shape)} for u {tuple(u.shape)}")
    mean = torch.empty(D, device=u.device, dtype=torch.float32)
    rstd = torch.empty(D, device=u.device, dtype=torch.float32)
    call("lafs_bn1d_gelu_fwd", _p(u), _ld(u), n, D, _p(gamma), _p(beta), float(eps), float(momentum), 1 if training else 0,
         _p(running_mean), _p(running_var), _p(a), _ld(a), _p(mean), _p(rstd))
    return a, mean, rstd


def bn1d_gelu_bwd(da, u, mean, rstd, gamma, beta, training, dgamma, dbeta, accumulate=True, out=None):
    """Backward of bn1d_gelu_fwd (lafs_bn1d_gelu_bwd): da f32 [n, D] is the gradient of a; returns du bf16 [n, D] (written into `out`
    when given); dgamma / dbeta are accumulated into or overwritten."""
    _chk(da, torch.float32, "da"); _chk(u, torch.float32, "u")
    n, D = u.shape
    if da.shape != u.shape:
        raise _lib.LafsHipError(f"bn1d_gelu_bwd: da {tuple(da.shape)} for u {tuple(u.shape)}")
    du = out if out is not None else torch.empty(n, D, device=u.device, dtype=bf16)
    _chk(du, bf16, "out")
    if du.shape != u.shape:
        raise _lib.LafsHipError(f"bn1d_gelu_bwd: out {tuple(du.shape)} for u {tuple(u.shape)}")
    call("lafs_bn1d_gelu_bwd", _p(da), _ld(da), _p(u), _ld(u), n, D, _p(mean), _p(rstd), _p(gamma), _p(beta), 1 if training else 0,
         _p(du), _ld(du), _p(dgamma), _p(dbeta), 1 if accumulate else 0)
    return du


def _group_rows(group_rows):
    """Host row table of the grouped BatchNorm entry points as a C int array (the entry point validates it)."""
    rows = [int(r) for r in group_rows]
    return (C.c_int * max(len(rows), 1))(*rows), len(rows) - 1


def bn1d_groups_fwd(x, group_rows, gamma, beta, eps, momentum, training, running_mean, running_var, out=None):
    """nn.BatchNorm1d on each row range [group_rows[g], group_rows[g + 1]) of f32 [n, D], in group order, one launch
    (lafs_bn1d_groups_fwd).  Returns (y, save_mean [G, D], save_rstd [G, D]); training updates the running buffers once per group.
    out: f32 [n, D] view to write y into (any row stride >= D)."""
    _chk(x, torch.float32, "x")
    n, D = x.shape
    tab, G = _group_rows(group_rows)
    if G >= 1 and tab[G] != n:
        raise _lib.LafsHipError(f"bn1d_groups_fwd: the row table ends at {tab[G]}, x has {n} rows")
    y = torch.empty(n, D, device=x.device, dtype=torch.float32) if out is None else out
    _chk(y, torch.float32, "out")
    if tuple(y.shape) != (n, D):
        raise _lib.LafsHipError(f"bn1d_groups_fwd: out {tuple(y.shape)} for x {tuple(x.shape)}")
    mean = torch.empty(max(G, 1), D, device=x.device, dtype=torch.float32)
    rstd = torch.empty(max(G, 1), D, device=x.device, dtype=torch.float32)
    call("lafs_bn1d_groups_fwd", _p(x), _ld(x), tab, G, D, _p(gamma), _p(beta), float(eps), float(momentum), 1 if training else 0,
         _p(running_mean), _p(running_var), _p(y), _ld(y), _p(mean), _p(rstd))
    return y, mean, rstd


def bn1d_groups_bwd(dy, x, group_rows, mean, rstd, gamma, training, dgamma, dbeta, accumulate=True, out=None):
    """Backward of bn1d_groups_fwd (lafs_bn1d_groups_bwd): returns dx (written into `out` when given); dgamma / dbeta take the groups'
    sums in group order."""
    _chk(dy, torch.float32, "dy"); _chk(x, torch.float32, "x")
    n, D = x.shape
    tab, G = _group_rows(group_rows)
    if G >= 1 and (tab[G] != n or dy.shape[0] != n or mean.shape[0] != G or rstd.shape[0] != G):
        raise _lib.LafsHipError(f"bn1d_groups_bwd: row table ending at {tab[G]} / {G} groups against x {tuple(x.shape)}, "
                                f"dy {tuple(dy.shape)}, statistics {tuple(mean.shape)}")
    dx = torch.empty(n, D, device=x.device, dtype=torch.float32) if out is None else out
    _chk(dx, torch.float32, "out")
    if tuple(dx.shape) != (n, D):
        raise _lib.LafsHipError(f"bn1d_groups_bwd: out {tuple(dx.shape)} for x {tuple(x.shape)}")
    call("lafs_bn1d_groups_bwd", _p(dy), _ld(dy), _p(x), _ld(x), tab, G, D, _p(mean), _p(rstd), _p(gamma), 1 if training else 0, _p(dx),
         _ld(dx),
         _p(dgamma), _p(dbeta), 1 if accumulate else 0)
    return dx


def _group_totals(group_total, G):
    tot = [int(v) for v in group_total]
    if len(tot) != G:
        raise _lib.LafsHipError(f"{len(tot)} total row counts for {G} groups")
    return (C.c_int * max(G, 1))(*tot)


def bn1d_groups_stats(x, group_rows, out=None):
    """This rank's partial statistics of the grouped BatchNorm1d head (lafs_bn1d_groups_stats): f32 [G, 1 + 2 D], per group
    {count, mean[D], M2[D]}.  out: contiguous f32 view of that shape (this rank's slot of the exchange buffer)."""
    _chk(x, torch.float32, "x")
    n, D = x.shape
    tab, G = _group_rows(group_rows)
    if G >= 1 and tab[G] != n:
        raise _lib.LafsHipError(f"bn1d_groups_stats: the row table ends at {tab[G]}, x has {n} rows")
    part = torch.empty(max(G, 1), 1 + 2 * D, device=x.device, dtype=torch.float32) if out is None else out
    _chk(part, torch.float32, "out")
    if tuple(part.shape) != (max(G, 1), 1 + 2 * D) or not part.is_contiguous():
        raise _lib.LafsHipError(f"bn1d_groups_stats: out {tuple(part.shape)} must be a contiguous [{G}, {1 + 2 * D}]")
    call("lafs_bn1d_groups_stats", _p(x), _ld(x), tab, G, D, _p(part))
    return part


def bn1d_groups_sync_fwd(x, group_rows, group_total, partials, gamma, beta, eps, momentum, running_mean, running_var, out=None):
    """Training forward of the grouped head with the statistics of all ranks (lafs_bn1d_groups_sync_fwd).  partials: f32 [W, G, 1 + 2 D]
    (the ranks' bn1d_groups_stats results, rank-major; any stride between the ranks, each rank's partial contiguous); group_total:
    the groups' row counts over all ranks.  Returns (y, save_mean [G, D], save_rstd [G, D]); the running buffers are updated once per
    group with the unbiased variance of the total count."""
    _chk(x, torch.float32, "x"); _chk(partials, torch.float32, "partials")
    n, D = x.shape
    tab, G = _group_rows(group_rows)
    if G >= 1 and tab[G] != n:
        raise _lib.LafsHipError(f"bn1d_groups_sync_fwd: the row table ends at {tab[G]}, x has {n} rows")
    if partials.dim() != 3 or tuple(partials.shape[1:]) != (G, 1 + 2 * D) or partials.stride(2) != 1 or partials.stride(1) != 1 + 2 * D:
        raise _lib.LafsHipError(f"bn1d_groups_sync_fwd: partials {tuple(partials.shape)} / strides {partials.stride()} for "
                                f"[W, {G}, {1 + 2 * D}] with contiguous rank slots")
    W = partials.shape[0]
    y = torch.empty(n, D, device=x.device, dtype=torch.float32) if out is None else out
    _chk(y, torch.float32, "out")
    if tuple(y.shape) != (n, D):
        raise _lib.LafsHipError(f"bn1d_groups_sync_fwd: out {tuple(y.shape)} for x {tuple(x.shape)}")
    mean = torch.empty(max(G, 1), D, device=x.device, dtype=torch.float32)
    rstd = torch.empty(max(G, 1), D, device=x.device, dtype=torch.float32)
    call("lafs_bn1d_groups_sync_fwd", _p(x), _ld(x), tab, _group_totals(group_total, G), G, D, _p(partials), W,
         partials.stride(0) if W > 1 else G * (1 + 2 * D), _p(gamma), _p(beta), float(eps), float(momentum), _p(running_mean),
         _p(running_var), _p(y), _ld(y), _p(mean), _p(rstd))
    return y, mean, rstd


def bn1d_groups_bwd_sums(dy, x, group_rows, mean, rstd, dgamma, dbeta, accumulate=True, out=None):
    """First half of the cross-rank backward (lafs_bn1d_groups_bwd_sums): returns sums f32 [G, 2 D] = {sum dy, sum dy xhat} over this
    rank's rows per group; dgamma / dbeta take the groups' sums in group order (rank-local)."""
    _chk(dy, torch.float32, "dy"); _chk(x, torch.float32, "x")
    n, D = x.shape
    tab, G = _group_rows(group_rows)
    if G >= 1 and (tab[G] != n or dy.shape[0] != n or mean.shape[0] != G or rstd.shape[0] != G):
        raise _lib.LafsHipError(f"bn1d_groups_bwd_sums: row table ending at {tab[G]} / {G} groups against x {tuple(x.shape)}, "
                                f"dy {tuple(dy.shape)}, statistics {tuple(mean.shape)}")
    sums = torch.empty(max(G, 1), 2 * D, device=x.device, dtype=torch.float32) if out is None else out
    _chk(sums, torch.float32, "out")
    if tuple(sums.shape) != (max(G, 1), 2 * D) or not sums.is_contiguous():
        raise _lib.LafsHipError(f"bn1d_groups_bwd_sums: out {tuple(sums.shape)} must be a contiguous [{G}, {2 * D}]")
    call("lafs_bn1d_groups_bwd_sums", _p(dy), _ld(dy), _p(x), _ld(x), tab, G, D, _p(mean), _p(rstd), _p(sums), _p(dgamma), _p(dbeta),
         1 if accumulate else 0)
    return sums


def bn1d_groups_sync_bwd(dy, x, group_rows, group_total, mean, rstd, gamma, sums, out=None):
    """Second half (lafs_bn1d_groups_sync_bwd): dx of this rank's rows from the sums of ALL ranks (f32 [G, 2 D], already added up) and
    the groups' total row counts."""
    _chk(dy, torch.float32, "dy"); _chk(x, torch.float32, "x"); _chk(sums, torch.float32, "sums")
    n, D = x.shape
    tab, G = _group_rows(group_rows)
    if G >= 1 and (tab[G] != n or dy.shape[0] != n or mean.shape[0] != G or rstd.shape[0] != G or tuple(sums.shape) != (G, 2 * D)
                   or not sums.is_contiguous()):
        raise _lib.LafsHipError(f"bn1d_groups_sync_bwd: row table ending at {tab[G]} / {G} groups against x {tuple(x.shape)}, "
                                f"dy {tuple(dy.shape)}, statistics {tuple(mean.shape)}, sums {tuple(sums.shape)}")
    dx = torch.empty(n, D, device=x.device, dtype=torch.float32) if out is None else out
    _chk(dx, torch.float32, "out")
    if tuple(dx.shape) != (n, D):
        raise _lib.LafsHipError(f"bn1d_groups_sync_bwd: out {tuple(dx.shape)} for x {tuple(x.shape)}")
    call("lafs_bn1d_groups_sync_bwd", _p(dy), _ld(dy), _p(x), _ld(x), tab, _group_totals(group_total, G), G, D, _p(mean), _p(rstd),
         _p(gamma), _p(sums), _p(dx), _ld(dx))
    return dx


def dino_head_loss(zn_s, zn_t, wn_s, wn_t, center, ncrops, K, student_temp, teacher_temp, grad, loss=None, colsum=None, ws=None,
                   dev_temps=None, grad_scale=1.0):
    """DINOHead's last layer of both networks + DINO loss + centre row sums with the logits never stored (csrc/dino_head_loss.hip).
    zn_*: bf16 [rows, 256], wn_*: bf16 [Kpad, 256]; grad: bf16 [ncrops B, >= Kpad] (written); returns (loss[1], grad)."""
    for t, n in ((zn_s, "zn_s"), (zn_t, "zn_t"), (wn_s, "wn_s"), (wn_t, "wn_t"), (grad, "grad")):
        _chk(t, bf16, n)
    rows, B = zn_s.shape[0], zn_t.shape[0] // 2
    if rows != ncrops * B or zn_s.shape[1] != zn_t.shape[1] or wn_s.shape != wn_t.shape or not zn_s.is_contiguous() or not wn_s.is_contiguous() \
            or not zn_t.is_contiguous() or not wn_t.is_contiguous():
        raise _lib.LafsHipError("dino_head_loss: student rows = ncrops * B, teacher rows = 2 * B, contiguous operands of equal widths")
    if ws is None:
        ws = torch.empty(_lib.lib().lafs_dino_head_loss_workspace(ncrops, B, K), device=zn_s.device, dtype=torch.float32)
    if loss is None:
        loss = torch.empty(1, device=zn_s.device, dtype=torch.float32)
    call("lafs_dino_head_loss", _p(zn_s), _p(zn_t), _p(wn_s), _p(wn_t), zn_s.shape[1], _p(center), ncrops, B, K, wn_s.shape[0],
         student_temp, teacher_temp, _p(dev_temps), _p(loss), _p(grad), _ld(grad), grad_scale, _p(colsum), _p(ws))
    return loss, grad


def dino_loss_fwd_bwd(student, teacher, center, ncrops, student_temp, teacher_temp, K=None, grad=None, grad_bf16=True,
                      grad_scale=1.0, ws=None, loss=None, dev_temps=None):
    """Returns (loss[1] f32, grad [rows, ld] bf16|f32).  student/teacher may be padded (ld >= K)."""
    _chk(student, torch.float32, "student"); _chk(teacher, torch.float32, "teacher")
    rows, ld = student.shape[0], _ld(student)
    K = student.shape[1] if K is None else K
    B = rows // ncrops
    if ws is None:
        ws = torch.empty(_lib.lib().lafs_dino_loss_workspace(ncrops, B, K), device=student.device, dtype=torch.float32)
    if loss is None:
        loss = torch.empty(1, device=student.device, dtype=torch.float32)
    if grad is None:
        grad = torch.zeros(rows, ld, device=student.device, dtype=bf16 if grad_bf16 else torch.float32)
    call("lafs_dino_loss_fwd_bwd", _p(student), _p(teacher), ld, _p(center), ncrops, B, K, student_temp, teacher_temp,
         _p(loss), _p(grad), _ld(grad), 1 if grad.dtype == bf16 else 0, grad_scale, _p(ws), _p(dev_temps))
    return loss, grad


def landmark_mse(pred, label, weight, grad_scale=1.0, loss_land=None, loss=None, dtheta=None):
    """lafs_landmark_mse: pred, label f32 [B, n, 2]; weight: a one-element f32 DEVICE tensor, read when the kernel runs.
    -> loss_land f32 [1] (the unweighted mean); `loss` [1] and `dtheta` [B, n, 2], when given, are accumulated into."""
    for t, name in ((pred, "pred"), (label, "label"), (weight, "weight"), (loss_land, "loss_land"), (loss, "loss"), (dtheta, "dtheta")):
        _chk(t, torch.float32, name)
    if pred.dim() != 3 or pred.shape[2] != 2 or label.shape != pred.shape or (dtheta is not None and dtheta.shape != pred.shape):
        raise _lib.LafsHipError("landmark_mse: pred, label (and dtheta) are [B, n, 2]")
    if not (pred.is_contiguous() and label.is_contiguous() and (dtheta is None or dtheta.is_contiguous())):
        raise _lib.LafsHipError("landmark_mse: contiguous operands expected")
    if loss_land is None:
        loss_land = torch.empty(1, device=pred.device, dtype=torch.float32)
    call("lafs_landmark_mse", _p(pred), _p(label), pred.shape[0], pred.shape[1], _p(weight), float(grad_scale), _p(loss_land), _p(loss),
         _p(dtheta))
    return loss_land


def jpeg_decode(stream, images, tables, B, H, W, out=None, status=None, workspace=None):
    """One launch of lafs_jpeg_decode (csrc/jpeg.hip) over what jpeg.pack built: stream / images / tables are uint8 device tensors
    (scan bytes, B 64-byte records, 1600-byte table blocks).  Writes out u8 [B,3,H,W] and returns status i32 [B] (0 = decoded)."""
    for t, n in ((stream, "stream"), (images, "images"), (tables, "tables"), (out, "out"), (workspace, "workspace")):
        _chk(t, torch.uint8, n)
    _chk(status, torch.int32, "status")
    if not (stream.is_contiguous() and images.is_contiguous() and tables.is_contiguous()) or images.numel() != 64 * B:
        raise _lib.LafsHipError("jpeg_decode: contiguous buffers and one 64-byte record per image")
    need = _lib.lib().lafs_jpeg_workspace_bytes(B, H, W)
    if need < 0:
        raise _lib.LafsHipError(f"jpeg_decode: B={B}, H={H}, W={W} outside 1..LAFS_JPEG_MAX_DIM")
    dev = stream.device
    if out is None:
        out = torch.empty(B, 3, H, W, device=dev, dtype=torch.uint8)
    if status is None:
        status = torch.empty(B, device=dev, dtype=torch.int32)
    if workspace is None:
        workspace = torch.empty(need, device=dev, dtype=torch.uint8)
    if tuple(out.shape) != (B, 3, H, W) or not out.is_contiguous() or status.numel() != B or workspace.numel() < need:
        raise _lib.LafsHipError("jpeg_decode: out must be contiguous [B,3,H,W], status [B], workspace lafs_jpeg_workspace_bytes(B,H,W)")
    call("lafs_jpeg_decode", _p(stream), stream.numel(), _p(images), _p(tables), tables.numel(), B, H, W, _p(out), _p(status), _p(workspace))
    return status


def knn_search(bank, query, k, bank_pos0=0, exclude=None, merge=False, splits=0, top_score=None, top_idx=None):
    """lafs_knn_search: bank f32 [N, D] and query f32 [Q, D] (row strides multiples of 4, 16-byte aligned) -> (top_score f32 [Q, k],
    top_idx i32 [Q, k]): per query the first k bank positions bank_pos0 + row of the ranking order of include/lafs_hip.h.  exclude:
    i32 [Q], the position left out per query (-1: none).  merge: top_score / top_idx hold an earlier result over other positions."""
    _chk(bank, torch.float32, "bank"); _chk(query, torch.float32, "query"); _chk(exclude, torch.int32, "exclude")
    _chk(top_score, torch.float32, "top_score"); _chk(top_idx, torch.int32, "top_idx")
    if bank.dim() != 2 or query.dim() != 2 or bank.shape[1] != query.shape[1]:
        raise _lib.LafsHipError("knn_search: bank [N, D] and query [Q, D] expected")
    (N, D), Q, k = bank.shape, query.shape[0], int(k)
    if exclude is not None and (exclude.dim() != 1 or exclude.numel() != Q or not exclude.is_contiguous()):
        raise _lib.LafsHipError("knn_search: exclude must be a contiguous int32 [Q]")
    if merge and (top_score is None or top_idx is None):
        raise _lib.LafsHipError("knn_search: merge needs the earlier top_score and top_idx")
    if top_score is None:
        top_score = torch.empty(Q, k, device=bank.device, dtype=torch.float32)
    if top_idx is None:
        top_idx = torch.empty(Q, k, device=bank.device, dtype=torch.int32)
    for t in (top_score, top_idx):
        if tuple(t.shape) != (Q, k) or not t.is_contiguous():
            raise _lib.LafsHipError("knn_search: top_score and top_idx must be contiguous [Q, k]")
    need = int(_lib.lib().lafs_knn_workspace(Q, N, k, int(splits)))
    ws = torch.empty(need, device=bank.device, dtype=torch.uint8) if need else None
    call("lafs_knn_search", _p(bank), _ld(bank), N, int(bank_pos0), _p(query), _ld(query), Q, D, k, _p(exclude), 1 if merge else 0,
         int(splits), _p(top_score), _p(top_idx), _p(ws), need)
    return top_score, top_idx


def knn_vote(top_score, top_idx, bank_label, ks, temperature=0.07):
    """lafs_knn_vote: a list of knn_search + bank_label i32 [n_label] (by position) -> (pred i32, vote f32) [len(ks), Q, 5]: the five
    best classes of the exp(score / temperature)-weighted vote over the first ks[i] entries; unused slots -1 and 0."""
    _chk(top_score, torch.float32, "top_score"); _chk(top_idx, torch.int32, "top_idx"); _chk(bank_label, torch.int32, "bank_label")
    if top_score.dim() != 2 or top_idx.shape != top_score.shape or not (top_score.is_contiguous() and top_idx.is_contiguous()):
        raise _lib.LafsHipError("knn_vote: top_score and top_idx must be contiguous [Q, k]")
    if bank_label.dim() != 1 or not bank_label.is_contiguous():
        raise _lib.LafsHipError("knn_vote: bank_label must be a contiguous int32 vector")
    ks = [int(v) for v in ks]
    Q, k = top_score.shape
    pred = torch.empty(len(ks), Q, 5, device=top_score.device, dtype=torch.int32)
    vote = torch.empty(len(ks), Q, 5, device=top_score.device, dtype=torch.float32)
    call("lafs_knn_vote", _p(top_score), _p(top_idx), Q, k, _p(bank_label), bank_label.numel(), (C.c_int32 * len(ks))(*ks), len(ks),
         float(temperature), _p(pred), _p(vote))
    return pred, vote


def softmax_ce_rank_workspace(B, n_classes, device):
    n = int(_lib.lib().lafs_softmax_ce_rank_workspace_bytes(int(B), int(n_classes)))
    if n < 0:
        raise _lib.LafsHipError("lafs_softmax_ce_rank_workspace_bytes: bad shape")
    return torch.empty(n // 4, device=device, dtype=torch.float32)


def softmax_ce_rank(logits, y, n_classes=None, grad_scale=1.0, dlogits=None, row_loss=None, row_rank=None, ws=None):
    """lafs_softmax_ce_rank: logits f32 [B, >= C] (read-only) and y i32 [B] -> (row_loss f32 [B], row_rank i32 [B]) and, when
    dlogits (bf16 [B, lddl], lddl % 8 == 0) is given, dlogits = bf16(grad_scale (softmax - one-hot)) with zero pad columns.  y == -1:
    no target (loss 0, rank -1, zero gradient row); any other label outside [0, C): loss NaN, rank -2."""
    _chk(logits, torch.float32, "logits"); _chk(y, torch.int32, "y"); _chk(dlogits, bf16, "dlogits")
    _chk(row_loss, torch.float32, "row_loss"); _chk(row_rank, torch.int32, "row_rank"); _chk(ws, torch.float32, "ws")
    if logits.dim() != 2 or y.dim() != 1 or y.numel() != logits.shape[0] or not y.is_contiguous():
        raise _lib.LafsHipError("softmax_ce_rank: logits [B, C] and a contiguous y [B] expected")
    B = logits.shape[0]
    n = logits.shape[1] if n_classes is None else int(n_classes)
    if dlogits is not None and (dlogits.dim() != 2 or dlogits.shape[0] != B):
        raise _lib.LafsHipError("softmax_ce_rank: dlogits must be [B, lddl]")
    if row_loss is None:
        row_loss = torch.empty(B, device=logits.device, dtype=torch.float32)
    if row_rank is None:
        row_rank = torch.empty(B, device=logits.device, dtype=torch.int32)
    for t in (row_loss, row_rank):
        if t.dim() != 1 or t.numel() != B or not t.is_contiguous():
            raise _lib.LafsHipError("softmax_ce_rank: row_loss and row_rank must be contiguous [B]")
    need = int(_lib.lib().lafs_softmax_ce_rank_workspace_bytes(B, n))
    if ws is None:
        ws = softmax_ce_rank_workspace(B, n, logits.device)
    elif ws.numel() * 4 < need or not ws.is_contiguous():
        raise _lib.LafsHipError(f"softmax_ce_rank: the workspace holds {ws.numel() * 4} bytes, {need} are needed")
    call("lafs_softmax_ce_rank", _p(logits), _ld(logits), B, n, _p(y), float(grad_scale), _p(dlogits), 0 if dlogits is None else _ld(dlogits),
         _p(row_loss), _p(row_rank), _p(ws))
    return row_loss, row_rank


def koleo_workspace(n_groups, rows, D, device):
    n = int(_lib.lib().lafs_koleo_workspace_bytes(int(n_groups), int(rows), int(D)))
    if n < 0:
        raise _lib.LafsHipError("lafs_koleo_workspace_bytes: bad shape (n_groups >= 1, 2 <= rows <= 1024, 4 <= D <= 1024, D % 4 == 0)")
    return torch.empty(n // 4, device=device, dtype=torch.float32)


def koleo(x, n_groups, rows, *, eps=1e-8, grad_scale=1.0, dx=None, accumulate=False, loss=None, nn=None, ws=None):
    """lafs_koleo_fwd_bwd: the KoLeo regulariser of n_groups groups of `rows` rows each, x f32 [n_groups * rows, D] (read-only, row
    stride % 4 == 0) -> (loss f32 [n_groups], unscaled; nn i32 [n_groups * rows], the neighbour of every row as an index inside its
    group).  With dx (f32, the shape of x): dx = (dx if accumulate else 0) + grad_scale dL_g/dx.  With loss, nn, ws (and dx) passed
    nothing is allocated: the call is capturable."""
    _chk(x, torch.float32, "x"); _chk(dx, torch.float32, "dx"); _chk(loss, torch.float32, "loss"); _chk(nn, torch.int32, "nn")
    _chk(ws, torch.float32, "ws")
    n_groups, rows = int(n_groups), int(rows)
    if x.dim() != 2 or x.shape[0] != n_groups * rows:
        raise _lib.LafsHipError("koleo: x must be [n_groups * rows, D]")
    R, D = x.shape
    if dx is not None and (dx.dim() != 2 or tuple(dx.shape) != (R, D)):
        raise _lib.LafsHipError("koleo: dx must have the shape of x")
    need = int(_lib.lib().lafs_koleo_workspace_bytes(n_groups, rows, D))
    if need < 0:
        raise _lib.LafsHipError(f"koleo: {n_groups} groups of {rows} rows x {D} columns: n_groups >= 1, 2 <= rows <= 1024, 4 <= D <= 1024 and "
                                "D % 4 == 0 are needed")
    if loss is None:
        loss = torch.empty(n_groups, device=x.device, dtype=torch.float32)
    if nn is None:
        nn = torch.empty(R, device=x.device, dtype=torch.int32)
    if loss.dim() != 1 or loss.numel() != n_groups or not loss.is_contiguous() or nn.dim() != 1 or nn.numel() != R or not nn.is_contiguous():
        raise _lib.LafsHipError("koleo: loss must be a contiguous [n_groups], nn a contiguous [n_groups * rows]")
    if ws is None:
        ws = koleo_workspace(n_groups, rows, D, x.device)
    elif ws.numel() * 4 < need or not ws.is_contiguous():
        raise _lib.LafsHipError(f"koleo: the workspace holds {ws.numel() * 4} bytes, {need} are needed")
    call("lafs_koleo_fwd_bwd", _p(x), _ld(x), n_groups, rows, D, float(eps), float(grad_scale), _p(loss), _p(nn), _p(dx),
         0 if dx is None else _ld(dx), int(bool(accumulate)), _p(ws))
    return loss, nn
