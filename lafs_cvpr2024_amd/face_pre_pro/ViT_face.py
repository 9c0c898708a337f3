"""Drop-in surface of the reference's ``face_pre_pro/ViT_face.py`` for the symbols on the hot path
(SURVEY.md section 8b): ``CosFace``, ``AdaFace`` (named by the reference, restated from the paper), ``ViT_face_landmark_patch8`` (Part-fViT) and
``extract_patches_pytorch_gridsample`` -- same constructor / forward signatures and state_dict keys, running on the
gfx950 HIP kernels -- and for fViT, ``ViTs_face_overlap`` (the plain face transformer with released weights).  The other experiment
variants the entry points never instantiate are not provided.
"""
import math

import torch
import torch.nn as nn

from .. import _lib, functional as Fn, ops
from ..ops import _p, call
from ..vision_transformer import attach_arena

f32, bf16 = torch.float32, torch.bfloat16


# ------------------------------------------------------------------------------------------------- landmark gather
class _PatchGather(torch.autograd.Function):
    @staticmethod
    def forward(ctx, imgs, landmarks, n):
        B, _, S, _ = imgs.shape
        r = int(math.isqrt(n))
        img = imgs.contiguous().float()
        th = landmarks[:, :n].contiguous().float()
        out = torch.empty(B, 3, 8 * r, 8 * r, device=imgs.device, dtype=f32)
        call("lafs_patch_gather_fwd", _p(img), _p(th), B, S, n, _p(out))
        ctx.save_for_backward(img, th)
        ctx.n, ctx.full_n = n, landmarks.shape[1]
        return out

    @staticmethod
    def backward(ctx, dout):
        img, th = ctx.saved_tensors
        B, _, S, _ = img.shape
        dth = torch.empty_like(th)
        dimg = torch.zeros_like(img) if ctx.needs_input_grad[0] else None
        call("lafs_patch_gather_bwd", _p(img), _p(th), _p(dout.contiguous().float()), B, S, ctx.n, _p(dth), _p(dimg))
        if ctx.full_n != ctx.n:
            full = torch.zeros(B, ctx.full_n, 2, device=th.device, dtype=f32)
            full[:, :ctx.n] = dth
            dth = full
        return dimg, dth, None


def extract_patches_pytorch_gridsample(imgs, landmarks, patch_shape=None, num_landm=49):
    """8x8 bilinear patches around ``landmarks`` (x, y in pixels) assembled into a sqrt(n) x sqrt(n) mosaic
    (reference face_pre_pro/ViT_face.py:1615-1656: n sequential grid_sample calls) as ONE kernel launch,
    differentiable with respect to the landmarks and the image.  Only 8x8 patches (the LAFS configuration)."""
    if patch_shape is not None and (int(patch_shape[0]) != 8 or int(patch_shape[1]) != 8):
        raise NotImplementedError("the HIP gather kernel is specialised for 8x8 patches")
    if imgs.shape[1] != 3:
        raise NotImplementedError("3-channel images only")
    return _PatchGather.apply(imgs, landmarks, int(num_landm))


# ------------------------------------------------------------------------------------------------- margin head
def _cosine_fwd(x, weight):
    """cos(x, W) f32 [B, C]: an MFMA GEMM over row-normalised bf16 operands; the normalisations are HIP row kernels.  Returns the
    cosines and what `_cosine_bwd` needs (inv_x: 1 / ||x_b|| as lafs_l2norm_fwd writes it)."""
    B, D = x.shape
    C = weight.shape[0]
    Cpad = (C + 127) // 128 * 128
    dev = x.device
    xn = torch.empty(B, D, device=dev, dtype=bf16); inv_x = torch.empty(B, device=dev, dtype=f32)
    x32 = x.contiguous().float()
    call("lafs_l2norm_fwd", _p(x32), D, _p(xn), D, _p(inv_x), B, D)
    wn = torch.empty(Cpad, D, device=dev, dtype=bf16); inv_w = torch.empty(C, device=dev, dtype=f32)
    ones = torch.ones(C, device=dev, dtype=f32)
    w32 = weight.contiguous().float()
    call("lafs_weightnorm_fwd", _p(w32), _p(ones), C, Cpad, D, _p(wn), None, Cpad, _p(inv_w))
    cos = ops.gemm_nt(xn, wn, _lib.EPI_F32, n_cols=Cpad)[:, :C]
    return cos, (x32, w32, xn, wn, inv_x, inv_w, ones)


def _cosine_bwd(saved, dcos_f32):
    """(d x, d W) from d cos f32 [B, C] (rounded to bf16, the operand format of the two gradient GEMMs)."""
    x32, w32, xn, wn, inv_x, inv_w, ones = saved
    B, D = x32.shape
    C, Cpad = w32.shape[0], wn.shape[0]
    dev = x32.device
    dcos = torch.zeros(B, Cpad, device=dev, dtype=bf16)
    dcos[:, :C] = dcos_f32.to(bf16)
    # d(xn) = dcos @ wn  (contraction over classes -> split-K), d(wn) = dcos^T @ xn
    wn_t = wn.t().contiguous()
    dxn = ops.gemm_nt(dcos, wn_t, _lib.EPI_ATOMIC_F32, splits=max(1, min(64, Cpad // 1024)))
    dwn = torch.zeros(Cpad, D, device=dev, dtype=f32)
    ops.gemm_tn_acc(dcos, xn, dwn, splits=1)
    dx = torch.empty(B, D, device=dev, dtype=f32)
    call("lafs_l2norm_bwd", _p(x32), D, _p(dxn), D, _p(inv_x), _p(dx), D, B, D)
    dw = torch.empty(C, D, device=dev, dtype=f32)
    call("lafs_weightnorm_bwd", _p(dwn), _p(w32), _p(ones), _p(inv_w), C, D, _p(dw), None, 0)
    return dx, dw


def _dense_label(label, B, C, dev):
    if label.dim() > 1:
        return label.to(f32)
    return torch.zeros(B, C, device=dev, dtype=f32).scatter_(1, label.view(-1, 1).long(), 1.0)


class _CosFaceFunction(torch.autograd.Function):
    """s * (cos(x, W) - m * y).  (The training engine fuses margin + softmax + CE instead: lafs_margin_softmax_ce_bf16 / _mix_bf16.)"""

    @staticmethod
    def forward(ctx, x, weight, label, s, m):
        cos, saved = _cosine_fwd(x, weight)
        y = _dense_label(label, x.shape[0], weight.shape[0], x.device)
        ctx.save_for_backward(*saved)
        ctx.s = s
        return s * (cos - m * y)

    @staticmethod
    def backward(ctx, dout):
        dx, dw = _cosine_bwd(ctx.saved_tensors, dout * ctx.s)
        return dx, dw, None, None, None


class CosFace(nn.Module):
    """CosFace margin head (reference face_pre_pro/ViT_face.py:26-96): out = s * (cos(x, W) - m * label), where label is a
    class-index vector or a dense soft target (the mixup branch).  ``device_id`` must be None (the reference's
    single-process model-parallel branch is dead code: both entry points pass GPU_ID=None)."""

    def __init__(self, in_features, out_features, device_id, s=64.0, m=0.4):
        super().__init__()
        if device_id is not None:
            raise NotImplementedError("device_id model parallelism is not part of the hot path (always None in the reference)")
        if in_features % 64:
            raise NotImplementedError("in_features must be a multiple of 64 for the MFMA GEMM")
        self.in_features, self.out_features, self.device_id, self.s, self.m = in_features, out_features, device_id, s, m
        self.weight = nn.Parameter(torch.empty(out_features, in_features))
        nn.init.xavier_uniform_(self.weight)

    def forward(self, input, label):
        return _CosFaceFunction.apply(input, self.weight, label, float(self.s), float(self.m))

    def __repr__(self):
        return f"{self.__class__.__name__}(in_features = {self.in_features}, out_features = {self.out_features}, s = {self.s}, m = {self.m})"


class _AdaFaceFunction(torch.autograd.Function):
    """AdaFace logits (lafs_hip.h, lafs_margin_softmax_ce_ada_bf16) on the eager module path: the margins come from
    lafs_adaface_margins, torch element-wise operations form the logits, as _CosFaceFunction does.  The margins are detached: no
    gradient flows through the norm statistics.  (The training engine fuses margin + softmax + CE: lafs_margin_softmax_ce_ada_bf16.)"""

    @staticmethod
    def forward(ctx, x, weight, label, state, s, m, h, t_alpha, update):
        B, C = x.shape[0], weight.shape[0]
        cos, saved = _cosine_fwd(x, weight)
        rm = torch.empty(B, 2, device=x.device, dtype=f32)
        call("lafs_adaface_margins", _p(saved[4]), B, _p(state), t_alpha, h, m, int(update), _p(rm))
        tgt = _dense_label(label, B, C, x.device) > 0
        one, eps = torch.tensor(1.0, dtype=f32), torch.tensor(1e-3, dtype=f32)        # the kernels' fp32 thresholds
        lo, hi, pi_hi = float(eps - one), float(one - eps), float(torch.tensor(math.pi, dtype=f32) - eps)
        cc = cos.clamp(lo, hi)
        th = torch.acos(cc)
        tm = th + rm[:, :1]
        z = s * torch.where(tgt, torch.cos(tm.clamp(float(eps), pi_hi)) - rm[:, 1:], cc)
        live = (cos >= lo) & (cos <= hi)
        dz = torch.where(tgt, torch.where((tm >= float(eps)) & (tm <= pi_hi), torch.sin(tm) / torch.sin(th), torch.zeros_like(cos)),
                         torch.ones_like(cos))
        ctx.save_for_backward(*saved, s * dz * live)
        return z

    @staticmethod
    def backward(ctx, dout):
        dx, dw = _cosine_bwd(ctx.saved_tensors[:-1], dout * ctx.saved_tensors[-1])
        return dx, dw, None, None, None, None, None, None, None


class AdaFace(nn.Module):
    """AdaFace margin head (Kim, Jain, Liu, CVPR 2022; PARITY UNPINNED: the reference names the head, train_largescale.py:820, and ships
    no class): the margin adapts per sample to the embedding's norm, the image-quality proxy.  `weight` has CosFace's name, layout and
    initialisation; `batch_mean` / `batch_std` (f32 [1] buffers, initially 20 and 100) are the running norm statistics, updated in
    training mode only.  ``forward(input, label)``: label is a class-index vector or a dense soft target (every class of positive
    weight carries the full margin)."""

    def __init__(self, in_features, out_features, device_id, s=64.0, m=0.4, h=0.333, t_alpha=0.01):
        super().__init__()
        if device_id is not None:
            raise NotImplementedError("device_id model parallelism is not part of the hot path (always None in the reference)")
        if in_features % 64:
            raise NotImplementedError("in_features must be a multiple of 64 for the MFMA GEMM")
        self.in_features, self.out_features, self.device_id = in_features, out_features, device_id
        self.s, self.m, self.h, self.t_alpha, self.eps = s, m, h, t_alpha, 1e-3
        self.weight = nn.Parameter(torch.empty(out_features, in_features))
        nn.init.xavier_uniform_(self.weight)
        self.register_buffer("batch_mean", torch.full((1,), 20.0))
        self.register_buffer("batch_std", torch.full((1,), 100.0))

    def state_storage(self):
        """f32 [2] = (batch_mean, batch_std) on the weight's device, the `state` operand of lafs_adaface_margins.  The two buffers
        are made views of it (once per device move), so state_dict() always holds the values the kernel wrote last."""
        st = getattr(self, "_state", None)
        dev = self.weight.device
        if (st is None or st.device != dev or self.batch_mean.data_ptr() != st.data_ptr()
                or self.batch_std.data_ptr() != st.data_ptr() + 4):
            st = torch.cat([self.batch_mean.detach().to(dev, f32), self.batch_std.detach().to(dev, f32)])
            self.batch_mean, self.batch_std = st[0:1], st[1:2]
            object.__setattr__(self, "_state", st)
        return st

    def forward(self, input, label):
        return _AdaFaceFunction.apply(input, self.weight, label, self.state_storage(), float(self.s), float(self.m), float(self.h),
                                      float(self.t_alpha), self.training)

    def __repr__(self):
        return (f"{self.__class__.__name__}(in_features = {self.in_features}, out_features = {self.out_features}, s = {self.s}, "
                f"m = {self.m}, h = {self.h}, t_alpha = {self.t_alpha})")


# ------------------------------------------------------------------------------------------------- Part-fViT
class _Holder(nn.Module):
    pass


class _PartFViTFunction(torch.autograd.Function):
    @staticmethod
    def forward(ctx, model, hook, x, pos):
        save = any(ctx.needs_input_grad)
        n_img = x.shape[0]
        n = x.shape[1] if x.dim() == 3 else (x.shape[-1] // 8) ** 2
        side = 8 * int(math.isqrt(n))
        if (side // 8) ** 2 != n:
            raise _lib.LafsHipError("the packed engine needs a square number of patches per image")
        geom = Fn.geometry([(n_img, side)], x.device)
        drop = model._sample_drop_scales(geom) if model.training else None
        feat, st, _ = Fn.vit_forward(model._arena, model._spec, geom, [x.contiguous().float()], [pos.detach().contiguous()],
                                     drop, save=save, dropout=model._next_dropout())
        ctx.model, ctx.st = model, (st if save else None)
        ctx.x_dim = x.dim()
        model._last_tokens = _.view(n_img, n + 1, -1)[:, 1:] if getattr(model, "_want_tokens", False) else None
        return feat

    @staticmethod
    def backward(ctx, dfeat):
        model, st = ctx.model, ctx.st
        if not ctx.needs_input_grad[2]:
            dpos = Fn.vit_backward(model._arena, model._spec, st, dfeat)
            return None, None, None, dpos[0]
        # landmark branch: the patch vectors themselves are differentiable (reference ViT_face.py:679-711)
        dpos, dx = Fn.vit_backward(model._arena, model._spec, st, dfeat, want_dx=True)
        dx = dx[0] if ctx.x_dim == 3 else Fn.unpatchify_grad(dx[0], model._spec.patch_order)
        return None, None, dx, dpos[0]


class ViT_face_landmark_patch8(nn.Module):
    """Part-fViT (reference face_pre_pro/ViT_face.py:560-795): pre-LN ViT with bias-free qkv, attention scale dim**-0.5,
    ``heads * 64`` inner width, DropPath 0.1 on every residual branch, LayerNorm head; 4-D images or 3-D [B, n, 192]
    patch vectors.  ``with_land=True`` adds the trainable MobileNetV3 landmark regressor (``stn`` + ``output_layer``, stock
    PyTorch-ROCm / MIOpen) whose landmarks drive the single-launch HIP patch gather; gradients flow back through the patch
    embedding and the gather into theta (reference :679-711).  Element dropout (``dropout`` after to_out / GELU / fc2,
    ``emb_dropout`` on the embedded tokens) is fused into the GEMM epilogues with counter-based masks (same distribution as
    nn.Dropout, different random stream)."""

    def __init__(self, *, loss_type, GPU_ID, num_class, image_size, patch_size, dim, depth, heads, mlp_dim, pool='cls',
                 num_patches=None, channels=3, dim_head=64, dropout=0., emb_dropout=0., fp16=True, with_land=False,
                 use_standcoord=False, Random_prob=False, shuffle=False, drop_path_rate=0.1):
        super().__init__()
        if patch_size != 8 or channels != 3 or dim_head != 64:
            raise NotImplementedError("HIP kernels are specialised for 3x8x8 patches and head_dim 64")
        if not (0.0 <= dropout < 1.0 and 0.0 <= emb_dropout < 1.0):
            raise ValueError("dropout rates must be in [0, 1)")
        if pool != 'cls':
            raise NotImplementedError("only cls pooling is on the hot path")
        if num_patches is None:
            num_patches = (image_size // patch_size) ** 2
        self.patch_size, self.fp16, self.num_patches = patch_size, fp16, num_patches
        self.row_num = int(math.sqrt(num_patches))
        self.with_land, self.pool, self.loss_type, self.GPU_ID = with_land, pool, loss_type, GPU_ID
        self.use_standcoord, self.Random_prob, self.shuffle = use_standcoord, Random_prob, shuffle      # reference :576, 717-742
        self._want_tokens, self._last_tokens = False, None
        if with_land:                                     # reference :577-602
            from .mobilenet import MobileNetV3_backbone
            self.stn = MobileNetV3_backbone(mode='large')
            self.output_layer = nn.Sequential(nn.Dropout(p=0.5), nn.Linear(160, self.row_num * self.row_num * 2))
        self.patch_shape = torch.tensor([patch_size, patch_size])
        self.dim, self.depth, self.heads, self.mlp_dim = dim, depth, heads, mlp_dim
        self.drop_path_rate = drop_path_rate
        # element dropout (after to_out, after GELU, after fc2, and on the embedded tokens): fused into the GEMM epilogues
        # with counter-based masks; `_drop_step` advances the seed every training forward
        self.dropout_rate, self.emb_dropout_rate, self._drop_seed0, self._drop_step = float(dropout), float(emb_dropout), 0x5EED, 0
        inner = heads * dim_head
        self.pos_embedding = nn.Parameter(torch.randn(1, num_patches + 1, dim))
        self.patch_to_embedding = nn.Linear(channels * patch_size ** 2, dim)
        self.cls_token = nn.Parameter(torch.randn(1, 1, dim))
        self.transformer = _Holder()
        layers = []
        for _ in range(depth):
            att = _Holder(); att.fn = _Holder(); att.fn.norm = nn.LayerNorm(dim); att.fn.fn = _Holder()
            att.fn.fn.to_qkv = nn.Linear(dim, inner * 3, bias=False)
            att.fn.fn.to_out = nn.Sequential(nn.Linear(inner, dim), nn.Dropout(dropout))
            ff = _Holder(); ff.fn = _Holder(); ff.fn.norm = nn.LayerNorm(dim); ff.fn.fn = _Holder()
            ff.fn.fn.net = nn.Sequential(nn.Linear(dim, mlp_dim), nn.GELU(), nn.Dropout(dropout), nn.Linear(mlp_dim, dim), nn.Dropout(dropout))
            layers.append(nn.ModuleList([att, ff]))
        self.transformer.layers = nn.ModuleList(layers)
        self.mlp_head = nn.Sequential(nn.LayerNorm(dim))
        if loss_type == 'None':
            pass
        elif loss_type == 'CosFace':
            self.loss = CosFace(in_features=dim, out_features=num_class, device_id=GPU_ID, m=0.4)
        elif loss_type == 'AdaFace':
            self.loss = AdaFace(in_features=dim, out_features=num_class, device_id=GPU_ID, m=0.4)
        else:
            raise NotImplementedError(f"loss_type {loss_type!r}: only 'CosFace' and 'None' exist in the reference")
        self.theta = 0
        self._arena, self._spec, self._hook = None, None, None

    def _bind_arena(self, arena, prefix):
        names = []
        for i in range(self.depth):
            a, f = f"{prefix}transformer.layers.{i}.0.fn.", f"{prefix}transformer.layers.{i}.1.fn."
            names.append(dict(ln1_g=a + "norm.weight", ln1_b=a + "norm.bias", w_qkv=a + "fn.to_qkv.weight", b_qkv=None,
                              w_proj=a + "fn.to_out.0.weight", b_proj=a + "fn.to_out.0.bias",
                              ln2_g=f + "norm.weight", ln2_b=f + "norm.bias",
                              w_fc1=f + "fn.net.0.weight", b_fc1=f + "fn.net.0.bias",
                              w_fc2=f + "fn.net.3.weight", b_fc2=f + "fn.net.3.bias"))
        trunk = Fn.TrunkSpec(dim=self.dim, heads=self.heads, mlp=self.mlp_dim, depth=self.depth, ln_eps=1e-5,
                             attn_scale=self.dim ** -0.5, block_names=names)      # scale quirk: model dim (ref :145)
        object.__setattr__(self, "_arena", arena)
        self._spec = Fn.ViTSpec(trunk=trunk, prefix=prefix, patch_order=_lib.PATCH_ORDER_HWC,
                                w_patch="patch_to_embedding.weight", b_patch="patch_to_embedding.bias", cls="cls_token",
                                final_g="mlp_head.0.weight", final_b="mlp_head.0.bias", pos="pos_embedding")
        self._hook = torch.zeros(1, device=arena.device, requires_grad=True)

    def _sample_drop_scales(self, geom):
        """Residual_droppath: the same rate on both branches of every layer (reference :106-112)."""
        if not self.drop_path_rate:
            return None
        keep = 1.0 - self.drop_path_rate
        u = torch.rand(self.depth, 2, geom.n_seq, device=self._arena.device)
        return (torch.floor(keep + u) / keep).contiguous()

    def _next_dropout(self):
        """(p_trunk, p_embedding, seed) for this forward, or None in eval mode / at rate 0."""
        if not self.training or (self.dropout_rate == 0.0 and self.emb_dropout_rate == 0.0):
            return None
        self._drop_step += 1
        return (self.dropout_rate, self.emb_dropout_rate, (self._drop_seed0 + 7919 * self._drop_step) & 0x3FFFFFFF)

    def forward_embedding(self, x):
        if self._arena is None:
            attach_arena(self)
        self._arena.ensure_fresh()
        n = x.shape[1] if x.dim() == 3 else (x.shape[-1] // 8) ** 2
        pos = self.pos_embedding[0, :n + 1]
        return _PartFViTFunction.apply(self, self._hook, x, pos)

    def landmarks(self, x):
        """[B,3,112,112] -> theta [B, r*r, 2] in pixels: CNN -> mean pool -> Dropout(0.5)+Linear(160, 2*r*r) -> per-sample
        min-max to [0, 111] (reference :680-706).  Differentiable (torch autograd over MIOpen convolutions)."""
        t = self.output_layer(self.stn(x).mean(dim=(-2, -1)))
        tmax, tmin = t.max(dim=1, keepdim=True)[0], t.min(dim=1, keepdim=True)[0]
        return ((t - tmin) / (tmax - tmin) * 111).view(-1, self.row_num * self.row_num, 2)

    def _gather_inputs(self, x, keep_num=None):
        """The front of `forward` (reference :679-742): images -> (what the trunk embeds, theta).  With the landmark branch or the
        standard coordinates a 4-D batch becomes the mosaic of patches gathered at theta; anything else passes through."""
        if self._arena is None:
            attach_arena(self)
        theta = self.theta
        if self.with_land and x.dim() == 4:
            num_land = keep_num if keep_num is not None else self.row_num * self.row_num
            theta = self.landmarks(x)
            self.theta = theta
            x = extract_patches_pytorch_gridsample(x, theta[:, :num_land], patch_shape=self.patch_shape, num_landm=num_land)
        if self.use_standcoord and x.dim() == 4:
            b, side = x.shape[0], x.shape[-1]
            num_land = (side // self.patch_size) ** 2
            rc = torch.arange(0, int(math.isqrt(num_land)), dtype=torch.float32) * 8 + 4
            cx, cy = torch.meshgrid(rc, rc, indexing="ij")
            theta = torch.stack((cx, cy), 2).view(1, -1, 2).repeat(b, 1, 1)
            if self.Random_prob:
                theta = theta + torch.randn(theta.shape) * 3
            if self.shuffle:
                ids = torch.randint(0, theta.shape[1], (b, theta.shape[1], 1))
                theta = torch.gather(theta, 1, ids.repeat(1, 1, 2))
            theta = theta.to(x.device)
            x = extract_patches_pytorch_gridsample(x, theta[:, :num_land], patch_shape=self.patch_shape, num_landm=num_land)
            x = x.permute(0, 1, 3, 2).contiguous()
        return x, theta

    def forward(self, x, label=None, mask=None, visualize=False, save_token=False, opt=None, keep_num=None, glo_diff=False):
        """(reference :659-795)  `save_token`: also the patch tokens behind the transformer, in front of the head's LayerNorm, detached
        (an analysis dump in the reference: returns (emb, tokens, theta)); `use_standcoord` (constructor): the patches are gathered at
        the centres of the regular 8 x 8 grid -- jittered by N(0, 3^2) px with `Random_prob`, re-drawn with replacement with `shuffle`,
        both from the CPU generator in the reference's order -- and the mosaic is transposed (:717-742).  Attention masks are not
        supported (never passed by either entry point)."""
        if mask is not None:
            raise NotImplementedError("attention masks are not on the training hot path (never passed by either entry point)")
        x, theta = self._gather_inputs(x, keep_num)
        self._want_tokens = bool(save_token)
        emb = self.forward_embedding(x)
        self._want_tokens = False
        if save_token:
            return emb, self._last_tokens, self.theta
        if label is not None:
            return self.loss(emb, label), self.theta
        return (emb, theta) if visualize else emb

    @torch.no_grad()
    def get_selfattention(self, x, layer=-1, cls_only=False):
        """Attention probabilities of block `layer` and the landmarks they belong to: (attn f32 [B, heads, n+1, n+1] -- or
        [B, heads, 1, n+1], the cls query alone, with `cls_only` -- , theta [B, r*r, 2] in pixels as `visualize=True` returns it).
        Replaces reading ``transformer.layers[l][0].fn.fn.attention_score`` behind a forward of the reference
        (face_pre_pro/ViT_face.py:175-177; drawn by util/utils.py visualize_attentionmap_*_landmark): the fused forward never stores
        the probabilities, so the blocks in front of `layer` run as usual and lafs_attention_probs forms P from that block's own q
        and k with the block's dim ** -0.5 scale.  Eval mode only: element dropout and DropPath would make the read-out differ from
        the forward that just ran.  Attention masks are not supported."""
        if self.training:
            raise RuntimeError("get_selfattention reads out the deterministic eval-mode forward: call model.eval() first")
        if not -self.depth <= layer < self.depth:
            raise ValueError(f"layer must be in {-self.depth}..{self.depth - 1}, got {layer}")
        layer %= self.depth
        x, theta = self._gather_inputs(x)
        self._arena.ensure_fresh()
        n_img = x.shape[0]
        n = x.shape[1] if x.dim() == 3 else (x.shape[-1] // 8) ** 2
        side = 8 * int(math.isqrt(n))
        if (side // 8) ** 2 != n:
            raise _lib.LafsHipError("the packed engine needs a square number of patches per image")
        geom = Fn.geometry([(n_img, side)], x.device)
        tokens, streams = Fn.vit_streams(self._arena, self._spec, geom, [x.contiguous().float()],
                                         [self.pos_embedding[0, :n + 1].detach().contiguous()], [max(layer, 1)])
        attn = Fn.vit_block_probs(self._arena, self._spec, geom, streams[0] if layer > 0 else tokens, layer, q_rows=1 if cls_only else 0)
        return attn, theta


# ------------------------------------------------------------------------------------------------- landmark CNN wrapper
class face_landmark_4simmin_glo_loc(nn.Module):
    """Frozen landmark regressor of the LAFS step (reference face_pre_pro/ViT_face.py:1218-1409): MobileNetV3 trunk ->
    mean pool -> Linear(160, 2*r*r) -> per-sample min-max to [0, 111] px -> optional N(0, 5^2) px jitter -> optional random
    choice of 36 landmarks (with replacement) -> 8x8 bilinear patch gather from ``x_Aug`` into a mosaic image.
    The CNN runs on stock PyTorch-ROCm; the gather is the single-launch HIP kernel.  Random draws are made on the CPU
    generator in the reference's order (randn for the jitter, then randint for the selection) and moved to the device."""

    def __init__(self, *, loss_type, GPU_ID, num_class, image_size, patch_size, dim, depth, heads, mlp_dim, pool='cls',
                 num_patches=None, channels=3, dim_head=64, dropout=0., emb_dropout=0., fp16=True):
        super().__init__()
        from .mobilenet import MobileNetV3_backbone
        if num_patches is None:
            num_patches = (image_size // patch_size) ** 2
        if patch_size != 8:
            raise NotImplementedError("the HIP gather kernel is specialised for 8x8 patches")
        self.patch_size, self.fp16, self.num_patches, self.dim = patch_size, fp16, num_patches, dim
        self.row_num = int(math.sqrt(num_patches))
        self.stn = MobileNetV3_backbone(mode='large')
        self.output_layer = nn.Sequential(nn.Dropout(p=0.5), nn.Linear(160, self.row_num * self.row_num * 2))
        self.global_token = nn.Sequential(nn.Dropout(p=0.5), nn.Linear(160, dim))
        self.patch_shape = torch.tensor([patch_size, patch_size])
        self.pos_embedding = nn.Parameter(torch.randn(1, num_patches + 1, dim))
        self.patch_to_embedding = nn.Linear(channels * patch_size ** 2, dim)
        self.cls_token = nn.Parameter(torch.randn(1, 1, dim))
        self.mask_token = nn.Parameter(torch.zeros(1, 1, dim))
        nn.init.trunc_normal_(self.mask_token, std=.02, a=-.02, b=.02)
        self.loss_type, self.GPU_ID, self.num_features, self.in_chans = loss_type, GPU_ID, dim, channels
        self.theta = 0

    def landmarks(self, x):
        """[B,3,S,S] -> theta [B, r*r, 2] in pixels (x, y), min-max scaled per sample (reference :1338-1355)."""
        t = self.output_layer(self.stn(x).mean(dim=(-2, -1)))
        tmax, tmin = t.max(dim=1, keepdim=True)[0], t.min(dim=1, keepdim=True)[0]
        return ((t - tmin) / (tmax - tmin) * 111).view(-1, self.row_num * self.row_num, 2)

    def forward(self, x, x_Aug=None, keep_num=None, patch_shape=None, Random_prob=False, return_prob=False, ran_sample=False,
                random_coor=False, return_land=False):
        if random_coor:
            num_land = 25 if ran_sample else self.row_num * self.row_num
            theta = (torch.rand(x.shape[0], num_land, 2) * 111.0).to(x.device)
        else:
            S = x.shape[-2]
            num_land = self.num_patches if (S == 112 and self.num_patches in (144, 196)) else (S // self.patch_size) ** 2
            theta = self.landmarks(x)
            if Random_prob:
                theta = theta + (torch.randn(theta.shape) * 5).to(theta.device)
                if not return_prob:
                    b, c, _ = theta.shape
                    num_land = 36 if ran_sample else self.row_num * self.row_num
                    idx = torch.randint(0, c, (b, num_land, 1)).to(theta.device).repeat(1, 1, 2)
                    theta = torch.gather(theta, 1, idx)
            self.theta = theta
        if return_land:
            return theta, x
        src = x if x_Aug is None else x_Aug
        return theta, extract_patches_pytorch_gridsample(src, theta[:, :num_land], patch_shape=self.patch_shape, num_landm=num_land)


# ------------------------------------------------------------------------------------------------- fViT
class _FViTFunction(torch.autograd.Function):
    """One crop group of fViT as one autograd node: window embedding, trunk, BatchNorm1d head.  Parameter gradients are accumulated by
    the kernels into the arena; the position slice and (when it asks for one) the input are differentiable."""

    @staticmethod
    def forward(ctx, model, hook, x, pos, geom):
        save = any(ctx.needs_input_grad)
        drop = model._sample_drop_scales(geom) if model.training else None
        feat, st, _ = Fn.vit_forward(model._arena, model._spec, geom, [x.contiguous().float()], [pos.detach().contiguous()],
                                     drop, save=save, dropout=model._next_dropout(), bn_training=model.training)
        ctx.model, ctx.st = model, (st if save else None)
        return feat

    @staticmethod
    def backward(ctx, dfeat):
        model, st = ctx.model, ctx.st
        if not ctx.needs_input_grad[2]:
            dpos = Fn.vit_backward(model._arena, model._spec, st, dfeat)
            return None, None, None, dpos[0], None
        dpos, dx = Fn.vit_backward(model._arena, model._spec, st, dfeat, want_dx=True)
        return None, None, dx[0], dpos[0], None


class _FViTGroupsFunction(torch.autograd.Function):
    """Several crop groups of fViT in ONE packed pass as one autograd node; the BatchNorm1d head keeps per-group statistics
    (lafs_bn1d_groups_fwd / _bwd).  Inputs behind the hook: the groups' images, then their position slices."""

    @staticmethod
    def forward(ctx, model, n_groups, hook, geom, *tensors):
        imgs, pos = tensors[:n_groups], tensors[n_groups:]
        save = any(ctx.needs_input_grad)
        drop = model._sample_drop_scales(geom) if model.training else None
        feat, st, _ = Fn.vit_forward(model._arena, model._spec, geom, [x.contiguous().float() for x in imgs],
                                     [p.detach().contiguous() for p in pos], drop, save=save, dropout=model._next_dropout(),
                                     bn_training=model.training)
        ctx.model, ctx.st, ctx.n_groups = model, (st if save else None), n_groups
        return feat

    @staticmethod
    def backward(ctx, dfeat):
        model, st, G = ctx.model, ctx.st, ctx.n_groups
        if not any(ctx.needs_input_grad[4:4 + G]):
            dpos = Fn.vit_backward(model._arena, model._spec, st, dfeat)
            return (None,) * (4 + G) + tuple(dpos)
        dpos, dx = Fn.vit_backward(model._arena, model._spec, st, dfeat, want_dx=True)
        return (None,) * 4 + tuple(d if need else None for d, need in zip(dx, ctx.needs_input_grad[4:4 + G])) + tuple(dpos)


class ViTs_face_overlap(nn.Module):
    """fViT (reference face_pre_pro/ViT_face.py:1506-1613): the Part-fViT transformer (pre-LN, bias-free qkv, scale dim**-0.5,
    ``heads * 64`` inner width, DropPath on every residual branch) behind an OVERLAPPING patch embedding -- nn.Unfold(ac_patch_size,
    stride patch_size, padding pad) + Linear, one lafs_unfold_bf16 launch + the embedding GEMM here -- and with a BatchNorm1d head on the
    cls rows (lafs_bn1d_fwd / lafs_bn1d_bwd).  4-D images or 3-D [B, n, 3 * ac_patch_size**2] window vectors; a list of crops runs
    one pass per run of equal-sided crops, so the batch statistics and the running-statistic updates are per group, in list order.
    ``forward_groups`` runs already concatenated groups as ONE packed pass with the same per-group statistics (lafs_bn1d_groups_fwd).
    ``soft_split``, ``dropout`` and ``to_latent`` are kept as attributes for parity and never called; ``fc``, whose result the
    reference discards (:1606-1607), is ignored.  ``drop_path_rate``: the reference hard-codes 0.1 in Residual_droppath.
    ``loss_type='CosFace'`` builds the margin head the reference left commented out (:1539-1549; key ``loss.weight``, as in Part-fViT), which
    ``forward_features(img, label=y)`` applies (:1609-1611) and FinetuneEngine trains; ``'None'`` builds the released key set."""

    def __init__(self, *, loss_type, GPU_ID, num_class, image_size, patch_size, ac_patch_size, pad, dim, depth, heads, mlp_dim,
                 pool='cls', channels=3, dim_head=64, dropout=0., emb_dropout=0., drop_path_rate=0.1):
        super().__init__()
        if pool != 'cls':
            raise NotImplementedError("only cls pooling is on the hot path (the gather kernel reads the first row of every sequence)")
        if channels != 3:
            raise NotImplementedError("lafs_unfold_bf16 reads 3-channel images")
        if dim_head != 64:
            raise NotImplementedError("the attention kernels are specialised for head_dim 64")
        if not (0.0 <= dropout < 1.0 and 0.0 <= emb_dropout < 1.0):
            raise ValueError("dropout rates must be in [0, 1)")
        if not (ac_patch_size >= 1 and patch_size >= 1 and 0 <= pad < ac_patch_size):
            raise ValueError("the embedding window needs ac_patch_size >= 1, patch_size >= 1 and 0 <= pad < ac_patch_size")
        num_patches = (image_size // patch_size) ** 2
        if num_patches <= 16:                             # reference :1513 (MIN_NUM_PATCHES)
            raise ValueError(f"your number of patches ({num_patches}) is way too small for attention to be effective (at least 16)")
        self.patch_size, self.ac_patch_size, self.pad, self.num_patches = patch_size, ac_patch_size, pad, num_patches
        self.soft_split = nn.Unfold(kernel_size=(ac_patch_size, ac_patch_size), stride=(patch_size, patch_size), padding=(pad, pad))
        self.dim, self.depth, self.heads, self.mlp_dim = dim, depth, heads, mlp_dim
        self.drop_path_rate = drop_path_rate
        self.dropout_rate, self.emb_dropout_rate, self._drop_seed0, self._drop_step = float(dropout), float(emb_dropout), 0x5EED, 0
        inner = heads * dim_head
        self.pos_embedding = nn.Parameter(torch.randn(1, num_patches + 1, dim))
        self.patch_to_embedding = nn.Linear(channels * ac_patch_size ** 2, dim)
        self.cls_token = nn.Parameter(torch.randn(1, 1, dim))
        self.dropout = nn.Dropout(emb_dropout)
        self.transformer = _Holder()
        layers = []
        for _ in range(depth):
            att = _Holder(); att.fn = _Holder(); att.fn.norm = nn.LayerNorm(dim); att.fn.fn = _Holder()
            att.fn.fn.to_qkv = nn.Linear(dim, inner * 3, bias=False)
            att.fn.fn.to_out = nn.Sequential(nn.Linear(inner, dim), nn.Dropout(dropout))
            ff = _Holder(); ff.fn = _Holder(); ff.fn.norm = nn.LayerNorm(dim); ff.fn.fn = _Holder()
            ff.fn.fn.net = nn.Sequential(nn.Linear(dim, mlp_dim), nn.GELU(), nn.Dropout(dropout), nn.Linear(mlp_dim, dim), nn.Dropout(dropout))
            layers.append(nn.ModuleList([att, ff]))
        self.transformer.layers = nn.ModuleList(layers)
        self.pool = pool
        self.to_latent = nn.Identity()
        self.mlp_head = nn.Sequential(nn.BatchNorm1d(dim))
        self.loss_type, self.pred, self.GPU_ID, self.fc = loss_type, None, GPU_ID, None
        # the margin head the reference left commented out at :1539-1549 (`loss.weight`, as in Part-fViT): what a fine-tune needs.
        # 'None' builds no module, so the released checkpoints still load with strict=True
        if loss_type == 'None':
            pass
        elif loss_type == 'CosFace':
            self.loss = CosFace(in_features=dim, out_features=num_class, device_id=GPU_ID)
        elif loss_type == 'AdaFace':
            self.loss = AdaFace(in_features=dim, out_features=num_class, device_id=GPU_ID)
        else:
            raise NotImplementedError(f"loss_type {loss_type!r}: only 'CosFace' and 'None' exist in the reference")
        self._arena, self._spec, self._hook = None, None, None

    _sample_drop_scales = ViT_face_landmark_patch8._sample_drop_scales
    _next_dropout = ViT_face_landmark_patch8._next_dropout

    def _bind_arena(self, arena, prefix):
        from dataclasses import replace
        ViT_face_landmark_patch8._bind_arena(self, arena, prefix)           # the same transformer, the same block naming
        bn = self.mlp_head[0]
        if bn.momentum is None or not bn.track_running_stats or not bn.affine:
            raise NotImplementedError("lafs_bn1d_fwd implements nn.BatchNorm1d's defaults: affine, running statistics, a fixed momentum")
        self._spec = replace(self._spec, patch_order=_lib.PATCH_ORDER_CHW, window=(self.ac_patch_size, self.patch_size, self.pad),
                             head="batchnorm", bn_mean="mlp_head.0.running_mean", bn_var="mlp_head.0.running_var",
                             bn_eps=float(bn.eps), bn_momentum=float(bn.momentum))

    def forward(self, x, return_before_head=False, patch_drop=0., for_fea=False):
        """(reference :1550-1573)  A tensor or a list of crops; consecutive crops of equal side form one group."""
        if for_fea:
            return self.forward_features(x, patch_drop=patch_drop)
        if not isinstance(x, list):
            x = [x]
        h, z, start = None, None, 0
        while start < len(x):
            end = start + 1
            while end < len(x) and x[end].shape[-1] == x[start].shape[-1]:
                end += 1
            _h = self.forward_features(torch.cat(x[start:end]) if end - start > 1 else x[start], patch_drop=patch_drop)
            _z = self.forward_head(_h)
            h, z = (_h, _z) if h is None else (torch.cat((h, _h)), torch.cat((z, _z)))
            patch_drop, start = 0., end
        return (h, z) if return_before_head else z

    def forward_head(self, x):
        return self.pred(x) if self.pred is not None else x

    def forward_groups(self, groups):
        """Already concatenated crop groups (one tensor per resolution) in ONE packed pass -> BatchNorm1d(cls) f32 [sum B, dim], the
        rows in group order.  What ``forward(list)`` gives by running the groups one after the other (reference :1556-1569): the
        BatchNorm statistics are per group and the running buffers are updated once per group, in list order
        (lafs_bn1d_groups_fwd); the trunk runs once over all tokens.  MultiCropWrapper.forward takes this pass."""
        if len(groups) == 1:
            return self.forward_features(groups[0])
        if len(groups) > 4:
            raise NotImplementedError("the packed trunk runs at most 4 crop resolutions in one pass")
        shapes = [self._window_geometry(img) for img in groups]
        if self.training and min(n_img for n_img, _, _ in shapes) < 2:
            raise ValueError("Expected more than 1 value per channel when training (a crop group of one image)")
        geom = Fn.geometry([(n_img, side) for n_img, side, _ in shapes], groups[0].device,
                           window=(self.ac_patch_size, self.patch_size, self.pad))
        pos = [self.pos_embedding[0, :n + 1] for _, _, n in shapes]
        emb = _FViTGroupsFunction.apply(self, len(groups), self._hook, geom, *groups, *pos)
        if self.training:
            self.mlp_head[0].num_batches_tracked += len(groups)
        return emb

    def forward_features(self, img, label=None, mask=None, patch_drop=None):
        """(reference :1578-1613)  One group: [B, 3, S, S] images or [B, n, 3 k^2] window vectors -> BatchNorm1d(cls) f32 [B, dim].
        The position table is sliced ``[:, :n + 1]``, not resampled (:1590)."""
        if mask is not None:
            raise NotImplementedError("attention masks are not on the hot path (the packed attention kernels take none)")
        if label is not None and not hasattr(self, "loss"):
            raise NotImplementedError("the reference builds no loss module for this class (its construction is commented out at "
                                      ":1539-1549), so its label branch cannot run there either")
        if patch_drop is not None and patch_drop > 0:
            raise NotImplementedError("patch_drop > 0 leaves a non-square number of tokens, which the packed geometry cannot describe yet")
        n_img, side, n = self._window_geometry(img)
        bn = self.mlp_head[0]
        if self.training and n_img < 2:                   # what nn.BatchNorm1d raises (torch/nn/functional.py _verify_batch_size)
            raise ValueError(f"Expected more than 1 value per channel when training, got input size {torch.Size([n_img, self.dim])}")
        geom = Fn.geometry([(n_img, side)], img.device, window=(self.ac_patch_size, self.patch_size, self.pad))
        emb = _FViTFunction.apply(self, self._hook, img, self.pos_embedding[0, :n + 1], geom)
        if self.training:
            bn.num_batches_tracked += 1
        if label is not None:                             # reference :1609-1611
            return self.loss(emb, label), emb
        return emb

    def _window_geometry(self, img):
        """(images, side, windows) of one group -- [B, 3, S, S] images or [B, n, 3 k^2] window vectors -- with the arena attached and
        fresh; `side` is a side that unfolds into sqrt(n) windows per side."""
        if self._arena is None:
            attach_arena(self)
        self._arena.ensure_fresh()
        k, stride, pad = self.ac_patch_size, self.patch_size, self.pad
        n_img = img.shape[0]
        if img.dim() == 4:
            if img.shape[1] != 3 or img.shape[-1] != img.shape[-2]:
                raise ValueError(f"expected square 3-channel images, got {tuple(img.shape)}")
            side = img.shape[-1]
            r = ops.unfold_windows(side, k, stride, pad) if side + 2 * pad >= k else 0
        elif img.dim() == 3:
            r = int(math.isqrt(img.shape[1]))
            if r * r != img.shape[1] or img.shape[2] != 3 * k * k:
                raise ValueError(f"expected [B, n, {3 * k * k}] window vectors with a square n, got {tuple(img.shape)}")
            side = (r - 1) * stride + k - 2 * pad         # a side that unfolds into r x r windows
        else:
            raise ValueError(f"expected a 4-D image batch or 3-D window vectors, got {img.dim()} dimensions")
        n = r * r
        if n < 1:
            raise ValueError(f"a {side}-pixel image is smaller than one {k}-pixel window")
        if n > self.num_patches:
            raise ValueError(f"the input unfolds into {n} windows, the position table holds {self.num_patches} "
                             f"((image_size // patch_size) ** 2): build the model with a larger image_size")
        return n_img, side, n

    @torch.no_grad()
    def get_selfattention(self, x, layer=-1, cls_only=False):
        """Attention probabilities of block `layer`: attn f32 [B, heads, n+1, n+1], or [B, heads, 1, n+1] (the cls query alone) with
        `cls_only`; token 1 + i r + j is window (i, j) of nn.Unfold's row-major r x r grid.  The signature and rules of
        ViT_face_landmark_patch8.get_selfattention, without a theta: the blocks in front of `layer` run as usual and
        lafs_attention_probs forms P from that block's own q and k with the dim ** -0.5 scale.  Eval mode only, so the BatchNorm head
        behind the blocks reads its running statistics and writes nothing: the buffers and num_batches_tracked stay as they are.
        Attention masks are not supported."""
        if self.training:
            raise RuntimeError("get_selfattention reads out the deterministic eval-mode forward: call model.eval() first")
        if not -self.depth <= layer < self.depth:
            raise ValueError(f"layer must be in {-self.depth}..{self.depth - 1}, got {layer}")
        layer %= self.depth
        n_img, side, n = self._window_geometry(x)
        geom = Fn.geometry([(n_img, side)], x.device, window=(self.ac_patch_size, self.patch_size, self.pad))
        pos = self.pos_embedding[0, :n + 1].detach().contiguous()
        tokens, streams = Fn.vit_streams(self._arena, self._spec, geom, [x.contiguous().float()], [pos], [max(layer, 1)])
        return Fn.vit_block_probs(self._arena, self._spec, geom, streams[0] if layer > 0 else tokens, layer, q_rows=1 if cls_only else 0)
