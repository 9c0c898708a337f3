#!/usr/bin/env python
"""How far do the REFERENCE's own LAFS-step results move when every nn.Linear multiplies bf16-rounded operands with fp32 accumulation --
what the HIP trunk and heads do -- and nothing else changes?  Runs the two-step recipe of F27 (fViT pair, BatchNorm1d head;
tools/make_golden_fvit_ssl.py) and of F16 (Part-fViT pair, LayerNorm head; tools/make_golden.py) on the CPU, once in fp32 and once
with that rounding, and prints the relative-L2 distance of the logits and of the clipped per-tensor gradients.  Seed 27 is F27's own
model and crops.  It tells a model's conditioning from a kernel's error: DESIGN.md section 2 quotes its figures next to the errors the
engine shows against F27.  Needs the reference checkout (LAFS_REFERENCE, as tools/make_golden.py); stores nothing.

    python tools/fvit_ssl_conditioning.py
"""
import os
import sys

import torch
import torch.distributed as dist
import torch.nn.functional as F

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from make_golden import _import_reference  # noqa: E402

os.environ.setdefault("MASTER_ADDR", "127.0.0.1"); os.environ.setdefault("MASTER_PORT", "29549")
dist.init_process_group("gloo", rank=0, world_size=1)              # DINOLoss.update_center all-reduces
ref_utils, ref_vit, ref_lafs, ref_face, _ = _import_reference()
torch.set_num_threads(8)
r = lambda t: t.bfloat16().float()


class BfLinear(torch.autograd.Function):
    """F.linear on bf16-rounded x and W; the backward rounds the incoming gradient for dgrad and wgrad, the bias gradient stays fp32."""
    @staticmethod
    def forward(ctx, x, w, b):
        xr, wr = r(x), r(w); ctx.save_for_backward(xr, wr); ctx.hb = b is not None
        y = xr @ wr.t()
        return y + b if b is not None else y
    @staticmethod
    def backward(ctx, g):
        xr, wr = ctx.saved_tensors; gr = r(g)
        dx = gr @ wr
        dw = gr.reshape(-1, gr.shape[-1]).t() @ xr.reshape(-1, xr.shape[-1])
        return dx, dw, (g.reshape(-1, g.shape[-1]).sum(0) if ctx.hb else None)


orig_linear = F.linear


def run(kind, emulate, seed):
    torch.manual_seed(seed)
    K, B = 256, 4 if kind == "fvit" else 2
    def mk():
        if kind == "fvit":
            m = ref_face.ViTs_face_overlap(loss_type="None", GPU_ID=None, num_class=10, image_size=112, patch_size=8, ac_patch_size=12, pad=4, dim=64, depth=2, heads=2, mlp_dim=128, dropout=0, emb_dropout=0)
        else:
            m = ref_face.ViT_face_landmark_patch8(loss_type="None", GPU_ID=None, num_class=10, image_size=112, patch_size=8, dim=64, depth=2, heads=2, num_patches=196, mlp_dim=128, dropout=0.0, emb_dropout=0.0, with_land=False, use_standcoord=False, Random_prob=False, shuffle=False)
        for q in m.modules():
            if isinstance(q, ref_vit.DropPath): q.drop_prob = 0.0
        return m
    student = ref_utils.MultiCropWrapper(mk(), ref_vit.DINOHead(64, K, hidden_dim=64, bottleneck_dim=32, norm_last_layer=True))
    teacher = ref_utils.MultiCropWrapper(mk(), ref_vit.DINOHead(64, K, hidden_dim=64, bottleneck_dim=32))
    if kind == "fvit":
        with torch.no_grad():
            sb = student.backbone; sb.pos_embedding.mul_(0.05); sb.cls_token.mul_(0.05)
            bn = sb.mlp_head[0]; bn.weight.copy_(1 + 0.1 * torch.randn(64)); bn.bias.copy_(0.1 * torch.randn(64))
    teacher.load_state_dict(student.state_dict())
    for p in teacher.parameters(): p.requires_grad = False
    crit = ref_lafs.DINOLoss(K, 4, 0.07, 0.04, 3, 10)
    opt = torch.optim.AdamW(ref_utils.get_params_groups(student))
    if kind == "fvit":
        crops = [torch.randn(B, 3, s, s).clamp(-1, 1).half().float() for s in (112, 112, 48, 48)]
    else:
        crops = [torch.randn(B, 196, 192).clamp(-1, 1) for _ in range(2)] + [torch.randn(B, 36, 192).clamp(-1, 1) for _ in range(2)]
    lrs, wds, moms = [5e-4, 4e-4], [0.04, 0.05], [0.9, 0.95]
    out = []
    F.linear = (lambda x, w, b=None: BfLinear.apply(x, w, b)) if emulate else orig_linear
    try:
        for step in range(2):
            for i, g in enumerate(opt.param_groups):
                g["lr"] = lrs[step]
                if i == 0: g["weight_decay"] = wds[step]
            t_out = teacher(crops[:2]); s_out = student(crops)
            loss = crit(s_out, t_out, step)
            opt.zero_grad(); loss.backward()
            ref_utils.clip_gradients(student, 3.0)
            out.append(dict(loss=loss.item(), s_out=s_out.detach().clone(), t_out=t_out.detach().clone(),
                            g={n: p.grad.clone() for n, p in student.named_parameters() if p.grad is not None}))
            ref_utils.cancel_gradients_last_layer(step, student, 1)
            opt.step()
            with torch.no_grad():
                for pq, pk in zip(student.parameters(), teacher.parameters()):
                    pk.data.mul_(moms[step]).add_((1 - moms[step]) * pq.detach().data)
    finally:
        F.linear = orig_linear
    return out


rel = lambda a, b: float((a.double() - b.double()).norm() / (b.double().norm() + 1e-30))
ZS = "backbone.transformer.layers.1.1.fn.fn.net.3.bias"
for kind in ("partfvit", "fvit"):
    for seed in (27, 28, 29):
        a, b = run(kind, False, seed), run(kind, True, seed)
        for s in range(2):
            eg = {k: rel(b[s]["g"][k], v) for k, v in a[s]["g"].items() if not (kind == "fvit" and k == ZS)}
            w = max(eg, key=eg.get)
            print(f"{kind} seed {seed} step {s}: loss {abs(a[s]['loss']-b[s]['loss'])/a[s]['loss']:.2e}  s_out {rel(b[s]['s_out'], a[s]['s_out']):.2e}  t_out {rel(b[s]['t_out'], a[s]['t_out']):.2e}  worst grad {eg[w]:.2e} at {w}  median grad {sorted(eg.values())[len(eg)//2]:.2e}", flush=True)
