#!/usr/bin/env python
"""Golden vectors of the DINO head with BatchNorm (DINOHead(use_bn=True), lafs_train.py --use_bn_in_head true)
-> tests/golden/f29_head_bn*.npz and tests/golden/f30_lafs_step_head_bn*.npz.

Runs where the read-only reference checkout is mounted (LAFS_REFERENCE, as for tools/make_golden.py) and imports the reference's own
modules on the CPU in fp32 through tools/make_golden.py's import recipe; only numeric arrays are stored, none of the reference's text.
No committed file may exceed 1 MiB and random floats do not compress: each fixture goes, in key order, into as many parts as it takes
(<name>.npz, <name>_1.npz, ... with disjoint keys).

F29  two heads DINOHead(128, 1000, use_bn=True, hidden_dim=256, bottleneck_dim=64), BatchNorm weight 1 + 0.1 n, bias 0.1 n, 16 rows:
     c0.* norm_last_layer=True; c1.* norm_last_layer=False with weight_g x (1 + 0.2 n) (as F2's second case).  Per case
       p.*            the state dict before anything ran
       x, w, out, gx, g.*        a training forward + backward of (out * w).sum(); b1.* the BatchNorm buffers behind it
       x2, b2.*       a second training forward on new rows: the buffers behind it (num_batches_tracked 2)
       xe, out_e, gx_e, ge.*     eval(): forward + backward on new rows (gradients from zero); the buffers stay at b2
F30  the F5 pair (DINO ViT embed 64, depth 2, 1 head, patch 8; head hidden 128, bottleneck 64, K 512; DropPath 0) with use_bn=True in
     both heads, the BatchNorm parameters perturbed as in F29, B = 4, 2 global + 2 local crops rounded to fp16 BEFORE the reference
     sees them (crop0 .. crop3, shared by both steps), two full steps of lafs_train.py:577-613 in F27's format: s<k>.loss, s_out,
     t_out, center, norms (pre-clip, norm_names order), grad_post.* (post-clip), student.* / teacher.* (state dicts behind the step,
     buffers included); norm_names, membership_names / membership_reg (get_params_groups), hyper.  Neither network is put in eval
     mode: both heads normalise with batch statistics (student 16 rows, teacher 8) and step their own buffers once per step.
cond.*  how far the REFERENCE's own results move when nothing changes but every nn.Linear's input and weight (and, in the backward,
     the incoming gradient) is rounded to bf16 (tools/fvit_ssl_conditioning.py's BfLinear): relative-L2 per tensor group, the
     worst over the group's tensors and over the steps / cases.  The yardstick of the tests' gates.

In training mode the gradient of a Linear bias directly in front of a BatchNorm is a column sum that vanishes identically
(mlp.0.bias, mlp.3.bias of the head): the tool asserts on the reference's own numbers that both are below 1e-4 of the matching weight
gradient's norm; the tests leave exactly these two out of their relative gates.  In the full step (F30) the same holds one tensor
further up: the backbone's final LayerNorm bias is a per-row constant added in front of the head's first Linear, so its gradient is
W0^T applied to that same vanishing column sum (the student's head sees all crops as ONE BatchNorm group).  The tool asserts it on the
reference's numbers against norm.weight's gradient, and F30's tests leave out backbone.norm.bias as well.

    python tools/make_golden_head_bn.py
"""
import os
import sys

import numpy as np
import torch
import torch.nn.functional as F

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from make_golden import _import_reference, save  # noqa: E402

PART_BYTES = 900 * 1024
ZERO_SUM = ("mlp.0.bias", "mlp.3.bias")
ZERO_SUM_STEP = {"head.mlp.0.bias": "head.mlp.0.weight", "head.mlp.3.bias": "head.mlp.3.weight", "backbone.norm.bias": "backbone.norm.weight"}
BN_KEYS = tuple(f"mlp.{i}.{k}" for i in (1, 4) for k in ("running_mean", "running_var", "num_batches_tracked"))
r16 = lambda t: t.bfloat16().float()


class BfLinear(torch.autograd.Function):
    """F.linear on bf16-rounded x and W; the backward rounds the incoming gradient for dgrad and wgrad, the bias gradient stays fp32."""
    @staticmethod
    def forward(ctx, x, w, b):
        xr, wr = r16(x), r16(w); ctx.save_for_backward(xr, wr); ctx.hb = b is not None
        y = xr @ wr.t()
        return y + b if b is not None else y

    @staticmethod
    def backward(ctx, g):
        xr, wr = ctx.saved_tensors; gr = r16(g)
        dx = gr @ wr
        dw = gr.reshape(-1, gr.shape[-1]).t() @ xr.reshape(-1, xr.shape[-1])
        return dx, dw, (g.reshape(-1, g.shape[-1]).sum(0) if ctx.hb else None)


class bf16_linears:
    def __init__(self, on):
        self.on = on

    def __enter__(self):
        self.orig = F.linear
        if self.on:
            F.linear = lambda x, w, b=None: BfLinear.apply(x, w, b)

    def __exit__(self, *a):
        F.linear = self.orig


def perturb_bn(head):
    with torch.no_grad():
        for m in head.mlp:
            if isinstance(m, torch.nn.BatchNorm1d):
                m.weight.copy_(1 + 0.1 * torch.randn_like(m.weight)); m.bias.copy_(0.1 * torch.randn_like(m.bias))


def run_f29(ref_vit, emulate):
    torch.manual_seed(29)
    fx = {}
    for case, norm_last in (("c0.", True), ("c1.", False)):
        head = ref_vit.DINOHead(128, 1000, use_bn=True, norm_last_layer=norm_last, nlayers=3, hidden_dim=256, bottleneck_dim=64)
        perturb_bn(head)
        if not norm_last:
            with torch.no_grad():
                head.last_layer.weight_g.mul_(1 + 0.2 * torch.randn_like(head.last_layer.weight_g))
        x, w = torch.randn(16, 128, requires_grad=True), torch.randn(16, 1000)
        x2, xe = torch.randn(16, 128), torch.randn(16, 128, requires_grad=True)
        c = {"p." + k: v.clone() for k, v in head.state_dict().items()}
        with bf16_linears(emulate):
            assert head.training
            out = head(x)
            (out * w).sum().backward()
            c.update(x=x, w=w, out=out, gx=x.grad, **{"g." + k: p.grad.clone() for k, p in head.named_parameters() if p.grad is not None})
            c.update({"b1." + k: head.state_dict()[k].clone() for k in BN_KEYS})
            for k in ZERO_SUM:                                  # the column sums in front of a training-mode BatchNorm vanish
                assert float(c["g." + k].norm()) < 1e-4 * float(c["g." + k.replace("bias", "weight")].norm()), k
            with torch.no_grad():
                head(x2)
            c.update(x2=x2, **{"b2." + k: head.state_dict()[k].clone() for k in BN_KEYS})
            assert int(c["b2.mlp.1.num_batches_tracked"]) == 2 and int(c["b2.mlp.4.num_batches_tracked"]) == 2
            head.eval()
            head.zero_grad()
            out_e = head(xe)
            (out_e * w).sum().backward()
            c.update(xe=xe, out_e=out_e, gx_e=xe.grad, **{"ge." + k: p.grad.clone() for k, p in head.named_parameters() if p.grad is not None})
            for k in BN_KEYS:
                assert torch.equal(head.state_dict()[k], c["b2." + k]), k
        fx.update({case + k: v for k, v in c.items()})
    return fx


def run_f30(ref_utils, ref_vit, ref_lafs, emulate):
    torch.manual_seed(30)
    K, B, ncrops = 512, 4, 4
    mk = lambda: ref_vit.VisionTransformer(img_size=[112], patch_size=8, embed_dim=64, depth=2, num_heads=1, qkv_bias=True, drop_path_rate=0.0,
                                           norm_layer=lambda d: torch.nn.LayerNorm(d, eps=1e-6))
    student = ref_utils.MultiCropWrapper(mk(), ref_vit.DINOHead(64, K, use_bn=True, hidden_dim=128, bottleneck_dim=64, norm_last_layer=True))
    teacher = ref_utils.MultiCropWrapper(mk(), ref_vit.DINOHead(64, K, use_bn=True, hidden_dim=128, bottleneck_dim=64))
    perturb_bn(student.head)
    teacher.load_state_dict(student.state_dict())
    for p in teacher.parameters():
        p.requires_grad = False
    assert student.training and teacher.training
    crit = ref_lafs.DINOLoss(K, ncrops, 0.07, 0.04, 3, 10)
    groups = ref_utils.get_params_groups(student)
    opt = torch.optim.AdamW(groups)
    reg_ids = {id(p) for p in groups[0]["params"]}
    membership = {n: (id(p) in reg_ids) for n, p in student.named_parameters() if p.requires_grad}
    fx = {"init." + k: v.clone() for k, v in student.state_dict().items()}
    crops = [torch.randn(B, 3, s, s).clamp(-1, 1).half().float() for s in (112, 112, 48, 48)]
    fx.update({f"crop{i}": c.half() for i, c in enumerate(crops)})
    lrs, wds, moms = [5e-4, 4e-4], [0.04, 0.05], [0.9, 0.95]
    names = [n for n, p in student.named_parameters() if p.requires_grad]
    with bf16_linears(emulate):
        for step in range(2):
            epoch = step
            for i, g in enumerate(opt.param_groups):
                g["lr"] = lrs[step]
                if i == 0:
                    g["weight_decay"] = wds[step]
            t_out = teacher(crops[:2]); s_out = student(crops)
            loss = crit(s_out, t_out, epoch)
            opt.zero_grad()
            loss.backward()
            norms = ref_utils.clip_gradients(student, 3.0)
            post = {n: p.grad.clone() for n, p in student.named_parameters() if p.grad is not None}
            ref_utils.cancel_gradients_last_layer(epoch, student, 1)
            opt.step()
            with torch.no_grad():
                for pq, pk in zip(student.parameters(), teacher.parameters()):
                    pk.data.mul_(moms[step]).add_((1 - moms[step]) * pq.detach().data)
            fx.update({f"s{step}.loss": loss.detach(), f"s{step}.center": crit.center.clone(), f"s{step}.t_out": t_out.detach(),
                       f"s{step}.s_out": s_out.detach(), f"s{step}.norms": np.array(norms)})
            fx.update({f"s{step}.grad_post.{n}": g for n, g in post.items()})
            fx.update({f"s{step}.student.{k}": v.clone() for k, v in student.state_dict().items()})
            fx.update({f"s{step}.teacher.{k}": v.clone() for k, v in teacher.state_dict().items()})
            nd = dict(zip(names, norms))
            for k, scale in ZERO_SUM_STEP.items():              # (fp32 run only: a bf16-rounded incoming gradient no longer sums to zero)
                assert emulate or nd[k] < 1e-4 * nd[scale], (k, nd[k], nd[scale])
            for net in (student, teacher):
                for i in (1, 4):
                    assert int(net.head.mlp[i].num_batches_tracked) == step + 1
    fx["hyper"] = np.array([lrs, wds, moms])
    fx["norm_names"] = np.array(names)
    fx["membership_names"] = np.array(list(membership.keys()))
    fx["membership_reg"] = np.array(list(membership.values()))
    for n, reg in membership.items():                           # BatchNorm weight and bias are 1-D: the no-decay group
        if n.startswith(("head.mlp.1.", "head.mlp.4.")):
            assert not reg, n
    return fx


def rel(a, b):
    a, b = torch.as_tensor(a).double(), torch.as_tensor(b).double()
    return float((a - b).norm() / (b.norm() + 1e-30))


def worst(a, b, keys):
    return max(rel(b[k], a[k]) for k in keys)


def save_parts(name, fx):
    parts, room = [{}], PART_BYTES
    for k in sorted(fx):
        a = fx[k].detach().numpy() if isinstance(fx[k], torch.Tensor) else np.asarray(fx[k])
        if a.nbytes > room and parts[-1]:
            parts.append({}); room = PART_BYTES
        parts[-1][k] = fx[k]; room -= a.nbytes
    for i, part in enumerate(parts):
        save(name + (f"_{i}" if i else ""), **part)


def main():
    import torch.distributed as dist
    os.environ.setdefault("MASTER_ADDR", "127.0.0.1"); os.environ.setdefault("MASTER_PORT", "29551")
    dist.init_process_group("gloo", rank=0, world_size=1)            # DINOLoss.update_center all-reduces
    ref_utils, ref_vit, ref_lafs, _, _ = _import_reference()
    torch.set_num_threads(4)

    print("F29 DINO head with BatchNorm")
    a, b = run_f29(ref_vit, False), run_f29(ref_vit, True)
    floatbn = [k for k in BN_KEYS if not k.endswith("num_batches_tracked")]
    a["cond.out"] = np.float64(worst(a, b, [c + k for c in ("c0.", "c1.") for k in ("out", "out_e")]))
    a["cond.gx"] = np.float64(worst(a, b, [c + k for c in ("c0.", "c1.") for k in ("gx", "gx_e")]))
    a["cond.grad"] = np.float64(worst(a, b, [k for k in a if (".g." in k and not k.endswith(ZERO_SUM)) or ".ge." in k]))
    a["cond.buffers"] = np.float64(worst(a, b, [c + p + k for c in ("c0.", "c1.") for p in ("b1.", "b2.") for k in floatbn]))
    print("  " + ", ".join(f"{k} {float(a[k]):.3e}" for k in sorted(a) if k.startswith("cond.")))
    save_parts("f29_head_bn", a)

    print("F30 LAFS step x2, BatchNorm heads")
    a, b = run_f30(ref_utils, ref_vit, ref_lafs, False), run_f30(ref_utils, ref_vit, ref_lafs, True)
    zs = tuple(ZERO_SUM_STEP)
    a["cond.loss"] = np.float64(max(abs(float(b[f"s{s}.loss"]) - float(a[f"s{s}.loss"])) / float(a[f"s{s}.loss"]) for s in range(2)))
    a["cond.logits"] = np.float64(worst(a, b, [f"s{s}.{k}" for s in range(2) for k in ("s_out", "t_out")]))
    a["cond.grad"] = np.float64(worst(a, b, [k for k in a if ".grad_post." in k and not k.endswith(zs)]))
    a["cond.buffers"] = np.float64(worst(a, b, [f"s{s}.{w}.head.{k}" for s in range(2) for w in ("student", "teacher") for k in floatbn]))
    for s in range(2):
        print(f"  step {s}: " + ", ".join(f"{n} {v:.3e}" for n, v in (
            ("loss", abs(float(b[f's{s}.loss']) - float(a[f's{s}.loss'])) / float(a[f's{s}.loss'])),
            ("s_out", rel(b[f"s{s}.s_out"], a[f"s{s}.s_out"])), ("t_out", rel(b[f"s{s}.t_out"], a[f"s{s}.t_out"])),
            ("worst grad", worst(a, b, [k for k in a if k.startswith(f"s{s}.grad_post.") and not k.endswith(zs)])))))
    print("  " + ", ".join(f"{k} {float(a[k]):.3e}" for k in sorted(a) if k.startswith("cond.")))
    save_parts("f30_lafs_step_head_bn", a)
    dist.destroy_process_group()


if __name__ == "__main__":
    main()
