"""DINOHead(use_bn=True) under autograd against the reference's own head in the F29 fixture (tools/make_golden_head_bn.py): a training
forward + backward, the BatchNorm buffers behind one and two training forwards, and an eval forward + backward; both norm_last_layer
cases.  The yardstick is the fixture; the gates are 2x the worst error observed on MI355X per tensor group, and `cond.*` -- how far the
reference itself moves when only its nn.Linear operands are rounded to bf16 -- stands next to them (rel-L2, worst of both cases):
                                        observed    gate      cond.*
  out (train / eval)                    5.15e-3     1.03e-2   5.17e-3
  gx  (train / eval)                    6.50e-3     1.30e-2   6.50e-3
  parameter gradients (train / eval)    6.98e-3     1.40e-2   6.97e-3   (mlp.1.bias, training)
  running_mean / running_var            2.70e-3     5.4e-3    2.70e-3   (mlp.1.running_mean behind two forwards)
The observed values ARE the cond figures to within a few per cent: what separates this head from the reference's is the bf16 rounding of
the Linear operands, the fused BatchNorm + GELU kernels add nothing that shows at this level.  The gradients of mlp.0.bias and mlp.3.bias are left out of the training-mode
gradient gate and nothing else is: in front of a training-mode BatchNorm they are column sums that vanish identically (the fixture's
own are below 1e-4 of the weight gradient, checked here); in eval mode they are compared like every other tensor."""
import pytest
import torch

pytestmark = pytest.mark.gpu

from conftest import gate_errors, load_golden, sub  # noqa: E402
import head_bn_cases as hc  # noqa: E402
from lafs_cvpr2024_amd import _lib, functional as Fn, ops  # noqa: E402
from lafs_cvpr2024_amd import vision_transformer as vits  # noqa: E402

DEV = "cuda"
GATE_OUT, GATE_GX, GATE_GRAD, GATE_BUF = 1.03e-2, 1.30e-2, 1.40e-2, 5.4e-3


def rel_l2(a, b):
    a, b = a.detach().double().cpu(), b.detach().double().cpu()
    return ((a - b).norm() / (b.norm() + 1e-30)).item()


def buffers(head):
    return {k: head.state_dict()[k] for k in hc.HEAD_BN_KEYS}


@pytest.mark.parametrize("case,norm_last", [("c0.", True), ("c1.", False)], ids=["norm_last_layer", "free_weight_g"])
def test_f29_head_with_batchnorm(case, norm_last):
    fx = sub(hc.load_f29(), case)
    cond = {k: float(v) for k, v in hc.load_f29().items() if k.startswith("cond.")}
    h = vits.DINOHead(norm_last_layer=norm_last, **hc.F29_HEAD)
    h.load_state_dict(sub(fx, "p."), strict=True)
    vits.attach_arena(h, DEV)
    params = dict(h.named_parameters())
    seen = dict(out={}, gx={}, grad={}, buf={})
    w = fx["w"].to(DEV)
    # ---- training forward + backward
    assert h.training
    x = fx["x"].to(DEV).requires_grad_(True)
    out = h(x)
    assert out.shape == (16, 1000)
    (out * w).sum().backward()
    seen["out"]["train"], seen["gx"]["train"] = rel_l2(out, fx["out"]), rel_l2(x.grad, fx["gx"])
    ref_g = sub(fx, "g.")
    for k in hc.ZERO_SUM:                                                     # the reference confirms that these sums vanish
        assert float(ref_g[k].double().norm()) < 1e-4 * float(ref_g[k.replace("bias", "weight")].double().norm())
    seen["grad"].update({"train." + k: rel_l2(params[k].grad, g) for k, g in ref_g.items() if k not in hc.ZERO_SUM})
    assert set(ref_g) == {k for k, p in params.items() if p.requires_grad}
    b1 = buffers(h)
    seen["buf"].update({"b1." + k: rel_l2(b1[k], fx["b1." + k]) for k in hc.HEAD_BN_KEYS if not k.endswith("num_batches_tracked")})
    assert int(b1["mlp.1.num_batches_tracked"]) == 1 and int(b1["mlp.4.num_batches_tracked"]) == 1
    # ---- a second training forward on new rows
    with torch.no_grad():
        h(fx["x2"].to(DEV))
    b2 = {k: v.clone() for k, v in buffers(h).items()}
    seen["buf"].update({"b2." + k: rel_l2(b2[k], fx["b2." + k]) for k in hc.HEAD_BN_KEYS if not k.endswith("num_batches_tracked")})
    assert int(b2["mlp.1.num_batches_tracked"]) == 2 and int(b2["mlp.4.num_batches_tracked"]) == 2
    # ---- eval forward + backward: running statistics, buffers untouched
    h.eval()
    h._arena.zero_grad()
    xe = fx["xe"].to(DEV).requires_grad_(True)
    out_e = h(xe)
    (out_e * w).sum().backward()
    seen["out"]["eval"], seen["gx"]["eval"] = rel_l2(out_e, fx["out_e"]), rel_l2(xe.grad, fx["gx_e"])
    seen["grad"].update({"eval." + k: rel_l2(params[k].grad, g) for k, g in sub(fx, "ge.").items()})
    for k, v in buffers(h).items():
        assert torch.equal(v.cpu(), b2[k].cpu()), f"{k} moved in eval mode"
    if norm_last:
        assert h.last_layer.weight_g.grad is None or float(h.last_layer.weight_g.grad.abs().max()) == 0.0
    for grp, c in (("out", "cond.out"), ("gx", "cond.gx"), ("grad", "cond.grad"), ("buf", "cond.buffers")):
        k = max(seen[grp], key=seen[grp].get)
        print(f"[F29 {case}] {grp}: worst {seen[grp][k]:.3e} at {k}; {c} {cond[c]:.3e}")
    gate_errors("F29 head output", seen["out"], GATE_OUT)
    gate_errors("F29 head input gradient", seen["gx"], GATE_GX)
    gate_errors("F29 head parameter gradients", seen["grad"], GATE_GRAD)
    gate_errors("F29 head BatchNorm buffers", seen["buf"], GATE_BUF)


def test_one_row_in_training_mode_is_refused():
    h = vits.DINOHead(**hc.F29_HEAD)
    vits.attach_arena(h, DEV)
    with pytest.raises(_lib.LafsHipError, match="more than one row"):
        h(torch.randn(1, 128, device=DEV))
    assert int(h.mlp[1].num_batches_tracked) == 0
    h.eval()
    with torch.no_grad():
        assert bool(torch.isfinite(h(torch.randn(1, 128, device=DEV))).all())


def test_plain_head_is_bit_equal_to_its_kernel_sequence():
    """use_bn=False: the module's output on F2 carries the bits of the launch sequence the plain head has always run -- written out
    here from ops, not taken from head_forward, so that the branch that selects the BatchNorm form cannot have changed it."""
    fx = load_golden("f2_head")
    h = vits.DINOHead(128, 1000, hidden_dim=256, bottleneck_dim=64)
    h.load_state_dict(sub(fx, "p."))
    a = vits.attach_arena(h, DEV)
    assert not h.use_bn and not Fn.head_has_bn(a, "")
    x = fx["x"].to(DEV)
    with torch.no_grad():
        out = h(x)
    m = lambda k: a.view(a.master, k)
    x_bf = ops.scale_cast_bf16(x.contiguous())
    _, a1 = ops.gemm_nt(x_bf, a.bf("mlp.0.weight"), _lib.EPI_BF16_GELU, bias=m("mlp.0.bias"))
    _, a2 = ops.gemm_nt(a1, a.bf("mlp.2.weight"), _lib.EPI_BF16_GELU, bias=m("mlp.2.bias"))
    z = ops.gemm_nt(a2, a.bf("mlp.4.weight"), _lib.EPI_F32, bias=m("mlp.4.bias"))
    zn = torch.empty(6, 64, device=DEV, dtype=torch.bfloat16)
    inv_z = torch.empty(6, device=DEV)
    ops.call("lafs_l2norm_fwd", ops._p(z), 64, ops._p(zn), 64, ops._p(inv_z), 6, 64)
    wn = torch.empty(1024, 64, device=DEV, dtype=torch.bfloat16)
    inv_v = torch.empty(1000, device=DEV)
    ops.call("lafs_weightnorm_fwd", ops._p(m("last_layer.weight_v")), ops._p(m("last_layer.weight_g")), 1000, 1024, 64, ops._p(wn), None, 1024,
             ops._p(inv_v))
    want = ops.gemm_nt(zn, wn, _lib.EPI_F32, n_cols=1024)[:, :1000]
    assert torch.equal(out.contiguous().view(torch.int32).cpu(), want.contiguous().view(torch.int32).cpu())
    _, st = Fn.head_forward(a, "", x, 1000, save=True)
    assert st.u1.dtype == torch.bfloat16 and not st.bn
