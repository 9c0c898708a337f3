"""fViT (ViTs_face_overlap) on the HIP path against the reference's fp32 CPU results in the F26 fixture (tools/make_golden_fvit.py).

Gates are relative-L2 per tensor, 2x the worst value observed on MI355X per tensor group (DESIGN.md section 2 has the table):
                                                   observed   gate
  z (training list forward, groups of 4 and 6)     9.3e-3     1.9e-2
  parameter gradients (27 tensors)                 2.8e-2     5.6e-2    (layers.1.0.fn.fn.to_out.0.bias)
  last block's fc2 bias gradient (see below)       9.6e-3     1.9e-2
  x112_a.grad                                      2.2e-2     4.4e-2
  running_mean / running_var                       2.9e-3     5.8e-3    (running_var 3.1e-5)
  eval features, pad 4 / pad 2                     5.2e-3     1.05e-2
The yardstick is always the fixture, never this build's own output.

One tensor has no relative error: the gradient of the LAST block's fc2 bias is the column sum of the gradient entering the cls rows,
i.e. of the BatchNorm input gradient, and in training mode that sum vanishes identically (sum_r dx_r = 0 per column and group).  The
fixture holds the reference's fp32 rounding residue (norm 2.6e-4 where its neighbours have 2e1 .. 3e2); this build sums the bf16
gradient operand of the weight-gradient GEMM and leaves the bf16 residue (norm 0.62).  Its error is therefore taken against the norm of
the same stream's sum one residual branch earlier, where nothing cancels (the reference's layers.1.0.fn.fn.to_out.0.bias gradient), and
the test first checks on the reference's own numbers that the tensor does vanish."""
import pytest
import torch
import torch.nn.functional as F

pytestmark = pytest.mark.gpu

from conftest import gate_errors, sub  # noqa: E402
from fvit_cases import FVIT_CFG, load_fvit  # noqa: E402
from lafs_cvpr2024_amd.face_pre_pro.ViT_face import ViTs_face_overlap  # noqa: E402
from lafs_cvpr2024_amd.vision_transformer import attach_arena  # noqa: E402

DEV = "cuda"
GATE_Z, GATE_GRAD, GATE_GX, GATE_BN, GATE_EVAL, GATE_ZERO_SUM = 1.9e-2, 5.6e-2, 4.4e-2, 5.8e-3, 1.05e-2, 1.9e-2
ZERO_SUM, ZERO_SUM_SCALE = "transformer.layers.1.1.fn.fn.net.3.bias", "transformer.layers.1.0.fn.fn.to_out.0.bias"

_FX = {}


def fixture():
    if not _FX:
        _FX.update(load_fvit())
    return _FX


def rel_l2(a, b):
    a, b = a.detach().double().cpu(), b.detach().double().cpu()
    return ((a - b).norm() / (b.norm() + 1e-30)).item()


def model(pad=4, state=None, **kw):
    fx = fixture()
    m = ViTs_face_overlap(pad=pad, drop_path_rate=0.0, **{**FVIT_CFG, **kw})
    m.load_state_dict(sub(fx, "p.") if state is None else state, strict=True)
    attach_arena(m, DEV)
    return m


def crops(fx):
    return [fx[f"x{i}"].float().to(DEV) for i in range(5)]


def bits(t):
    return t.detach().contiguous().view(torch.int32).cpu()


def test_state_dict_keys_and_strict_load():
    fx = fixture()
    m = ViTs_face_overlap(pad=4, **FVIT_CFG)
    sd = m.state_dict()
    assert set(sd) == set(sub(fx, "p."))
    assert all(tuple(sd[k].shape) == tuple(v.shape) for k, v in sub(fx, "p.").items())
    m.load_state_dict(sub(fx, "p."), strict=True)


def test_training_list_forward_and_backward_against_the_reference():
    fx = fixture()
    m = model()
    m.train()
    xs = crops(fx)
    xs[0].requires_grad_(True)
    z = m(xs)
    assert z.shape == fx["z"].shape
    (z * fx["w"].to(DEV)).sum().backward()
    bn = m.mlp_head[0]
    params = dict(m.named_parameters())
    ref_g = sub(fx, "g.")
    assert set(ref_g) == set(params)
    errs_g = {k: rel_l2(params[k].grad, g) for k, g in ref_g.items() if k != ZERO_SUM}
    # the identically vanishing sum (module docstring): the reference confirms it vanishes; error against the neighbouring sum's norm
    scale = float(ref_g[ZERO_SUM_SCALE].double().norm())
    assert float(ref_g[ZERO_SUM].double().norm()) < 1e-4 * scale
    e_zero = float((params[ZERO_SUM].grad.detach().double().cpu() - ref_g[ZERO_SUM].double()).norm()) / scale
    # (measure everything before any gate fires)
    e_z, e_gx = rel_l2(z, fx["z"]), rel_l2(xs[0].grad, fx["gx112_a"])
    e_bn = {k: rel_l2(getattr(bn, k), fx["bn." + k]) for k in ("running_mean", "running_var")}
    print(f"[F26] z {e_z:.3e}, gx112_a {e_gx:.3e}, running_mean {e_bn['running_mean']:.3e}, running_var {e_bn['running_var']:.3e}, "
          f"worst gradient {max(errs_g.values()):.3e} at {max(errs_g, key=errs_g.get)}")
    for k in sorted(errs_g, key=errs_g.get)[-4:]:
        print(f"[F26]   grad {k}: {errs_g[k]:.3e}")
    gate_errors("F26 fViT z", {"z": e_z}, GATE_Z)
    gate_errors("F26 fViT parameter gradients", errs_g, GATE_GRAD)
    gate_errors("F26 fViT vanishing fc2-bias gradient (absolute, over the neighbouring sum's norm)", {ZERO_SUM: e_zero}, GATE_ZERO_SUM)
    gate_errors("F26 fViT input gradient", {"gx112_a": e_gx}, GATE_GX)
    gate_errors("F26 fViT BatchNorm buffers", e_bn, GATE_BN)
    assert int(bn.num_batches_tracked) == 2 == int(fx["bn.num_batches_tracked"])


@pytest.mark.parametrize("pad,xk,zk", [(4, "xe", "ze"), (2, "xe2", "ze2")])
def test_eval_features_against_the_reference(pad, xk, zk):
    fx = fixture()
    state = dict(sub(fx, "p."))
    state.update({"mlp_head.0." + k: fx["bn." + k] for k in ("running_mean", "running_var", "num_batches_tracked")})
    m = model(pad=pad, state=state)
    m.eval()
    bn = m.mlp_head[0]
    before = (bits(bn.running_mean), bits(bn.running_var), int(bn.num_batches_tracked))
    with torch.no_grad():
        e = m(fx[xk].float().to(DEV), for_fea=True)
    gate_errors(f"F26 fViT eval pad {pad}", {zk: rel_l2(e, fx[zk])}, GATE_EVAL)
    assert torch.equal(before[0], bits(bn.running_mean)) and torch.equal(before[1], bits(bn.running_var))
    assert before[2] == int(bn.num_batches_tracked)


def test_tensor_and_one_element_list_give_the_same_bits():
    fx = fixture()
    x = crops(fx)[0]
    a, b = model(), model()
    a.train(); b.train()
    with torch.no_grad():
        za, zb = a(x), b([x])
    assert torch.equal(bits(za), bits(zb))
    assert torch.equal(bits(a.mlp_head[0].running_var), bits(b.mlp_head[0].running_var))


def test_list_forward_is_the_groups_run_one_after_the_other():
    """Bits of the outputs and of the running statistics: the statistics are per group and updated in list order."""
    fx = fixture()
    xs = crops(fx)
    a, b = model(), model()
    a.train(); b.train()
    with torch.no_grad():
        h, z = a(xs, return_before_head=True)
        z1 = b.forward_features(torch.cat(xs[:2]))
        mid = bits(b.mlp_head[0].running_mean)
        z2 = b.forward_features(torch.cat(xs[2:]))
    assert torch.equal(bits(h), bits(z)) and torch.equal(bits(z), bits(torch.cat((z1, z2))))
    for k in ("running_mean", "running_var"):
        assert torch.equal(bits(getattr(a.mlp_head[0], k)), bits(getattr(b.mlp_head[0], k)))
    assert not torch.equal(mid, bits(b.mlp_head[0].running_mean))            # (the second group did update them)
    assert int(a.mlp_head[0].num_batches_tracked) == int(b.mlp_head[0].num_batches_tracked) == 2
    a.pred = torch.nn.Identity()
    a.eval()
    with torch.no_grad():
        assert a(xs).shape == z.shape                                        # forward_head applies `pred` when set


def test_3d_window_vectors_equal_the_image():
    """A [2, 196, 432] input made with F.unfold on the CPU against the 4-D image.  The only difference between the two paths could be
    the bf16 rounding of the input -- and both round the SAME fp32 window values to bf16 once (lafs_unfold_bf16 / lafs_pad_cast_bf16),
    so the gate is zero: the features must agree bit for bit."""
    fx = fixture()
    x = fx["x0"].float()
    x3 = F.unfold(x, 12, stride=8, padding=4).transpose(1, 2).contiguous()
    assert x3.shape == (2, 196, 432)
    m = model()
    m.eval()
    with torch.no_grad():
        e4, e3 = m(x.to(DEV), for_fea=True), m(x3.to(DEV), for_fea=True)
    assert torch.equal(bits(e4), bits(e3))
    m.train()                                                                # and its gradient is the slice of the window gradient
    x3g = x3.to(DEV).requires_grad_(True)
    m(x3g).sum().backward()
    assert x3g.grad.shape == x3g.shape and bool(torch.isfinite(x3g.grad).all())


def test_guards():
    for kw in (dict(pool="mean"), dict(channels=1), dict(dim_head=32)):
        with pytest.raises(NotImplementedError):
            ViTs_face_overlap(pad=4, **{**FVIT_CFG, **kw})
    fx = fixture()
    m = model()
    x = crops(fx)[0]
    with pytest.raises(NotImplementedError):
        m.forward_features(x, mask=torch.ones(1, device=DEV))
    with pytest.raises(NotImplementedError):
        m.forward_features(x, label=torch.zeros(2, dtype=torch.long, device=DEV))
    with pytest.raises(NotImplementedError):
        m(x, patch_drop=0.5)
    m.eval()
    with torch.no_grad():
        assert m.forward_features(x, patch_drop=None).shape == (2, 128)       # None counts as 0
        assert m(x[:1], for_fea=True).shape == (1, 128)                       # one image is fine in eval mode
    m.train()
    with pytest.raises(ValueError, match="Expected more than 1 value per channel"):
        m(x[:1])
    with pytest.raises(ValueError, match="position table"):
        m(torch.zeros(2, 3, 128, 128, device=DEV))                            # 16 x 16 windows > (112 // 8) ** 2
