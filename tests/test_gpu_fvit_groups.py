"""fViT's packed pass over several crop groups (ViTs_face_overlap.forward_groups: one trunk pass, the BatchNorm1d head per group
through lafs_bn1d_groups_fwd / _bwd) against the reference's fp32 CPU results in the F26 fixture.

The reference ran forward([x0 .. x4]), i.e. the groups cat(x0, x1) (4 rows, 112 px) and cat(x2, x3, x4) (6 rows, 48 px) one after the
other; the packed pass must give the same z, gradients and BatchNorm buffers.  The gates are those of tests/test_gpu_fvit.py (its
docstring and DESIGN.md section 2 hold the observed values): they are the project's own numbers for exactly these groups, and the last
block's fc2-bias gradient -- which vanishes identically under a training BatchNorm -- is treated as that file treats it."""
import pytest
import torch

pytestmark = pytest.mark.gpu

from conftest import gate_errors, sub  # noqa: E402
from fvit_cases import FVIT_CFG, load_fvit  # noqa: E402
from lafs_cvpr2024_amd.face_pre_pro.ViT_face import ViTs_face_overlap  # noqa: E402
from lafs_cvpr2024_amd.utils import MultiCropWrapper  # noqa: E402
from lafs_cvpr2024_amd.vision_transformer import attach_arena  # noqa: E402

DEV = "cuda"
GATE_Z, GATE_GRAD, GATE_GX, GATE_BN, GATE_ZERO_SUM = 1.9e-2, 5.6e-2, 4.4e-2, 5.8e-3, 1.9e-2      # tests/test_gpu_fvit.py
ZERO_SUM, ZERO_SUM_SCALE = "transformer.layers.1.1.fn.fn.net.3.bias", "transformer.layers.1.0.fn.fn.to_out.0.bias"

_FX = {}


def fixture():
    if not _FX:
        _FX.update(load_fvit())
    return _FX


def rel_l2(a, b):
    a, b = a.detach().double().cpu(), b.detach().double().cpu()
    return ((a - b).norm() / (b.norm() + 1e-30)).item()


def bits(t):
    return t.detach().contiguous().view(torch.int32).cpu()


def model(wrap=False):
    m = ViTs_face_overlap(pad=4, drop_path_rate=0.0, **FVIT_CFG)
    m.load_state_dict(sub(fixture(), "p."), strict=True)
    if wrap:
        m = MultiCropWrapper(m, torch.nn.Identity())
    attach_arena(m, DEV)
    return m


def crops(fx):
    return [fx[f"x{i}"].float().to(DEV) for i in range(5)]


def test_packed_groups_forward_and_backward_against_the_reference():
    fx = fixture()
    m = model()
    m.train()
    xs = crops(fx)
    xs[0].requires_grad_(True)
    z = m.forward_groups([torch.cat(xs[:2]), torch.cat(xs[2:])])
    assert z.shape == fx["z"].shape
    (z * fx["w"].to(DEV)).sum().backward()
    bn = m.mlp_head[0]
    params = dict(m.named_parameters())
    ref_g = sub(fx, "g.")
    assert set(ref_g) == set(params)
    errs_g = {k: rel_l2(params[k].grad, g) for k, g in ref_g.items() if k != ZERO_SUM}
    scale = float(ref_g[ZERO_SUM_SCALE].double().norm())
    assert float(ref_g[ZERO_SUM].double().norm()) < 1e-4 * scale             # the reference confirms that the sum vanishes
    e_zero = float((params[ZERO_SUM].grad.detach().double().cpu() - ref_g[ZERO_SUM].double()).norm()) / scale
    e_z, e_gx = rel_l2(z, fx["z"]), rel_l2(xs[0].grad, fx["gx112_a"])
    e_bn = {k: rel_l2(getattr(bn, k), fx["bn." + k]) for k in ("running_mean", "running_var")}
    print(f"[F26 packed] z {e_z:.3e}, gx112_a {e_gx:.3e}, running_mean {e_bn['running_mean']:.3e}, running_var {e_bn['running_var']:.3e}, "
          f"vanishing sum {e_zero:.3e}, worst gradient {max(errs_g.values()):.3e} at {max(errs_g, key=errs_g.get)}")
    gate_errors("F26 packed fViT z", {"z": e_z}, GATE_Z)
    gate_errors("F26 packed fViT parameter gradients", errs_g, GATE_GRAD)
    gate_errors("F26 packed fViT vanishing fc2-bias gradient (absolute, over the neighbouring sum's norm)", {ZERO_SUM: e_zero},
                GATE_ZERO_SUM)
    gate_errors("F26 packed fViT input gradient", {"gx112_a": e_gx}, GATE_GX)
    gate_errors("F26 packed fViT BatchNorm buffers", e_bn, GATE_BN)
    assert int(bn.num_batches_tracked) == 2 == int(fx["bn.num_batches_tracked"])


def test_one_group_is_forward_features_bit_for_bit():
    x = torch.cat(crops(fixture())[:2])
    a, b = model(), model()
    a.train(); b.train()
    with torch.no_grad():
        za, zb = a.forward_groups([x]), b.forward_features(x)
    assert torch.equal(bits(za), bits(zb))
    assert torch.equal(bits(a.mlp_head[0].running_var), bits(b.mlp_head[0].running_var))
    assert int(a.mlp_head[0].num_batches_tracked) == 1


def test_eval_groups_leave_the_buffers_alone():
    xs = crops(fixture())
    m = model()
    m.eval()
    bn = m.mlp_head[0]
    before = (bits(bn.running_mean), bits(bn.running_var))
    with torch.no_grad():
        z = m.forward_groups([torch.cat(xs[:2]), xs[2][:1]])                 # eval takes a group of one image
    assert z.shape == (5, FVIT_CFG["dim"]) and bool(torch.isfinite(z).all())
    assert torch.equal(before[0], bits(bn.running_mean)) and torch.equal(before[1], bits(bn.running_var))
    assert int(bn.num_batches_tracked) == 0
    m.train()
    with pytest.raises(ValueError, match="Expected more than 1 value per channel"):
        m.forward_groups([torch.cat(xs[:2]), xs[2][:1]])


def test_multicrop_wrapper_takes_the_packed_pass():
    xs = crops(fixture())
    w, twin = model(wrap=True), model()
    w.train(); twin.train()
    seen = []
    packed = w.backbone.forward_groups
    w.backbone.forward_groups = lambda groups: (seen.append([tuple(g.shape) for g in groups]), packed(groups))[1]
    with torch.no_grad():
        out = w(xs)
        ref = twin.forward_groups([torch.cat(xs[:2]), torch.cat(xs[2:])])
    assert seen == [[(4, 3, 112, 112), (6, 3, 48, 48)]]
    assert torch.equal(bits(out), bits(ref))
    for k in ("running_mean", "running_var"):
        assert torch.equal(bits(getattr(w.backbone.mlp_head[0], k)), bits(getattr(twin.mlp_head[0], k)))
    assert int(w.backbone.mlp_head[0].num_batches_tracked) == 2
