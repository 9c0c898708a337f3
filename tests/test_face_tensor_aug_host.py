"""CPU checks of the host side of the torchvision tensor chain (lafs_cvpr2024_amd/face_tensor_aug.py): the decisions equal those
of the torchvision 0.9.1 restatement in tests/facedataset_tv_oracle.py, draw for draw, and the oracle's own properties."""
import numpy as np
import pytest
import torch

import facedataset_tv_oracle as O
from lafs_cvpr2024_amd import face_tensor_aug as A


def _fields(rec):
    blend = [float(v) for v in rec["blend"]]
    erase = tuple(int(v) for v in rec["erase_box"]) if rec["erase"] else None
    return dict(crop=tuple(int(v) for v in rec["crop"]), order=[int(v) for v in rec["order"]], blend=blend,
                hue=float(rec["hue"]), erase=erase)


def _oracle_fields(p):
    blend = []
    for f in (p["brightness"], p["contrast"], p["saturation"]):
        blend += [float(np.float32(f)), float(np.float32(1.0 - f))]
    return dict(crop=tuple(p["crop"]), order=p["order"], blend=blend, hue=float(np.float32(p["hue"])), erase=p["erase"])


@pytest.mark.parametrize("seed", [0, 1, 7, 1234, 99991])
def test_sampler_equals_torchvision_draws(seed):
    aug = A.FaceTensorAug(seed)
    recs = aug.sample(1100)
    g = torch.Generator().manual_seed(seed)
    fallback = no_erase = 0
    for b in range(len(recs)):
        p = O.get_params(112, 112, g)
        assert _fields(recs[b]) == _oracle_fields(p), b
        fallback += p["crop"] == (0, 0, 112, 112)
        no_erase += p["erase"] is None
    assert fallback > 0 and no_erase > 0                       # both fallback paths occur in every seed's stream
    assert torch.equal(aug.gen.get_state(), g.get_state())     # the same number of draws, not just the same values


def test_generator_state_after_sample_equals_oracle():
    for B in (1, 3, 64):
        aug = A.FaceTensorAug(42)
        aug.sample(B)
        g = torch.Generator().manual_seed(42)
        for _ in range(B):
            O.get_params(112, 112, g)
        assert torch.equal(aug.gen.get_state(), g.get_state())


def test_boxes_inside_image_and_fallback_rate():
    recs = A.FaceTensorAug(3).sample(6000)
    c, e = recs["crop"], recs["erase_box"]
    assert (c[:, 0] >= 0).all() and (c[:, 1] >= 0).all() and (c[:, 0] + c[:, 2] <= 112).all() and (c[:, 1] + c[:, 3] <= 112).all()
    assert (c[:, 2] >= 100).all() and (c[:, 3] >= 100).all()  # scale (0.9, 1) and ratio (3/4, 4/3): no antialias question
    on = recs["erase"] == 1
    assert (e[on, 2] >= 1).all() and (e[on, 3] >= 1).all()
    assert (e[on, 0] + e[on, 2] <= 112).all() and (e[on, 1] + e[on, 3] <= 112).all()
    assert (e[~on] == 0).all()
    full = ((c[:, 2] == 112) & (c[:, 3] == 112)).mean()
    assert 0.06 < full < 0.14, full                            # ~10 % of the draws end in the whole-image fallback
    assert 0.45 < on.mean() < 0.55
    A.check_records(recs, 6000, 112, 112)


def test_check_records_rejects_bad_boxes():
    recs = A.FaceTensorAug(0).sample(4)
    bad = recs.copy(); bad["crop"][1] = (20, 0, 100, 100)
    with pytest.raises(ValueError):
        A.check_records(bad, 4, 112, 112)
    bad = recs.copy(); bad["order"][2] = (0, 0, 1, 2)
    with pytest.raises(ValueError):
        A.check_records(bad, 4, 112, 112)
    bad = recs.copy(); bad["erase"][0] = 1; bad["erase_box"][0] = (100, 0, 20, 5)
    with pytest.raises(ValueError):
        A.check_records(bad, 4, 112, 112)


def test_sample_draws_for_non_square_sources():
    aug = A.FaceTensorAug(5)
    recs = aug.sample(500, 96, 112)
    g = torch.Generator().manual_seed(5)
    for b in range(500):
        p = O.get_params(96, 112, g)
        assert _fields(recs[b]) == _oracle_fields(p)


def _img(seed):
    return torch.from_numpy(np.random.RandomState(seed).randint(0, 256, (3, 112, 112)).astype(np.uint8))


def test_oracle_unit_factors_are_identities():
    for s in range(4):
        x = _img(s)
        assert torch.equal(O.adjust_brightness(x, 1.0), x)
        assert torch.equal(O.adjust_contrast(x, 1.0), x)
        assert torch.equal(O.adjust_saturation(x, 1.0), x)
        assert torch.equal(O.resize(x, 112), x)               # the whole-image crop is an exact copy


def test_oracle_hue_zero_is_not_an_identity():
    """Documented, not assumed: hue 0 goes through x / 255 -> hsv -> rgb -> (x * 255).to(uint8); the truncating cast turns a
    value a hair below an integer into the integer below, so a zero hue shift changes some pixels by -1 (never by more, never up)."""
    x = _img(0)
    y = O.adjust_hue(x, 0.0)
    d = y.to(torch.int32) - x.to(torch.int32)
    assert d.min().item() >= -1 and d.max().item() == 0
    assert (d != 0).any()
    gray = x[:1].expand(3, -1, -1).contiguous()
    assert torch.equal(O.adjust_hue(gray, 0.05), O.adjust_hue(gray, 0.0))   # maxc == minc: hue is irrelevant


def test_oracle_apply_shapes_and_erase():
    x = _img(1)
    p = O.get_params(112, 112, torch.Generator().manual_seed(0))
    p["erase"] = (0, 0, 5, 7)
    y = O.apply(x, p)
    assert y.shape == (3, 112, 112) and y.dtype == torch.uint8
    assert (y[:, :5, :7] == 0).all()


def test_symbol_is_bound():
    from lafs_cvpr2024_amd import _lib
    assert "lafs_face_tensor_aug" in _lib.EXPORTED
    assert A.RECORD.itemsize == 80
