"""CPU: the DINO-face views (DataAugmentationDINO, reference lafs_train.py:743-788) -- the test-side oracle against Pillow itself
at both output sizes (112 global, 48 local), the 48-output coefficient table, the parameter sampler's distributions, and the
argument checks of lafs_dino_views / --views dino that need no device."""
import ctypes as C
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(__file__))
PIL = pytest.importorskip("PIL")
from PIL import Image, ImageEnhance, ImageFilter, ImageOps  # noqa: E402

import dino_views_oracle as D  # noqa: E402
from lafs_cvpr2024_amd import augment as aug  # noqa: E402
from oracle import augment as A  # noqa: E402

# (i, j, h, w): whole image; 48x48 (both passes skipped at 48); 48 wide (no horizontal pass at 48); 48 high (no vertical pass at
# 48); a near miss of both; one pixel; an upsample at both sizes; a box that ends at row and column 112
BOXES = [(0, 0, 112, 112), (10, 20, 48, 48), (5, 9, 100, 48), (30, 1, 48, 110), (33, 2, 47, 110), (50, 60, 1, 1), (40, 33, 30, 21),
         (75, 53, 37, 59)]


def _img(seed, smooth=True):
    return D.images(1, seed)[0] if smooth else np.random.RandomState(seed).randint(0, 256, (112, 112, 3)).astype(np.uint8)


def _pil_hue(pil, hue_factor):
    """torchvision F_pil.adjust_hue."""
    h, s, v = pil.convert("HSV").split()
    np_h = np.array(h, dtype=np.uint8)
    with np.errstate(over="ignore"):
        np_h += np.array(int(hue_factor * 255)).astype(np.uint8)
    return Image.merge("HSV", (Image.fromarray(np_h, "L"), s, v)).convert("RGB")


def _pil_view(img, p, size):
    """The view of one record from the Pillow calls torchvision makes, in DataAugmentationDINO's order."""
    q = Image.fromarray(img).crop((p["j"], p["i"], p["j"] + p["w"], p["i"] + p["h"])).resize((size, size), Image.BICUBIC)
    if p["flip"]:
        q = q.transpose(Image.FLIP_LEFT_RIGHT)
    if p["jitter"]:
        f = p["factors"]
        ops = (lambda x: ImageEnhance.Brightness(x).enhance(f[0]), lambda x: ImageEnhance.Contrast(x).enhance(f[1]),
               lambda x: ImageEnhance.Color(x).enhance(f[2]), lambda x: _pil_hue(x, f[3]))
        for fn in p["order"]:
            q = ops[fn](q)
    if p["gray"]:
        q = Image.merge("RGB", [q.convert("L")] * 3)
    if p["blur_radius"] > 0:
        q = q.filter(ImageFilter.GaussianBlur(p["blur_radius"]))
    if p["solarize"]:
        q = ImageOps.solarize(q, 128)
    return np.asarray(q)


@pytest.mark.parametrize("size", [48, 112])
@pytest.mark.parametrize("box", BOXES)
def test_oracle_resized_crop_is_pillows(box, size):
    i, j, h, w = box
    for img in (_img(1), _img(2, smooth=False)):
        ref = np.asarray(Image.fromarray(img).crop((j, i, j + w, i + h)).resize((size, size), Image.BICUBIC))
        assert np.array_equal(A.resized_crop(img, i, j, h, w, size), ref)


@pytest.mark.parametrize("size", [48, 112])
def test_oracle_colour_pieces_are_pillows(size):
    img = A.resized_crop(_img(3), 3, 5, 101, 97, size)
    pil = Image.fromarray(img)
    assert np.array_equal(A.hflip(img), np.asarray(pil.transpose(Image.FLIP_LEFT_RIGHT)))
    for f in (0.61, 1.0, 1.39):
        assert np.array_equal(A.adjust_brightness(img, f), np.asarray(ImageEnhance.Brightness(pil).enhance(f)))
        assert np.array_equal(A.adjust_contrast(img, f), np.asarray(ImageEnhance.Contrast(pil).enhance(f)))
        assert np.array_equal(A.adjust_saturation(img, 1 + (f - 1) / 2), np.asarray(ImageEnhance.Color(pil).enhance(1 + (f - 1) / 2)))
    for hf in (-0.1, 0.037, 0.1):
        assert np.array_equal(A.adjust_hue(img, hf), np.asarray(_pil_hue(pil, hf)))
    assert np.array_equal(A.to_grayscale3(img), np.asarray(Image.merge("RGB", [pil.convert("L")] * 3)))
    for r in (0.1, 0.7, 1.3, 2.0):
        assert np.array_equal(A.gaussian_blur(img, r), np.asarray(pil.filter(ImageFilter.GaussianBlur(r))))
    assert np.array_equal(A.solarize(img), np.asarray(ImageOps.solarize(pil, 128)))


@pytest.mark.parametrize("size", [48, 112])
@pytest.mark.parametrize("box", BOXES)
def test_oracle_composed_chain_is_pillows(box, size):
    i, j, h, w = box
    img = _img(4)
    for n, p in enumerate((
            dict(flip=True, jitter=True, order=[3, 1, 0, 2], factors=[0.61, 1.39, 0.8, -0.1], gray=False, blur_radius=2.0, solarize=True),
            dict(flip=False, jitter=True, order=[0, 1, 2, 3], factors=[1.39, 0.61, 1.2, 0.1], gray=True, blur_radius=0.1, solarize=False),
            dict(flip=True, jitter=False, order=[0, 1, 2, 3], factors=[1, 1, 1, 0], gray=False, blur_radius=0.0, solarize=False))):
        p = dict(p, i=i, j=j, h=h, w=w)
        u8 = D.view_u8(img, p, size)
        assert np.array_equal(u8, _pil_view(img, p, size)), (n, p)
        for mean, std in (D.IMAGENET, D.HALF):
            ref = (np.asarray(u8).astype(np.float32) / np.float32(255) - np.asarray(mean, np.float32)) / np.asarray(std, np.float32)
            got = D.normalize(u8, mean, std)
            assert got.dtype == np.float32 and got.shape == (3, size, size) and np.array_equal(got, ref.transpose(2, 0, 1))


def test_make_views_orders_and_sizes_the_crops():
    rng = np.random.RandomState(0)
    crops = aug.sample_dino_params(rng, 3)
    g, l = D.make_views(_img(5), crops, *D.IMAGENET)
    assert [v.shape for v in g] == [(3, 112, 112)] * 2 and [v.shape for v in l] == [(3, 48, 48)] * 3
    assert np.array_equal(l[1], D.normalize(D.view_u8(_img(5), crops[3], 48), *D.IMAGENET))


# ------------------------------------------------------------------------------------------------ coefficient tables
def test_local_coefficient_table_matches_oracle_and_holds_ten_taps():
    tab = aug.coeff_table(112, 48)
    assert tab.shape[:2] == (113, 48) and tab.shape[2] - 2 >= 10 and tab.dtype == np.int32
    assert tab[1:, :, 1].max() == 10                                     # 112 -> 48: support 2 * 112 / 48 on either side
    for n in (1, 2, 5, 21, 47, 48, 49, 82, 111, 112):
        for xx, (xmin, k) in enumerate(A.resample_coeffs(n, 48)):
            assert tab[n, xx, 0] == xmin and tab[n, xx, 1] == len(k) and list(tab[n, xx, 2:2 + len(k)]) == k
            assert not tab[n, xx, 2 + len(k):].any() and xmin + len(k) <= n


def test_global_coefficient_table_keeps_its_layout():
    tab = aug.coeff_table()
    assert tab.shape == (113, 112, 8) and tab[1:, :, 1].max() == 4
    assert np.array_equal(tab, aug.coeff_table(112, 112))


# ------------------------------------------------------------------------------------------------ sampler
def _check_boxes(i, j, h, w, scale):
    """Inside the image; the area within `scale`, widened by the rounding of h and w to integers: target = area * U(scale) and
    w, h = round(sqrt(target * aspect)), round(sqrt(target / aspect)), so (w - .5)(h - .5) <= target <= (w + .5)(h + .5)."""
    assert (h > 0).all() and (w > 0).all() and (i >= 0).all() and (j >= 0).all() and (i + h <= 112).all() and (j + w <= 112).all()
    area = 112.0 * 112.0
    assert ((w - 0.5) * (h - 0.5) <= scale[1] * area + 1e-9).all()
    assert ((w + 0.5) * (h + 0.5) >= scale[0] * area - 1e-9).all()
    ratio = (w + 0.5) / (h - 0.5)
    assert (ratio >= 3.0 / 4.0).all() and ((w - 0.5) / (h + 0.5) <= 4.0 / 3.0).all()


@pytest.mark.parametrize("gs,ls", [((0.4, 1.0), (0.05, 0.4)), ((0.25, 0.9), (0.1, 0.3))])
def test_dino_sampler_distributions(gs, ls):
    rng = np.random.RandomState(0)
    ps = [aug.sample_dino_params(rng, 8, global_scale=gs, local_scale=ls) for _ in range(400)]          # 4000 crops
    g1, g2, loc = [c[0] for c in ps], [c[1] for c in ps], [p for c in ps for p in c[2:]]
    for sel, scale in ((g1 + g2, gs), (loc, ls)):
        _check_boxes(*(np.array([p[k] for p in sel]) for k in "ijhw"), scale)
    larea = np.array([p["h"] * p["w"] for p in loc]) / 112.0 ** 2
    garea = np.array([p["h"] * p["w"] for p in g1 + g2]) / 112.0 ** 2
    # (get_params rejects boxes wider or taller than the image: that only removes large global boxes)
    assert abs(larea.mean() - (ls[0] + ls[1]) / 2) < 0.03 and -0.1 < garea.mean() - (gs[0] + gs[1]) / 2 < 0.04
    flat = g1 + g2 + loc
    frac = lambda key, sel: np.mean([bool(p[key]) for p in sel])
    for sel in (g1 + g2, loc):
        assert abs(frac("flip", sel) - 0.5) < 0.05 and abs(frac("jitter", sel) - 0.8) < 0.04 and abs(frac("gray", sel) - 0.2) < 0.04
    assert all(p["blur_radius"] > 0 for p in g1) and abs(np.mean([p["blur_radius"] > 0 for p in g2]) - 0.1) < 0.05
    assert abs(np.mean([p["blur_radius"] > 0 for p in loc]) - 0.5) < 0.05
    assert abs(np.mean([p["solarize"] for p in g2]) - 0.2) < 0.06 and not any(p["solarize"] for p in g1 + loc)
    radii = np.array([p["blur_radius"] for p in flat if p["blur_radius"] > 0])
    assert 0.1 <= radii.min() and radii.max() <= 2.0 and abs(radii.mean() - 1.05) < 0.05
    f = np.array([p["factors"] for p in flat])
    assert (f.min(0) >= [0.6, 0.6, 0.8, -0.1]).all() and (f.max(0) <= [1.4, 1.4, 1.2, 0.1]).all()
    assert all(sorted(p["order"]) == [0, 1, 2, 3] for p in flat)


def test_dino_packed_sampler_distributions_and_records():
    rng = np.random.RandomState(1)
    B, nl = 40, 8
    gs, ls = (0.4, 1.0), (0.05, 0.4)
    recs, dicts = [], []
    for _ in range(10):                                                  # 4000 crops
        r, d = aug.sample_dino_packed(rng, B, nl, return_dicts=True)
        assert r.shape == (B, 2 + nl, aug.P_WORDS) and r.dtype == np.int32
        recs.append(r), dicts.extend(d)
    # the records decode to the dicts returned with them: pack_params of the dicts is the record array
    assert np.array_equal(aug.pack_params(dicts), np.concatenate(recs))
    r = np.concatenate(recs)
    k = np.broadcast_to(np.arange(2 + nl), r.shape[:2])
    for sel, scale in ((k < 2, gs), (k >= 2, ls)):
        q = r[sel]
        _check_boxes(q[:, 0], q[:, 1], q[:, 2], q[:, 3], scale)
        assert abs((q[:, 4] & 1).mean() - 0.5) < 0.03 and abs(((q[:, 4] >> 1) & 1).mean() - 0.8) < 0.03
        assert abs(((q[:, 4] >> 2) & 1).mean() - 0.2) < 0.03
    larea = (r[k >= 2][:, 2] * r[k >= 2][:, 3]) / 112.0 ** 2
    garea = (r[k < 2][:, 2] * r[k < 2][:, 3]) / 112.0 ** 2
    assert abs(larea.mean() - 0.225) < 0.03 and 0.6 < garea.mean() < 0.74
    assert r[k == 0][:, 13].mean() > 0.99 and abs(r[k == 1][:, 13].mean() - 0.1) < 0.05 and abs(r[k >= 2][:, 13].mean() - 0.5) < 0.03
    assert abs(((r[k == 1][:, 4] >> 3) & 1).mean() - 0.2) < 0.06 and ((r[k != 1][:, 4] >> 3) & 1).sum() == 0
    # honoured scales: a narrow local range moves the local areas and leaves the globals alone
    r2 = aug.sample_dino_packed(np.random.RandomState(2), 64, 8, local_scale=(0.3, 0.35))
    a2 = r2[:, 2:, 2] * r2[:, 2:, 3] / 112.0 ** 2
    assert 0.28 < a2.min() and a2.max() < 0.37


# ------------------------------------------------------------------------------------------------ argument checks (no device)
def test_lafs_dino_views_rejects_bad_arguments_before_any_launch():
    import __graft_entry__ as g
    g.build()
    from lafs_cvpr2024_amd import _lib
    h = _lib.lib()
    ms = (C.c_float * 6)(*D.IMAGENET[0], *D.IMAGENET[1])
    buf = (C.c_int32 * 64)()                                             # a non-null operand; never dereferenced: the checks come first
    p = C.cast(buf, C.c_void_p)
    cases = {
        "null images": (None, p, p, p, 12, 2, 2, ms, p, p),
        "null params": (p, None, p, p, 12, 2, 2, ms, p, p),
        "null global table": (p, p, None, p, 12, 2, 2, ms, p, p),
        "null mean/std": (p, p, p, p, 12, 2, 2, None, p, p),
        "null globals": (p, p, p, p, 12, 2, 2, ms, None, p),
        "null locals with local crops": (p, p, p, p, 12, 2, 2, ms, p, None),
        "null local table with local crops": (p, p, p, None, 12, 2, 2, ms, p, p),
        "B = 0": (p, p, p, p, 12, 0, 2, ms, p, p),
        "B < 0": (p, p, p, p, 12, -3, 2, ms, p, p),
        "n_local < 0": (p, p, p, p, 12, 2, -1, ms, p, p),
    }
    for name, args in cases.items():
        rc = h.lafs_dino_views(*args, None)
        assert rc < 0 and h.lafs_last_error(), name


def test_views_dino_needs_uint8_images(monkeypatch):
    from lafs_cvpr2024_amd import lafs_train as L
    from lafs_cvpr2024_amd import utils
    monkeypatch.setattr(utils, "init_distributed_mode", lambda args: pytest.fail("the run was started"))
    a = L.get_args_parser().parse_args([])
    assert (a.views, a.views_norm) == ("lafs", "imagenet")
    for data in ("synthetic", "synthetic_views"):
        a = L.get_args_parser().parse_args(f"--arch fvit --views dino --data {data}".split())
        with pytest.raises(SystemExit, match="uint8"):
            L.train_lafs(a)
    a = L.get_args_parser().parse_args("--views dino --data synthetic_u8 --local_crops_scale 0.4 0.05".split())
    with pytest.raises(SystemExit, match="local_crops_scale"):
        L.train_lafs(a)
    with pytest.raises(SystemExit):
        L.get_args_parser().parse_args("--views simclr".split())
    L.check_views(L.get_args_parser().parse_args("--views dino --data recordio --views_norm half".split()))
