"""Test-side oracle of the DINO-face views (DataAugmentationDINO, reference lafs_train.py:743-788): one view per crop, composed from
the Pillow-pinned pieces of oracle/augment.py -- resized_crop to 112 (globals) or 48 (locals), hflip, the colour chain -- and
ToTensor + Normalize(mean, std) in numpy float32, each operation rounded on its own.  tests/test_dino_views_host.py pins every
piece and the composition against the Pillow calls themselves, at both output sizes."""
import numpy as np

from oracle import augment as A

IMAGENET = ((0.485, 0.456, 0.406), (0.229, 0.224, 0.225))
HALF = ((0.5, 0.5, 0.5), (0.5, 0.5, 0.5))
GLOBAL, LOCAL = 112, 48


def normalize(img, mean, std):
    """ToTensor + Normalize(mean, std): uint8 HWC -> float32 CHW, (v / 255.f - mean) / std."""
    x = img.astype(np.float32) / np.float32(255.0)
    m, s = np.asarray(mean, np.float32), np.asarray(std, np.float32)
    return ((x - m) / s).astype(np.float32).transpose(2, 0, 1).copy()


def view_u8(img, p, size):
    """The uint8 HWC view of one crop record before ToTensor."""
    base = A.resized_crop(img, p["i"], p["j"], p["h"], p["w"], size)
    if p["flip"]:
        base = A.hflip(base)
    return A.color_pipeline(base, p)


def make_views(img, crops, mean, std):
    """One source image [112,112,3] uint8 and its 2 + n_local records -> (2 global views [3,112,112], n_local local views
    [3,48,48]), float32."""
    views = [normalize(view_u8(img, p, GLOBAL if k < 2 else LOCAL), mean, std) for k, p in enumerate(crops)]
    return views[:2], views[2:]


def images(B, seed):
    """Smooth photograph-like test images (the construction of tests/test_gpu_augment.py)."""
    rng = np.random.RandomState(seed)
    yy, xx = np.mgrid[0:112, 0:112]
    out = []
    for b in range(B):
        base = np.stack([127 + 90 * np.sin(xx / (6.0 + b) + c) * np.cos(yy / (5.0 + c) - b) for c in range(3)], -1)
        out.append(np.clip(base + rng.randn(112, 112, 3) * 20, 0, 255).astype(np.uint8))
    return out


def count_differing(globals_, locals_, imgs, params, mean, std):
    """Differing elements between the device result (crop-major numpy arrays [2B,3,112,112], [n_local*B,3,48,48]) and the oracle,
    and the list of (image, crop) that differ."""
    B = len(imgs)
    bad, where = 0, []
    for b in range(B):
        g, l = make_views(imgs[b], params[b], mean, std)
        for k, r in enumerate(g + l):
            got = globals_[k * B + b] if k < 2 else locals_[(k - 2) * B + b]
            n = int((got != r).sum())
            if n:
                bad += n
                where.append((b, k, n))
    return bad, where
