"""CPU-torch restatement of the torchvision 0.9.1 tensor transforms of the reference's FaceDataset (image_iter.py:214-219,
349-351):

    Compose([RandomResizedCrop(112, scale=(0.9, 1.0)), ColorJitter(0.1, 0.1, 0.1, 0.1), RandomErasing(scale=(0.02, 0.1))])

applied to a uint8 CHW tensor.  A helper of the tests (not collected), independent of the product code
(lafs_cvpr2024_amd/face_tensor_aug.py): `get_params` below are the three transforms' own get_params / forward draws, and `apply`
is built from the tensor expressions of torchvision.transforms.functional_tensor (resize through _cast_squeeze_in/out, _blend,
rgb_to_grayscale, _rgb2hsv / _hsv2rgb with the einsum select, erase).

PARITY UNPINNED: torchvision is not installed, so this is restated from the 0.9.1 sources (the version the reference pins,
README.md:43), not executed against them.  Where later releases differ, 0.9.1 is followed: resize has no antialias argument and
no uint8 fast path (the crop is cast to float32, interpolated with align_corners=False, rounded half to even and cast back), and
the hue adjustment ends with `(x * 255.0).to(uint8)` (truncation; later releases multiply by 255 + 1 - eps).
"""
import math

import torch
import torch.nn.functional as F

SIZE = 112
RRC_SCALE, RRC_RATIO = (0.9, 1.0), (3.0 / 4.0, 4.0 / 3.0)
JITTER = 0.1
RE_P, RE_SCALE, RE_RATIO = 0.5, (0.02, 0.1), (0.3, 3.3)


# ---------------------------------------------------------------------------------------------------------- random decisions
def rrc_get_params(height, width, g, scale=RRC_SCALE, ratio=RRC_RATIO):
    """transforms.RandomResizedCrop.get_params -> (i, j, h, w)."""
    area = height * width
    for _ in range(10):
        target_area = area * torch.empty(1).uniform_(scale[0], scale[1], generator=g).item()
        log_ratio = torch.log(torch.tensor(ratio))
        aspect_ratio = torch.exp(torch.empty(1).uniform_(log_ratio[0], log_ratio[1], generator=g)).item()
        w = int(round(math.sqrt(target_area * aspect_ratio)))
        h = int(round(math.sqrt(target_area / aspect_ratio)))
        if 0 < w <= width and 0 < h <= height:
            i = torch.randint(0, height - h + 1, size=(1,), generator=g).item()
            j = torch.randint(0, width - w + 1, size=(1,), generator=g).item()
            return i, j, h, w
    in_ratio = float(width) / float(height)                    # fallback to central crop
    if in_ratio < min(ratio):
        w = width
        h = int(round(w / min(ratio)))
    elif in_ratio > max(ratio):
        h = height
        w = int(round(h * max(ratio)))
    else:
        w = width
        h = height
    return (height - h) // 2, (width - w) // 2, h, w


def jitter_get_params(g):
    """transforms.ColorJitter(0.1, 0.1, 0.1, 0.1).get_params -> (fn_idx list, b, c, s, h)."""
    fn_idx = torch.randperm(4, generator=g)
    b = float(torch.empty(1).uniform_(1 - JITTER, 1 + JITTER, generator=g))
    c = float(torch.empty(1).uniform_(1 - JITTER, 1 + JITTER, generator=g))
    s = float(torch.empty(1).uniform_(1 - JITTER, 1 + JITTER, generator=g))
    h = float(torch.empty(1).uniform_(-JITTER, JITTER, generator=g))
    return [int(v) for v in fn_idx], b, c, s, h


def erase_get_params(img_h, img_w, g, p=RE_P, scale=RE_SCALE, ratio=RE_RATIO):
    """transforms.RandomErasing(scale=(0.02, 0.1)).forward's draws -> None (not applied, or no box found) or (i, j, h, w)."""
    if not torch.rand(1, generator=g) < p:
        return None
    area = img_h * img_w
    for _ in range(10):
        erase_area = area * torch.empty(1).uniform_(scale[0], scale[1], generator=g).item()
        log_ratio = torch.log(torch.tensor(ratio))
        aspect_ratio = torch.exp(torch.empty(1).uniform_(log_ratio[0], log_ratio[1], generator=g)).item()
        h = int(round(math.sqrt(erase_area * aspect_ratio)))
        w = int(round(math.sqrt(erase_area / aspect_ratio)))
        if not (h < img_h and w < img_w):
            continue
        i = torch.randint(0, img_h - h + 1, size=(1,), generator=g).item()
        j = torch.randint(0, img_w - w + 1, size=(1,), generator=g).item()
        return i, j, h, w
    return None                                                # get_params returns the image itself: nothing changes


def get_params(height, width, g, size=SIZE):
    """All decisions of one call of the Compose, in torchvision's order."""
    crop = rrc_get_params(height, width, g)
    order, b, c, s, h = jitter_get_params(g)
    erase = erase_get_params(size, size, g)
    return dict(crop=crop, order=order, brightness=b, contrast=c, saturation=s, hue=h, erase=erase)


# ---------------------------------------------------------------------------------------------------------- pixel arithmetic
def resize(img, size):
    """F_t.resize(img, [size, size], 'bilinear') on uint8 CHW (0.9.1: no antialias, float32 interpolate, round, cast)."""
    x = img.unsqueeze(0).to(torch.float32)
    x = F.interpolate(x, size=[size, size], mode="bilinear", align_corners=False)
    return torch.round(x).squeeze(0).to(torch.uint8)


def _blend(img1, img2, ratio):
    ratio = float(ratio)
    return (ratio * img1 + (1.0 - ratio) * img2).clamp(0, 255.0).to(img1.dtype)


def rgb_to_grayscale(img):
    r, g, b = img.unbind(dim=-3)
    return (0.2989 * r + 0.587 * g + 0.114 * b).to(img.dtype).unsqueeze(dim=-3)


def adjust_brightness(img, f):
    return _blend(img, torch.zeros_like(img), f)


def adjust_contrast(img, f):
    mean = torch.mean(rgb_to_grayscale(img).to(torch.float32), dim=(-3, -2, -1), keepdim=True)
    return _blend(img, mean, f)


def adjust_saturation(img, f):
    return _blend(img, rgb_to_grayscale(img), f)


def _rgb2hsv(img):
    r, g, b = img.unbind(dim=-3)
    maxc = torch.max(img, dim=-3).values
    minc = torch.min(img, dim=-3).values
    eqc = maxc == minc
    cr = maxc - minc
    ones = torch.ones_like(maxc)
    s = cr / torch.where(eqc, ones, maxc)
    cr_divisor = torch.where(eqc, ones, cr)
    rc = (maxc - r) / cr_divisor
    gc = (maxc - g) / cr_divisor
    bc = (maxc - b) / cr_divisor
    hr = (maxc == r) * (bc - gc)
    hg = ((maxc == g) & (maxc != r)) * (2.0 + rc - bc)
    hb = ((maxc != g) & (maxc != r)) * (4.0 + gc - rc)
    h = hr + hg + hb
    h = torch.fmod((h / 6.0 + 1.0), 1.0)
    return torch.stack((h, s, maxc), dim=-3)


def _hsv2rgb(img):
    h, s, v = img.unbind(dim=-3)
    i = torch.floor(h * 6.0)
    f = (h * 6.0) - i
    i = i.to(dtype=torch.int32)
    p = torch.clamp((v * (1.0 - s)), 0.0, 1.0)
    q = torch.clamp((v * (1.0 - s * f)), 0.0, 1.0)
    t = torch.clamp((v * (1.0 - s * (1.0 - f))), 0.0, 1.0)
    i = i % 6
    mask = i.unsqueeze(dim=-3) == torch.arange(6, device=i.device).view(-1, 1, 1)
    a1 = torch.stack((v, q, p, p, t, v), dim=-3)
    a2 = torch.stack((t, v, v, q, p, p), dim=-3)
    a3 = torch.stack((p, p, t, v, v, q), dim=-3)
    a4 = torch.stack((a1, a2, a3), dim=-4)
    return torch.einsum("...ijk, ...xijk -> ...xjk", mask.to(dtype=img.dtype), a4)


def adjust_hue(img, f):
    x = img.to(dtype=torch.float32) / 255.0
    x = _rgb2hsv(x)
    h, s, v = x.unbind(dim=-3)
    h = (h + f) % 1.0
    x = _hsv2rgb(torch.stack((h, s, v), dim=-3))
    return (x * 255.0).to(dtype=torch.uint8)


def apply(img, params, size=SIZE):
    """uint8 CHW [3,H,W] -> uint8 [3,size,size] under the decisions of get_params."""
    i, j, h, w = params["crop"]
    out = resize(img[..., i:i + h, j:j + w], size)
    for fn in params["order"]:
        if fn == 0:
            out = adjust_brightness(out, params["brightness"])
        elif fn == 1:
            out = adjust_contrast(out, params["contrast"])
        elif fn == 2:
            out = adjust_saturation(out, params["saturation"])
        else:
            out = adjust_hue(out, params["hue"])
    if params["erase"] is not None:
        i, j, h, w = params["erase"]
        out = out.clone()
        out[..., i:i + h, j:j + w] = 0
    return out
