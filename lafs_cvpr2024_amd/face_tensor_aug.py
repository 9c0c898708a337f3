"""FaceDataset's torchvision tensor chain on the device (reference image_iter.py:214-219, applied per sample at :349-351 after
mirror, channel reversal and RandAugment):

    Compose([RandomResizedCrop(112, scale=(0.9, 1.0)), ColorJitter(0.1, 0.1, 0.1, 0.1), RandomErasing(scale=(0.02, 0.1))])

PARITY UNPINNED (restated from torchvision 0.9.1; torchvision is not installed).  The reference pins torchvision==0.9.1
(README.md:43).  Every random decision of the chain is a plain torch call, so `sample_one` makes exactly the calls 0.9.1 makes,
in its order, from a `torch.Generator`:

    RandomResizedCrop.get_params  up to 10 x (uniform_ area, exp(uniform_ log ratio)), w = round(sqrt(area * ratio)),
                                  h = round(sqrt(area / ratio)); accepted -> randint i, randint j; else the central-crop fallback
    ColorJitter.get_params        randperm(4), then brightness, contrast, saturation in [0.9, 1.1] and hue in [-0.1, 0.1]
    RandomErasing.forward         rand(1) < 0.5, then up to 10 x (uniform_ area, exp(uniform_ log ratio in (0.3, 3.3))),
                                  h = round(sqrt(area * ratio)), w = round(sqrt(area / ratio)), strict h < S and w < S; accepted ->
                                  randint i, randint j; else nothing is erased (value 0)

and packs them into one 80-byte record per image (include/lafs_hip.h `lafs_face_tensor_aug_rec`); lafs_face_tensor_aug
(csrc/face_tensor_aug.hip) applies a batch of them in one launch.  The pixel arithmetic is 0.9.1's functional_tensor as the
installed torch evaluates it on the CPU, bit-identical to tests/facedataset_tv_oracle.py.  Where later torchvision releases
differ, 0.9.1 is followed: `resize` has no antialias and no uint8 fast path (float32 bilinear interpolate with
align_corners=False, torch.round, uint8 cast), and adjust_hue ends with `(x * 255).to(uint8)`, a truncation (later releases
multiply by 255 + 1 - eps).  torch's CPU bilinear kernel evaluates the source coordinate and both interpolation steps as fused
multiply-adds; the kernel does the same.
"""
import math

import numpy as np
import torch

from .ops import _p, call

SIZE = 112
RECORD = np.dtype([("crop", "<i4", (4,)), ("order", "<i4", (4,)), ("blend", "<f4", (6,)), ("hue", "<f4"), ("erase", "<i4"),
                   ("erase_box", "<i4", (4,))])
assert RECORD.itemsize == 80

_RRC_SCALE, _RRC_RATIO = (0.9, 1.0), (3.0 / 4.0, 4.0 / 3.0)       # RandomResizedCrop(112, scale=(0.9, 1.0)), default ratio
_JITTER = 0.1                                                     # ColorJitter(0.1, 0.1, 0.1, 0.1)
_RE_P, _RE_SCALE, _RE_RATIO = 0.5, (0.02, 0.1), (0.3, 3.3)       # RandomErasing(scale=(0.02, 0.1)), default p and ratio
# torch.log(torch.tensor(ratio)) as get_params computes it, as the doubles uniform_ receives (no draw involved)
_RRC_LOG = tuple(float(v) for v in torch.log(torch.tensor(_RRC_RATIO)))
_RE_LOG = tuple(float(v) for v in torch.log(torch.tensor(_RE_RATIO)))


def _uniform(g, lo, hi):
    return torch.empty(1).uniform_(lo, hi, generator=g).item()


def _exp_uniform(g, lo, hi):
    return torch.exp(torch.empty(1).uniform_(lo, hi, generator=g)).item()


def _randint(g, n):
    return torch.randint(0, n, size=(1,), generator=g).item()


def sample_one(g, H=SIZE, W=SIZE, S=SIZE, rec=None):
    """The decisions of one call of the chain on a [3,H,W] image, drawn from generator `g` -> one RECORD."""
    if rec is None:
        rec = np.zeros((), RECORD)
    # RandomResizedCrop.get_params
    area = H * W
    box = None
    for _ in range(10):
        target_area = area * _uniform(g, *_RRC_SCALE)
        aspect_ratio = _exp_uniform(g, *_RRC_LOG)
        w = int(round(math.sqrt(target_area * aspect_ratio)))
        h = int(round(math.sqrt(target_area / aspect_ratio)))
        if 0 < w <= W and 0 < h <= H:
            i = _randint(g, H - h + 1)
            j = _randint(g, W - w + 1)
            box = (i, j, h, w)
            break
    if box is None:
        in_ratio = float(W) / float(H)
        if in_ratio < min(_RRC_RATIO):
            w, h = W, int(round(W / min(_RRC_RATIO)))
        elif in_ratio > max(_RRC_RATIO):
            h, w = H, int(round(H * max(_RRC_RATIO)))
        else:
            h, w = H, W
        box = ((H - h) // 2, (W - w) // 2, h, w)
    rec["crop"] = box
    # ColorJitter.get_params
    rec["order"] = torch.randperm(4, generator=g).numpy()
    factors = [float(torch.empty(1).uniform_(1 - _JITTER, 1 + _JITTER, generator=g)) for _ in range(3)]
    hue = float(torch.empty(1).uniform_(-_JITTER, _JITTER, generator=g))
    rec["blend"] = [v for f in factors for v in (f, 1.0 - f)]        # _blend: float32(r), float32(1.0 - r)
    rec["hue"] = hue
    # RandomErasing.forward / get_params
    rec["erase"] = 0
    rec["erase_box"] = 0
    if torch.rand(1, generator=g) < _RE_P:
        area = S * S
        for _ in range(10):
            erase_area = area * _uniform(g, *_RE_SCALE)
            aspect_ratio = _exp_uniform(g, *_RE_LOG)
            h = int(round(math.sqrt(erase_area * aspect_ratio)))
            w = int(round(math.sqrt(erase_area / aspect_ratio)))
            if not (h < S and w < S):
                continue
            i = _randint(g, S - h + 1)
            j = _randint(g, S - w + 1)
            rec["erase"] = 1
            rec["erase_box"] = (i, j, h, w)
            break
    return rec


def check_records(records, B, H, W, S=SIZE):
    """Host-side validation of records before they reach the device (the kernel clamps, but a bad record is an error)."""
    if records.dtype != RECORD or records.shape != (B,):
        raise ValueError(f"records must be a RECORD array of shape ({B},)")
    c, e = records["crop"], records["erase_box"]
    ok = (c[:, 0] >= 0) & (c[:, 1] >= 0) & (c[:, 2] >= 1) & (c[:, 3] >= 1) & (c[:, 0] + c[:, 2] <= H) & (c[:, 1] + c[:, 3] <= W)
    ok &= (np.sort(records["order"], axis=1) == np.arange(4)).all(axis=1)
    on = records["erase"] != 0
    ok &= ~on | ((e[:, 0] >= 0) & (e[:, 1] >= 0) & (e[:, 2] >= 0) & (e[:, 3] >= 0) & (e[:, 0] + e[:, 2] <= S) & (e[:, 1] + e[:, 3] <= S))
    if not ok.all():
        raise ValueError(f"invalid records at {np.nonzero(~ok)[0][:8].tolist()}")


class FaceTensorAug:
    """aug = FaceTensorAug(seed); out = aug(images_u8)   ([B,3,H,W] uint8 CUDA -> [B,3,112,112] uint8)"""

    def __init__(self, seed=None, size=SIZE):
        self.size = size
        self.gen = torch.Generator()
        if seed is not None:
            self.gen.manual_seed(int(seed))

    def sample(self, B, H=SIZE, W=SIZE):
        """Records [B], drawn image after image like B consecutive calls of the chain."""
        recs = np.zeros(B, RECORD)
        for b in range(B):
            sample_one(self.gen, H, W, self.size, recs[b])
        return recs

    def __call__(self, images, records=None, out=None):
        if images.dtype != torch.uint8 or not images.is_cuda or images.dim() != 4 or images.shape[1] != 3:
            raise ValueError("expected a uint8 CUDA tensor [B,3,H,W]")
        B, _, H, W = images.shape
        S = self.size
        if records is None:
            records = self.sample(B, H, W)
        check_records(records, B, H, W, S)
        images = images.contiguous()
        if out is None:
            out = torch.empty((B, 3, S, S), dtype=torch.uint8, device=images.device)
        elif out.dtype != torch.uint8 or tuple(out.shape) != (B, 3, S, S) or not out.is_contiguous() or out.device != images.device:
            raise ValueError(f"out must be a contiguous uint8 tensor [{B},3,{S},{S}] on {images.device}")
        rec = torch.from_numpy(np.ascontiguousarray(records).view(np.uint8).reshape(B, RECORD.itemsize)).to(images.device)
        call("lafs_face_tensor_aug", _p(images), _p(out), _p(rec), B, H, W, S)
        return out
