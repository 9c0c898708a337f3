#!/usr/bin/env python3
"""Write a small synthetic verification set in the pickled .bin layout of LFW / CFP-FP / AgeDB ((encoded images, issame_list), pair i =
images 2i, 2i+1) for end-to-end runs of `train_largescale.py --val_path` and of `python -m lafs_cvpr2024_amd.verification`.  Pairs
alternate same / different identity; the two images of a same-identity pair share a base pattern.
usage: tools/make_synthetic_bin.py OUT.bin [pairs] [png|jpeg]   (jpeg: quality 100)"""
import io
import os
import pickle
import sys

import numpy as np
from PIL import Image


def make(path, pairs=60, fmt="png", seed=0):
    rng = np.random.RandomState(seed)
    yy, xx = np.mgrid[0:112, 0:112]

    def base(ident):
        return np.stack([127 + 90 * np.sin(xx / (5.0 + ident % 7) + c) * np.cos(yy / (6.0 + c) - ident) for c in range(3)], -1)

    def encode(img):
        b = io.BytesIO()
        if fmt == "jpeg":
            Image.fromarray(img).save(b, format="JPEG", quality=100)
        else:
            Image.fromarray(img).save(b, format="PNG")
        return b.getvalue()

    bins, issame = [], []
    for i in range(pairs):
        same = i % 2 == 0
        a, b = 2 * i, (2 * i if same else 2 * i + 1)
        for ident in (a, b):
            img = np.clip(base(ident) + rng.randn(112, 112, 3) * 25, 0, 255).astype(np.uint8)
            bins.append(encode(img))
        issame.append(same)
    os.makedirs(os.path.dirname(os.path.abspath(path)), exist_ok=True)
    with open(path, "wb") as f:
        pickle.dump((bins, issame), f, protocol=4)
    return bins, issame


if __name__ == "__main__":
    out = sys.argv[1]
    n = int(sys.argv[2]) if len(sys.argv) > 2 else 60
    fmt = sys.argv[3] if len(sys.argv) > 3 else "png"
    make(out, n, fmt)
    print(f"wrote {2 * n} images ({n} pairs) to {out}")
