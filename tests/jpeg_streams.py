"""JPEG streams for tests/test_jpeg_host.py and tests/test_gpu_jpeg.py: written with Pillow from a seed at test time, together
with Pillow's own decode of each (the reference the device decoder must equal byte for byte)."""
import io
import zlib

import numpy as np
from PIL import Image

SAMPLINGS = ("444", "422", "420", "gray")
_SUBSAMPLING = {"444": 0, "422": 1, "420": 2}
CONTENTS = ("noise", "ramps", "binary")


def picture(content, w, h, seed):
    """uint8 [h, w, 3]: uniform noise, ramps + noise, or binary noise."""
    rng = np.random.RandomState(seed)
    if content == "noise":
        return rng.randint(0, 256, (h, w, 3)).astype(np.uint8)
    if content == "binary":
        return (rng.randint(0, 2, (h, w, 3)) * 255).astype(np.uint8)
    yy, xx = np.mgrid[0:h, 0:w]
    base = np.stack([xx * 255.0 / max(w - 1, 1), yy * 255.0 / max(h - 1, 1), (xx + yy) * 255.0 / max(w + h - 2, 1)], axis=-1)
    return np.clip(base + rng.normal(0, 6, (h, w, 3)), 0, 255).astype(np.uint8)


def encode(w, h, sampling, quality, content="ramps", optimize=False, seed=None, **save_args):
    """One stream; the seed defaults to a hash of the parameters, so every stream of a grid differs."""
    if seed is None:
        seed = zlib.crc32(repr((w, h, sampling, quality, content, optimize, sorted(save_args.items()))).encode()) & 0x7FFFFFFF
    img = Image.fromarray(picture(content, w, h, seed))
    f = io.BytesIO()
    if sampling == "gray":
        img.convert("L").save(f, "JPEG", quality=quality, optimize=optimize, **save_args)
    else:
        img.save(f, "JPEG", quality=quality, subsampling=_SUBSAMPLING[sampling], optimize=optimize, **save_args)
    return f.getvalue()


def pillow_rgb(buf):
    """uint8 [3, H, W] as the CPU loader decodes it."""
    return np.ascontiguousarray(np.asarray(Image.open(io.BytesIO(buf)).convert("RGB")).transpose(2, 0, 1))


def restart_streams(sizes=((112, 112), (40, 24), (17, 23))):
    """(w, h, stream) with restart intervals: restart_marker_blocks 1 and 3 and restart_marker_rows 1, three colour samplings."""
    out = []
    for (w, h) in sizes:
        for sampling in ("444", "422", "420"):
            for args in ({"restart_marker_blocks": 1}, {"restart_marker_blocks": 3}, {"restart_marker_rows": 1}):
                out.append((w, h, encode(w, h, sampling, 90, "ramps", **args)))
    return out


def splice_after_soi(buf, segment):
    return buf[:2] + segment + buf[2:]


def segment(marker, payload):
    return bytes([0xFF, marker]) + (len(payload) + 2).to_bytes(2, "big") + payload
