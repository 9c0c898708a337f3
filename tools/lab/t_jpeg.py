"""GPU box: time of the device JPEG decode on a fine-tune batch (128 x 112 x 112, q95) against Pillow on one host core, and the
images/s of the fine-tune RecordIO loader (6 workers) with --decode pillow and --decode device."""
import io
import tempfile
import time

import numpy as np
import torch
from PIL import Image

import os, sys
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__)))))
from lafs_cvpr2024_amd import jpeg as J, ops, recordio as R
from lafs_cvpr2024_amd.train_largescale import RecordIOFaces

B, N_LOADER, WORKERS = 128, 4096, 6
dev = torch.device("cuda", 0)
rng = np.random.RandomState(0)
yy, xx = np.mgrid[0:112, 0:112]


def face_like(k):
    """Smooth structure + mild noise: about the byte count of an aligned face crop at q95 (8 KB in 4:2:0)."""
    base = np.stack([127 + 90 * np.sin(xx / (9.0 + k % 7) + c) * np.cos(yy / (11.0 + k % 5) - c) for c in range(3)], -1)
    return np.clip(base + rng.randn(112, 112, 3) * 12, 0, 255).astype(np.uint8)


def jpeg_bytes(arr, subsampling):
    f = io.BytesIO()
    Image.fromarray(arr).save(f, "JPEG", quality=95, subsampling=subsampling)
    return f.getvalue()


pics = [face_like(k) for k in range(B)]
for name, sub in (("4:2:0", 2), ("4:4:4", 0)):
    bufs = [jpeg_bytes(a, sub) for a in pics]
    J.pack([J.parse(b) for b in bufs])                                  # warm-up: the first pinned allocation
    t0 = time.perf_counter()
    for _ in range(5):
        plans = [J.parse(b) for b in bufs]
        packed = J.pack(plans)
    t_host = (time.perf_counter() - t0) / 5
    stream, images, tables = (t.to(dev) for t in packed)
    out = torch.empty(B, 3, 112, 112, dtype=torch.uint8, device=dev)
    ws = torch.empty(ops._lib.lib().lafs_jpeg_workspace_bytes(B, 112, 112), dtype=torch.uint8, device=dev)
    st = torch.empty(B, dtype=torch.int32, device=dev)
    for _ in range(3):
        ops.jpeg_decode(stream, images, tables, B, 112, 112, out=out, status=st, workspace=ws)
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda.synchronize(); e0.record()
    for _ in range(20):
        ops.jpeg_decode(stream, images, tables, B, 112, 112, out=out, status=st, workspace=ws)
    e1.record(); torch.cuda.synchronize()
    assert not st.cpu().any()
    t0 = time.perf_counter()
    for _ in range(3):
        ref = [J.pillow_decode(b) for b in bufs]
    t_pil = (time.perf_counter() - t0) / 3
    assert torch.equal(out.cpu(), torch.from_numpy(np.stack(ref)).permute(0, 3, 1, 2))
    t_dev = e0.elapsed_time(e1) / 20
    print(f"{name} q95, batch of {B} x 112 x 112, mean stream {np.mean([len(b) for b in bufs]):.0f} bytes: device decode {t_dev:.3f} ms per batch "
          f"({t_dev / B * 1e3:.1f} us per image, device events), parse + pack on one host core {t_host * 1e3:.2f} ms per batch "
          f"({t_host / B * 1e6:.1f} us per image), Pillow on one host core {t_pil * 1e3:.1f} ms per batch ({t_pil / B * 1e6:.1f} us per image)")

with tempfile.TemporaryDirectory() as d:
    wr = R.IndexedRecordWriter(os.path.join(d, "train.idx"), os.path.join(d, "train.rec"))
    for k in range(N_LOADER):
        wr.write_idx(k, R.pack(R.IRHeader(0, float(k % 100), k, 0), jpeg_bytes(pics[k % B], 2)))
    wr.close()
    for mode in ("pillow", "device"):
        data = RecordIOFaces(d, B, dev, 0, WORKERS, 0, 1, 100, tensor_records=True, decode=mode)
        best = 0.0
        for epoch in range(2):                                          # the first pass also pays for the page cache
            data.set_epoch(epoch)
            n, t0 = 0, None
            for x, y, recs in data:
                if t0 is None:                                          # the clock starts once the workers are up
                    torch.cuda.synchronize(); t0 = time.perf_counter(); continue
                n += x.shape[0]
            torch.cuda.synchronize()
            best = max(best, n / (time.perf_counter() - t0))
        print(f"fine-tune loader (RecordIOFaces, tensor records, {WORKERS} workers, batch {B}, loader alone): --decode {mode} {best:.0f} images/s")
