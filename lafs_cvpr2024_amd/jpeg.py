"""JPEG decode of the RecordIO loaders on the device (csrc/jpeg.hip, csrc/jpeg_core.hpp), bit-identical to Pillow.

The host does the cheap, branchy part -- the marker walk (`parse`, no GPU needed, fit for a DataLoader worker) and the packing of
a batch into three flat buffers (`pack`) -- and lafs_jpeg_decode does the rest in one launch per batch: Huffman decoding,
dequantisation, libjpeg's "islow" IDCT, its "fancy" chroma upsampling and its YCbCr -> RGB conversion.

`parse` accepts baseline / extended-sequential Huffman streams with 8-bit samples, a single scan, one component or three read as
YCbCr in 4:4:4 / 4:2:2 / 4:2:0, with or without restart intervals, and raises `UnsupportedJpeg` for everything else (progressive,
arithmetic, lossless, 12-bit, CMYK, RGB-tagged, other samplings, several scans, non-JPEG bytes, sizes over MAX_DIM).
`DeviceJpegDecoder` decodes those samples -- and any sample the kernel flags -- with Pillow into their slots, so its batches
always equal `Image.open(...).convert("RGB")` byte for byte; a truly corrupt record raises Pillow's own error.

Only streams written by Pillow (libjpeg-turbo) have been tested; see DESIGN.md section 7."""
import io

import numpy as np

MAX_DIM = 1024                      # LAFS_JPEG_MAX_DIM
TABLE_BYTES = 1600                  # LAFS_JPEG_TABLE_BYTES: 4 x 64 uint16 quantisers + (DC0, DC1, AC0, AC1) x (16 BITS + 256 HUFFVAL)
_QUANT_BYTES, _HUFF_BYTES = 512, 272
IMAGE = np.dtype([("data_off", "<i8"), ("data_len", "<i4"), ("table_off", "<i4"), ("width", "<i4"), ("height", "<i4"),
                  ("ncomp", "<i4"), ("restart_interval", "<i4"), ("hs", "u1", (3,)), ("vs", "u1", (3,)), ("tq", "u1", (3,)),
                  ("td", "u1", (3,)), ("ta", "u1", (3,)), ("pad", "u1", (17,))])
assert IMAGE.itemsize == 64
ST_RECORD, ST_OVERRUN, ST_CODE, ST_COEF, ST_RESTART = 1, 2, 4, 8, 16

_SOF_REFUSED = {0xC2: "progressive", 0xC3: "lossless", 0xC5: "differential sequential", 0xC6: "differential progressive",
                0xC7: "differential lossless", 0xC9: "arithmetic sequential", 0xCA: "arithmetic progressive", 0xCB: "arithmetic lossless",
                0xCD: "arithmetic differential sequential", 0xCE: "arithmetic differential progressive",
                0xCF: "arithmetic differential lossless"}


class UnsupportedJpeg(ValueError):
    """The stream is not one the device decoder accepts (it may still be a valid image: Pillow decodes it)."""


class Plan:
    """What `parse` found: geometry, table selectors, the 1600-byte table block and where the scan's bytes lie in `buf`."""
    __slots__ = ("buf", "data_off", "data_len", "width", "height", "ncomp", "hs", "vs", "tq", "td", "ta", "restart_interval", "tables")

    def detach(self):
        """Drop the reference to the stream (the loaders ship the bytes next to the plan, not twice)."""
        self.buf = None
        return self


def _check_huffman(bits, what):
    if sum(bits) > 256:
        raise UnsupportedJpeg(f"{what}: more than 256 codes")
    space = 0
    for l, n in enumerate(bits, 1):
        space += n << (16 - l)
    if space > 1 << 16:
        raise UnsupportedJpeg(f"{what}: over-subscribed code lengths")


def parse(buf):
    """Marker walk of one JPEG stream -> Plan; raises UnsupportedJpeg for anything the device decoder does not take."""
    buf = bytes(buf) if not isinstance(buf, bytes) else buf
    n = len(buf)
    if n < 4 or buf[0] != 0xFF or buf[1] != 0xD8:
        raise UnsupportedJpeg("not a JPEG stream (no SOI)")
    quant, huff = {}, {}
    frame, ri, jfif, adobe_transform = None, 0, False, None
    pos = 2
    while True:
        if pos + 1 >= n:
            raise UnsupportedJpeg("no scan found")
        if buf[pos] != 0xFF:
            raise UnsupportedJpeg(f"expected a marker at byte {pos}")
        while pos + 1 < n and buf[pos + 1] == 0xFF:                  # fill bytes
            pos += 1
        if pos + 1 >= n:
            raise UnsupportedJpeg("no scan found")
        m = buf[pos + 1]
        pos += 2
        if m == 0x01 or 0xD0 <= m <= 0xD7:                           # TEM / stray RSTn: no payload
            continue
        if m in (0xD8, 0xD9):
            raise UnsupportedJpeg("SOI / EOI before the scan")
        if pos + 2 > n:
            raise UnsupportedJpeg("truncated segment")
        seglen = (buf[pos] << 8) | buf[pos + 1]
        if seglen < 2 or pos + seglen > n:
            raise UnsupportedJpeg("truncated segment")
        seg = buf[pos + 2: pos + seglen]
        pos += seglen
        if m in _SOF_REFUSED:
            raise UnsupportedJpeg(_SOF_REFUSED[m] + " JPEG")
        if m in (0xC0, 0xC1):
            if frame is not None:
                raise UnsupportedJpeg("several frames")
            if len(seg) < 6:
                raise UnsupportedJpeg("short SOF")
            precision, height, width, ncomp = seg[0], (seg[1] << 8) | seg[2], (seg[3] << 8) | seg[4], seg[5]
            if precision != 8:
                raise UnsupportedJpeg(f"{precision}-bit samples")
            if ncomp not in (1, 3):
                raise UnsupportedJpeg(f"{ncomp} components")
            if not (1 <= width <= MAX_DIM and 1 <= height <= MAX_DIM):
                raise UnsupportedJpeg(f"size {width}x{height} outside 1..{MAX_DIM}")
            if len(seg) != 6 + 3 * ncomp:
                raise UnsupportedJpeg("bad SOF length")
            comps = [(seg[6 + 3 * i], seg[7 + 3 * i] >> 4, seg[7 + 3 * i] & 15, seg[8 + 3 * i]) for i in range(ncomp)]
            frame = (width, height, comps)
        elif m == 0xDB:                                              # DQT: one or more tables
            i = 0
            while i < len(seg):
                pq, tq = seg[i] >> 4, seg[i] & 15
                size = 128 if pq else 64
                if pq > 1 or tq > 3 or i + 1 + size > len(seg):
                    raise UnsupportedJpeg("bad DQT")
                raw = seg[i + 1: i + 1 + size]
                quant[tq] = np.frombuffer(raw, dtype=">u2" if pq else "u1").astype("<u2").tobytes()
                i += 1 + size
        elif m == 0xC4:                                              # DHT: one or more tables
            i = 0
            while i < len(seg):
                if i + 17 > len(seg):
                    raise UnsupportedJpeg("bad DHT")
                tc, th = seg[i] >> 4, seg[i] & 15
                bits = seg[i + 1: i + 17]
                total = sum(bits)
                if tc > 1 or th > 1:
                    raise UnsupportedJpeg(f"Huffman table class {tc} id {th} (two DC and two AC tables are held)")
                _check_huffman(bits, "DHT")
                if i + 17 + total > len(seg):
                    raise UnsupportedJpeg("bad DHT")
                huff[(tc, th)] = bytes(bits) + bytes(seg[i + 17: i + 17 + total]) + bytes(256 - total)
                i += 17 + total
        elif m == 0xDD:
            if len(seg) != 2:
                raise UnsupportedJpeg("bad DRI")
            ri = (seg[0] << 8) | seg[1]
        elif m == 0xE0 and seg[:5] == b"JFIF\0":
            jfif = True
        elif m == 0xEE and seg[:5] == b"Adobe" and len(seg) >= 12:
            adobe_transform = seg[11]
        elif m == 0xDA:
            break
        # every other APPn, COM, DNL ... segment is skipped
    if frame is None:
        raise UnsupportedJpeg("scan before the frame header")
    width, height, comps = frame
    ncomp = len(comps)
    if len(seg) != 4 + 2 * ncomp or seg[0] != ncomp:
        raise UnsupportedJpeg("several scans (the scan does not hold every component)")
    if seg[1 + 2 * ncomp] != 0 or seg[2 + 2 * ncomp] != 63 or seg[3 + 2 * ncomp] != 0:
        raise UnsupportedJpeg("not a sequential full-precision scan")
    if ncomp == 3:
        if adobe_transform == 0:
            raise UnsupportedJpeg("Adobe transform 0 (RGB)")
        if not jfif and adobe_transform is None and tuple(c[0] for c in comps) == (82, 71, 66):
            raise UnsupportedJpeg("components tagged R, G, B")
    p = Plan()
    p.width, p.height, p.ncomp, p.restart_interval = width, height, ncomp, ri
    p.hs, p.vs, p.tq, p.td, p.ta = [1, 1, 1], [1, 1, 1], [0, 0, 0], [0, 0, 0], [0, 0, 0]
    for i, (cid, h, v, tq) in enumerate(comps):
        if seg[1 + 2 * i] != cid:
            raise UnsupportedJpeg("scan components out of frame order")
        td, ta = seg[2 + 2 * i] >> 4, seg[2 + 2 * i] & 15
        if tq not in quant:
            raise UnsupportedJpeg(f"quantisation table {tq} is not defined")
        if (0, td) not in huff or (1, ta) not in huff:
            raise UnsupportedJpeg(f"Huffman table DC {td} / AC {ta} is not defined")
        p.hs[i], p.vs[i], p.tq[i], p.td[i], p.ta[i] = h, v, tq, td, ta
    if ncomp == 1:
        p.hs[0] = p.vs[0] = 1                                        # a one-component scan is not interleaved: the factors do not matter
    else:
        if (p.hs[0], p.vs[0]) not in ((1, 1), (2, 1), (2, 2)) or (p.hs[1], p.vs[1], p.hs[2], p.vs[2]) != (1, 1, 1, 1):
            raise UnsupportedJpeg(f"sampling {list(zip(p.hs, p.vs))}")
    # the scan's bytes: up to the first marker that is neither a stuffed FF 00 nor RSTn; it must be EOI
    start, i = pos, pos
    while True:
        i = buf.find(b"\xff", i)
        if i < 0 or i + 1 >= n:
            raise UnsupportedJpeg("no EOI after the scan")
        nxt = buf[i + 1]
        if nxt == 0x00 or 0xD0 <= nxt <= 0xD7:
            i += 2
        elif nxt == 0xFF:
            i += 1
        else:
            break
    end = i
    while end > start and buf[end - 1] == 0xFF:                      # fill bytes in front of the marker
        end -= 1
    if buf[i + 1] != 0xD9:
        raise UnsupportedJpeg("several scans, or tables after the scan")
    if end - start >= 1 << 31:
        raise UnsupportedJpeg("scan too long")
    p.buf, p.data_off, p.data_len = buf, start, end - start
    tables = bytearray(TABLE_BYTES)
    for tq, raw in quant.items():
        tables[tq * 128: tq * 128 + 128] = raw
    for (tc, th), raw in huff.items():
        o = _QUANT_BYTES + (2 * tc + th) * _HUFF_BYTES
        tables[o: o + _HUFF_BYTES] = raw
    p.tables = bytes(tables)
    return p


def pack(plans, bufs=None, pin=None):
    """Plans of one batch (None = a sample the device does not take: its record is refused by the kernel and gets status 1) ->
    (stream, images, tables): three uint8 host tensors, pinned when a GPU is there.  `bufs[i]` replaces a detached plan's stream;
    identical table blocks are stored once."""
    import torch
    if pin is None:
        pin = torch.cuda.is_available()
    live = [(i, p) for i, p in enumerate(plans) if p is not None]
    table_index = {}
    for _, p in live:
        table_index.setdefault(p.tables, len(table_index) * TABLE_BYTES)
    # the three buffers are allocated once (pinned) and filled in place: each scan is copied exactly once on the host
    stream = torch.empty(max(sum(p.data_len for _, p in live), 1), dtype=torch.uint8, pin_memory=pin)
    images = torch.zeros(len(plans) * IMAGE.itemsize, dtype=torch.uint8, pin_memory=pin)
    tables = torch.zeros(max(len(table_index), 1) * TABLE_BYTES, dtype=torch.uint8, pin_memory=pin)
    sv, recs, tv = stream.numpy(), images.numpy().view(IMAGE), tables.numpy()
    sv[:1] = 0
    for blk, t in table_index.items():
        tv[t: t + TABLE_BYTES] = np.frombuffer(blk, np.uint8)
    off = 0
    for i, p in live:
        buf = p.buf if p.buf is not None else bufs[i]
        sv[off: off + p.data_len] = np.frombuffer(buf, np.uint8, p.data_len, p.data_off)
        r = recs[i]
        r["data_off"], r["data_len"], r["table_off"] = off, p.data_len, table_index[p.tables]
        r["width"], r["height"], r["ncomp"], r["restart_interval"] = p.width, p.height, p.ncomp, p.restart_interval
        r["hs"], r["vs"], r["tq"], r["td"], r["ta"] = p.hs, p.vs, p.tq, p.td, p.ta
        off += p.data_len
    return stream, images, tables


def pillow_decode(buf):
    """The CPU path: uint8 [H, W, 3]."""
    from PIL import Image
    return np.asarray(Image.open(io.BytesIO(buf)).convert("RGB"))


def try_parse(buf):
    """parse(buf) detached from the stream, or None when the device does not take it (what a loader worker ships)."""
    try:
        return parse(buf).detach()
    except UnsupportedJpeg:
        return None


class DeviceJpegDecoder:
    """dec = DeviceJpegDecoder(device); u8 = dec(list_of_bytes)  ->  uint8 [B,3,H,W] on the device, equal to Pillow's decode."""

    def __init__(self, device):
        import torch
        self.device = torch.device(device)
        self.launched = 0               # samples decoded by the kernel / by Pillow so far
        self.fell_back = 0

    def __call__(self, bufs, plans=None):
        import torch
        from . import ops
        B = len(bufs)
        if B == 0:
            raise ValueError("empty batch")
        if plans is None:
            plans = [False] * B         # False = not parsed yet, None = parsed and refused
        plans = [try_parse(b) if p is False else p for b, p in zip(bufs, plans)]
        fallback = {i: pillow_decode(bufs[i]) for i, p in enumerate(plans) if p is None}
        sizes = {(p.height, p.width) for p in plans if p is not None} | {a.shape[:2] for a in fallback.values()}
        if len(sizes) != 1:
            raise ValueError(f"mixed image sizes in one batch: {sorted(sizes)}")
        H, W = sizes.pop()
        out = torch.empty(B, 3, H, W, dtype=torch.uint8, device=self.device)
        if len(fallback) < B:
            if H > MAX_DIM or W > MAX_DIM:
                raise ValueError(f"images of {W}x{H} are over the decoder's limit of {MAX_DIM}")
            stream, images, tables = pack(plans, bufs)
            dev = lambda t: t.to(self.device, non_blocking=True)
            status = ops.jpeg_decode(dev(stream), dev(images), dev(tables), B, H, W, out=out)
            bad = torch.nonzero(status.cpu()).flatten().tolist()          # waits for the decode only (same stream)
            for i in bad:
                if i not in fallback:
                    fallback[i] = pillow_decode(bufs[i])                   # raises Pillow's error for a corrupt record
        for i, arr in fallback.items():
            if arr.shape != (H, W, 3):
                raise ValueError(f"mixed image sizes in one batch: {arr.shape[:2]} and {(H, W)}")
            out[i].copy_(torch.from_numpy(np.ascontiguousarray(arr.transpose(2, 0, 1))))
        self.launched += B - len(fallback)
        self.fell_back += len(fallback)
        return out
