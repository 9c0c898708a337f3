"""CPU: the JPEG decoder's arithmetic (csrc/jpeg_core.hpp, the text the gfx950 kernel is compiled from) as a stand-alone program
(tests/jpeg_host_main.cpp) built with -fsanitize=address,undefined and run as a child process, against Pillow byte for byte; the
marker walk of lafs_cvpr2024_amd.jpeg.parse; and the decoder's behaviour on truncated and corrupted scans (host only: no
malformed stream is ever sent to a GPU)."""
import copy
import io
import os
import shutil
import subprocess
import sys

import numpy as np
import pytest
from PIL import Image

sys.path.insert(0, os.path.dirname(__file__))
import jpeg_streams as S  # noqa: E402
from lafs_cvpr2024_amd import jpeg as J  # noqa: E402

HERE = os.path.dirname(os.path.abspath(__file__))
SIZES = ((1, 1), (3, 5), (8, 8), (16, 16), (17, 23), (23, 17), (32, 48), (40, 24), (9, 33))


@pytest.fixture(scope="module")
def program(tmp_path_factory):
    cxx = shutil.which("clang++") or shutil.which("g++") or shutil.which("clang++", path="/opt/rocm/lib/llvm/bin:/opt/rocm/llvm/bin")
    assert cxx, "no host C++ compiler (clang++ or g++)"
    exe = str(tmp_path_factory.mktemp("jpeg_host") / "jpeg_host_main")
    # the sanitizer runtimes are linked statically (clang++ does so by default), so the program runs in whatever environment
    # the suite runs in, untouched
    static = ["-static-libasan", "-static-libubsan"] if os.path.basename(cxx).startswith("g++") else []
    subprocess.run([cxx, "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all"] + static +
                   [os.path.join(HERE, "jpeg_host_main.cpp"), "-o", exe], check=True)
    return exe


def run_batches(program, tmp_path, batches):
    """batches: list of (plans, H, W) -> list of (status [B], pixels [B,3,H,W]); one run of the program for all of them."""
    src, dst = str(tmp_path / "in.bin"), str(tmp_path / "out.bin")
    with open(src, "wb") as f:
        for plans, H, W in batches:
            stream, images, tables = J.pack(plans, pin=False)
            f.write(np.array([len(plans), H, W, stream.numel(), tables.numel()], dtype="<i8").tobytes())
            for t in (images, stream, tables):
                f.write(t.numpy().tobytes())
    r = subprocess.run([program, src, dst], capture_output=True, text=True)
    assert r.returncode == 0, f"exit {r.returncode}\n{r.stderr[-4000:]}"
    raw = open(dst, "rb").read()
    out, o = [], 0
    for plans, H, W in batches:
        B = len(plans)
        st = np.frombuffer(raw, "<i4", B, o); o += 4 * B
        px = np.frombuffer(raw, "u1", B * 3 * H * W, o).reshape(B, 3, H, W); o += B * 3 * H * W
        out.append((st, px))
    assert o == len(raw), "every image has a status and a full set of pixels"
    return out


def exactness_grid():
    """(w, h, stream) of the issue's grid."""
    streams = []
    for (w, h) in SIZES:
        for sampling in S.SAMPLINGS:
            for quality in (50, 95, 100):
                for content in S.CONTENTS:
                    for optimize in (False, True):
                        streams.append((w, h, S.encode(w, h, sampling, quality, content, optimize)))
    for sampling in S.SAMPLINGS:
        streams.append((112, 112, S.encode(112, 112, sampling, 95, "ramps")))
    return streams + S.restart_streams()


def large_streams():
    """Sizes up to the decoder's limit: 256x256 in the four samplings, MAX_DIM x MAX_DIM and one odd size next to it."""
    streams = [(256, 256, S.encode(256, 256, sampling, 95, "noise" if sampling == "444" else "ramps")) for sampling in S.SAMPLINGS]
    m = J.MAX_DIM
    streams += [(m, m, S.encode(m, m, "420", 75, "ramps")), (m, m, S.encode(m, m, "444", 50, "ramps", optimize=True)),
                (m - 5, m - 11, S.encode(m - 5, m - 11, "422", 75, "ramps", restart_marker_rows=1)), (m, 3, S.encode(m, 3, "gray", 90, "noise"))]
    return streams


def test_every_stream_of_the_grid_equals_pillow_bit_for_bit(program, tmp_path):
    streams = exactness_grid()
    assert len(streams) == 9 * 4 * 3 * 3 * 2 + 4 + 27
    by_size = {}
    for w, h, buf in streams:
        by_size.setdefault((h, w), []).append(buf)
    batches, refs = [], []
    for (h, w), bufs in by_size.items():
        batches.append(([J.parse(b) for b in bufs], h, w))            # nothing in the grid may be refused: parse must not raise
        refs.append(np.stack([S.pillow_rgb(b) for b in bufs]))
    n_restart = sum(1 for plans, _, _ in batches for p in plans if p.restart_interval > 0)
    assert n_restart == 27
    for (plans, h, w), ref, (st, px) in zip(batches, refs, run_batches(program, tmp_path, batches)):
        assert not st.any(), f"{w}x{h}: status {st.tolist()}"
        bad = [i for i in range(len(plans)) if not np.array_equal(px[i], ref[i])]
        assert not bad, f"{w}x{h}: streams {bad} differ from Pillow (max |d| {np.abs(px.astype(int) - ref.astype(int)).max()})"


def test_sizes_up_to_the_limit_equal_pillow_bit_for_bit(program, tmp_path):
    streams = large_streams()
    batches = [([J.parse(buf)], h, w) for w, h, buf in streams]
    for (w, h, buf), (st, px) in zip(streams, run_batches(program, tmp_path, batches)):
        assert st[0] == 0 and np.array_equal(px[0], S.pillow_rgb(buf)), f"{w}x{h} differs from Pillow"


def test_sixteen_bit_quantiser_entries_and_merged_segments(program, tmp_path):
    """The same tables re-written as ONE DQT segment with 16-bit entries and ONE DHT segment holding all four tables decode to the
    same pixels."""
    buf = S.encode(17, 23, "420", 95, "noise")
    pos, dqt, dht, rest = 2, b"", b"", b""
    while buf[pos + 1] != 0xDA:
        m, n = buf[pos + 1], int.from_bytes(buf[pos + 2: pos + 4], "big")
        seg = buf[pos + 4: pos + 2 + n]
        if m == 0xDB:
            i = 0
            while i < len(seg):
                assert seg[i] >> 4 == 0
                dqt += bytes([0x10 | seg[i]]) + b"".join(bytes([0, v]) for v in seg[i + 1: i + 65])
                i += 65
        elif m == 0xC4:
            dht += seg
        else:
            rest += buf[pos: pos + 2 + n]
        pos += 2 + n
    merged = buf[:2] + rest + S.segment(0xDB, dqt) + S.segment(0xC4, dht) + buf[pos:]
    assert np.array_equal(S.pillow_rgb(merged), S.pillow_rgb(buf))
    (st, px), = run_batches(program, tmp_path, [([J.parse(merged)], 23, 17)])
    assert st[0] == 0 and np.array_equal(px[0], S.pillow_rgb(buf))


def test_parser_fields_and_skipped_segments(program, tmp_path):
    buf = S.encode(17, 23, "420", 95, "ramps", restart_marker_blocks=3)
    p = J.parse(buf)
    assert (p.width, p.height, p.ncomp, p.restart_interval) == (17, 23, 3, 3)
    assert (p.hs, p.vs) == ([2, 1, 1], [2, 1, 1]) and p.tq == [0, 1, 1] and p.td == [0, 1, 1] and p.ta == [0, 1, 1]
    assert len(p.tables) == J.TABLE_BYTES and buf[p.data_off - 14: p.data_off - 12] == b"\xff\xda"
    assert buf[p.data_off + p.data_len: p.data_off + p.data_len + 2] == b"\xff\xd9"
    g = J.parse(S.encode(9, 33, "gray", 50))
    assert (g.ncomp, g.hs[0], g.vs[0], g.restart_interval) == (1, 1, 1, 0)
    assert J.parse(S.encode(16, 16, "422", 50)).hs == [2, 1, 1] and J.parse(S.encode(16, 16, "444", 50)).vs == [1, 1, 1]

    variants = [S.splice_after_soi(buf, S.segment(0xFE, b"a comment \xff\xd9 with marker-like bytes")),
                S.splice_after_soi(buf, S.segment(0xE1, b"Exif\0\0" + bytes(range(256)))),
                S.splice_after_soi(buf, b"\xff\xff\xff"),
                buf[:-2] + b"\xff\xff" + buf[-2:]]
    plans = [J.parse(v) for v in variants]
    for q in plans:
        assert q.tables == p.tables and q.data_len == p.data_len
    (st, px), = run_batches(program, tmp_path, [(plans, 23, 17)])
    ref = S.pillow_rgb(buf)
    assert not st.any() and all(np.array_equal(px[i], ref) for i in range(len(variants)))


def test_parser_refuses_what_the_device_does_not_decode():
    img = Image.fromarray(S.picture("ramps", 16, 16, 5))

    def saved(im, fmt="JPEG", **kw):
        f = io.BytesIO(); im.save(f, fmt, **kw); return f.getvalue()

    with pytest.raises(J.UnsupportedJpeg, match="progressive"):
        J.parse(saved(img, progressive=True))
    with pytest.raises(J.UnsupportedJpeg, match="4 components"):
        J.parse(saved(img.convert("CMYK")))
    with pytest.raises(J.UnsupportedJpeg, match="not a JPEG"):
        J.parse(saved(img, "PNG"))
    base = saved(img.convert("L"), quality=90)
    sof = base.index(b"\xff\xc0")
    with pytest.raises(J.UnsupportedJpeg, match="12-bit"):
        J.parse(base[:sof + 4] + b"\x0c" + base[sof + 5:])
    sos = base.index(b"\xff\xda")
    with pytest.raises(J.UnsupportedJpeg, match="not defined"):
        J.parse(base[:sos + 6] + b"\x11" + base[sos + 7:])
    dht = base.index(b"\xff\xc4")
    bits = bytearray(base[dht + 5: dht + 21])
    donor = next(i for i in range(2, 16) if bits[i] >= 2)
    bits[0] += 2; bits[donor] -= 2                                   # same number of codes, more than the code space holds
    with pytest.raises(J.UnsupportedJpeg, match="over-subscribed"):
        J.parse(base[:dht + 5] + bytes(bits) + base[dht + 21:])
    # a size over the limit, RGB-tagged components, and a second scan
    with pytest.raises(J.UnsupportedJpeg, match="outside"):
        J.parse(saved(Image.new("L", (J.MAX_DIM + 1, 8))))
    with pytest.raises(J.UnsupportedJpeg):
        J.parse(base[:-2] + base[sos:])
    assert J.try_parse(saved(img, "PNG")) is None and J.try_parse(base).buf is None


def test_truncated_and_corrupted_scans_stay_in_bounds(program, tmp_path):
    """Three streams; every 61st truncation point and 200 seeded single-byte corruptions of each scan.  The program must exit 0
    under the sanitizers with a status and a full set of pixels for every image; a truncated scan that still reports status 0 did
    not need the missing bits, so its pixels are those of the whole stream."""
    streams = [(112, 112, S.encode(112, 112, "420", 95, "ramps")), (40, 24, S.encode(40, 24, "444", 100, "noise", restart_marker_blocks=3)),
               (17, 23, S.encode(17, 23, "422", 50, "binary", optimize=True))]
    rng = np.random.RandomState(61)
    batches, n_trunc = [], []
    for w, h, buf in streams:
        p = J.parse(buf)
        plans = []
        for cut in range(0, p.data_len, 61):
            q = copy.copy(p); q.data_len = cut
            plans.append(q)
        n_trunc.append(len(plans))
        for _ in range(200):
            at = p.data_off + int(rng.randint(p.data_len))
            q = copy.copy(p)
            q.buf = buf[:at] + bytes([int(buf[at] ^ rng.randint(1, 256))]) + buf[at + 1:]
            plans.append(q)
        batches.append((plans, h, w))
    flagged = 0
    for (w, h, buf), nt, (plans, _, _), (st, px) in zip(streams, n_trunc, batches, run_batches(program, tmp_path, batches)):
        assert st.shape == (len(plans),) and px.shape == (len(plans), 3, h, w)
        ref = S.pillow_rgb(buf)
        for i in range(nt):
            assert st[i] != 0 or np.array_equal(px[i], ref)
        assert st[0] != 0                                             # an empty scan cannot decode
        flagged += int((st != 0).sum())
    assert flagged > 0
