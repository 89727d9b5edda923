"""CPU: the PNG file format as tests/png_ref.py states it (the GPU tests pin the kernels to that model byte for byte), checked
against things it shares no code with: PIL and zlib decode every file to the input's pixels (PIL verifies every chunk's CRC-32,
zlib the Adler-32), the filter choice against a per-sample raster loop, the codes against Kraft's sum, the library's host
functions against the model, the sizes against the host writer's stored file and zlib's own Huffman-only strategy; and that the
pictures of tests/test_gpu_png.py reach the cases they claim."""
import io
import zlib

import numpy as np
import pytest
from PIL import Image

from minivideo_amd import hotpath
from tests import png_ref as P

# (w, h, seed, kind): the pictures of tests/test_gpu_png.py's test_content, and its widest and tallest sizes
PICTURES = ((322, 182, 3, "content"), (322, 182, 1, "fib"), (16384, 2, 1, "fib"), (64, 64, 0, "flat"), (64, 64, 200, "flat"),
            (64, 64, 1, "noise"), (320, 180, 1, "smooth"), (16384, 2, 1, "smooth3"), (322, 182, 4, "content"), (322, 182, 2, "mixed"),
            (2, 2, 3, "content"), (18, 6, 3, "content"), (2, 16384, 3, "content"), (10922, 2, 3, "content"), (10924, 2, 3, "content"),
            (21844, 2, 3, "content"), (1920, 36, 1, "smooth"))


def _trace(w, h, seed, kind):
    t = P.Trace()
    f = P.encode(P.picture(w, h, seed, kind), w, h, t)
    assert f == P.model_file(w, h, seed, kind)
    return f, t


@pytest.mark.parametrize("w,h,seed,kind", PICTURES)
def test_round_trip(w, h, seed, kind):
    """PIL opens the file (checking every CRC; zlib checks the Adler-32) and finds the input's pixels"""
    f = P.model_file(w, h, seed, kind)
    im = Image.open(io.BytesIO(f))
    assert im.mode == "RGB" and im.size == (w, h)
    assert np.array_equal(np.asarray(im), P.picture(w, h, seed, kind))
    assert len(f) <= P.max_bytes(w, h)


def test_container():
    """signature, IHDR, one IDAT per segment, IEND, nothing else; every IDAT's block starts on a byte: the zlib stream cut at
    the chunk boundaries inflates piece by piece"""
    w, h = 322, 182
    f = P.model_file(w, h, 3)
    assert f[:8] == P.SIGNATURE
    pos, kinds, payloads = 8, [], []
    while pos < len(f):
        n = int.from_bytes(f[pos:pos + 4], "big")
        kinds.append(f[pos + 4:pos + 8])
        payloads.append(f[pos + 8:pos + 8 + n])
        assert zlib.crc32(f[pos + 4:pos + 8 + n]) == int.from_bytes(f[pos + 8 + n:pos + 12 + n], "big")
        pos += 12 + n
    S = -(-h // P.segment_rows(w))
    assert kinds == [b"IHDR"] + [b"IDAT"] * S + [b"IEND"] and S == 6
    d = zlib.decompressobj()
    got = [len(d.decompress(p)) for p in payloads[1:-1]]
    assert got == [33 * 967] * 5 + [17 * 967] and d.eof      # (every piece gives exactly its segment's rows)


def _paeth(a, b, c):
    p = a + b - c
    pa, pb, pc = abs(p - a), abs(p - b), abs(p - c)
    return a if pa <= pb and pa <= pc else (b if pb <= pc else c)


@pytest.mark.parametrize("w,h,seed,kind", [(18, 6, 3, "content"), (40, 22, 5, "content"), (6, 30, 2, "content"), (24, 8, 1, "smooth")])
def test_filter_choice_against_a_raster_loop(w, h, seed, kind):
    img = P.picture(w, h, seed, kind).reshape(h, 3 * w).astype(int)
    types, filt, _ = P.filter_rows(img, w, h)
    for y in range(h):
        best, best_cost, best_row = None, None, None
        for t in range(5):
            row, cost = [], 0
            for i in range(3 * w):
                x = img[y][i]
                a = img[y][i - 3] if i >= 3 else 0
                b = img[y - 1][i] if y else 0
                c = img[y - 1][i - 3] if y and i >= 3 else 0
                pred = (0, a, b, (a + b) >> 1, _paeth(a, b, c))[t]
                f = (x - pred) & 255
                row.append(f)
                cost += f if f < 128 else 256 - f
            if best is None or cost < best_cost:
                best, best_cost, best_row = t, cost, row
        assert types[y] == best and list(filt[y]) == best_row, y


def test_code_shape():
    """every segment's literal code is complete (Kraft sum exactly 1) and no code is longer than 15 bits"""
    for w, h, seed, kind in PICTURES:
        _, t = _trace(w, h, seed, kind)
        for s in t.segments:
            lens = s["lens"]
            assert lens.max() <= 15 and lens[256] >= 1
            assert sum(1 << (15 - int(l)) for l in lens if l) == 1 << 15, (w, h, kind)
    for hist in ([5] + [0] * 255, [0] * 255 + [70000], [1] * 256, list(range(256))):
        lens, _ = P.code_lengths(np.array(hist))
        assert lens.max() <= 15 and sum(1 << (15 - int(l)) for l in lens if l) == 1 << 15
        assert ((lens[:256] > 0) == (np.array(hist) > 0)).all()


def test_content_reaches_every_case():
    f, t = _trace(322, 182, 3, "content")
    assert set(t.types) == {0, 1, 2, 3, 4}                                       # every filter type
    assert [s["rows"] for s in t.segments] == [33] * 5 + [17]                    # a first, middle ones and a short last segment
    _, t4 = _trace(322, 182, 4, "content")
    for tr in (t, t4):
        tied = np.flatnonzero(tr.ties)
        assert tied.size > 0                                                     # flat rows tie, and the lowest type wins
        for y in tied:
            assert tr.types[y] == min(k for k in range(5) if tr.cost[y][k] == tr.cost[y].min())
    _, tn = _trace(64, 64, 1, "noise")
    assert [s["dynamic"] for s in tn.segments] == [False]                        # noise is stored
    _, tm = _trace(322, 182, 2, "mixed")
    assert {s["dynamic"] for s in tm.segments} == {False, True}                  # ... beside dynamic segments of the same file
    assert tm.segments[0]["dynamic"] and tm.segments[-1]["dynamic"] and not tm.segments[2]["dynamic"]
    _, tf = _trace(64, 64, 0, "flat")
    assert tf.segments[0]["used"] == 1 and list(tf.segments[0]["lens"][[0, 256]]) == [1, 1]   # one literal: two codes of one bit
    _, th = _trace(322, 182, 1, "fib")
    assert max(s["halvings"] for s in th.segments) >= 1 and min(s["halvings"] for s in th.segments) == 0
    _, tw = _trace(16384, 2, 1, "fib")
    assert all(s["halvings"] >= 1 and s["bytes"] == 49153 for s in tw.segments)  # the longest row of the issue's sizes
    _, tl = _trace(21844, 2, 3, "content")
    assert all(s["bytes"] == 65533 and s["rows"] == 1 for s in tl.segments)      # the longest row a stored block holds


def test_host_functions():
    assert hotpath.png_header_bytes() == P.HEADER_BYTES
    for w in list(range(1, 40)) + [320, 322, 1920, 5460, 5461, 5462, 10921, 10922, 10923, 10924, 16384, 21844]:
        assert hotpath.png_segment_rows(w) == P.segment_rows(w), w
        for h in (1, 2, 3, 17, 18, 19, 180, 1080, 16384):
            assert hotpath.png_max_bytes(w, h) == P.max_bytes(w, h), (w, h)
    assert hotpath.png_segment_rows(10922) == 1 and hotpath.png_segment_rows(10923) == 1 and hotpath.png_segment_rows(5461) == 2
    assert hotpath.png_segment_rows(0) == 0 and hotpath.png_max_bytes(0, 4) == 0 and hotpath.png_max_bytes(4, 0) == 0
    for w, h, seed, kind in PICTURES:                                            # the bound holds, and noise meets it
        assert len(P.model_file(w, h, seed, kind)) <= hotpath.png_max_bytes(w, h)
    assert len(P.model_file(64, 64, 1, "noise")) == hotpath.png_max_bytes(64, 64)


def _stored_file_bytes(w, h):
    """the host writer's file (export.cpp write_png): filter 0, one IDAT, stored blocks of at most 65 535 bytes"""
    data = h * (3 * w + 1)
    return 8 + 25 + 12 + 2 + 5 * -(-data // 65535) + data + 4 + 12


@pytest.mark.parametrize("w,h", [(320, 180), (1920, 36)])
def test_sizes_on_smooth_content(w, h):
    """smaller than the stored file, and within 2 % of zlib's Huffman-only strategy (one code for the whole picture, no chunking)
    on the same filtered bytes.  Measured: 320 x 180: 75 360 against 74 739 (1.0083); 1920 x 36: 92 881 against 91 972 (1.0099)"""
    assert _stored_file_bytes(320, 180) == 173058
    img = P.picture(w, h, 1, "smooth")
    f = P.model_file(w, h, 1, "smooth")
    types, filt, _ = P.filter_rows(img, w, h)
    stream = np.concatenate([types[:, None], filt], axis=1).tobytes()
    co = zlib.compressobj(6, zlib.DEFLATED, 15, 8, zlib.Z_HUFFMAN_ONLY)
    z = len(co.compress(stream) + co.flush())
    print("%d x %d: file %d, stored file %d, zlib Z_HUFFMAN_ONLY %d, ratio %.4f" % (w, h, len(f), _stored_file_bytes(w, h), z, len(f) / z))
    assert len(f) < _stored_file_bytes(w, h)
    assert len(f) <= 1.02 * z
