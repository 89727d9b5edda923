"""CPU: the JPEG stream format and arithmetic as tests/jpeg_ref.py states them (the GPU tests pin the kernels to that model byte
for byte): the quantisation tables of the library, the model against its own entropy decoder, against the exact transform, and
against libjpeg-turbo inside PIL; and that the cases of tests/test_gpu_jpeg_extents.py are what they claim to be."""
import io
import re

import numpy as np
import pytest
from PIL import Image

from minivideo_amd import hotpath
from tests import jpeg_ref as J, test_gpu_jpeg_extents as X

QUALITIES = (1, 50, 75, 100)
# the inputs of the accuracy checks: the GPU tests' content (tests/jpeg_ref.py content(): flat, single-coefficient, sparse and
# noise tiles) at their sizes, and a smooth picture
INPUTS = ((320, 272, 3), (322, 182, 3), (112, 144, 5), (80, 272, 3))


def _smooth(w, h):
    y, x = np.mgrid[0:h, 0:w]
    Y = (128 + 90 * np.sin(x / 23.0) * np.cos(y / 17.0) + 20 * np.sin((x + y) / 3.0)).clip(0, 255).astype(np.uint8)
    c = Y[::2, ::2]
    return np.concatenate([Y.reshape(-1), c.reshape(-1), (255 - c).reshape(-1)])


def _inputs():
    for w, h, seed in INPUTS:
        yield w, h, J.content(w, h, seed)
    yield 320, 272, _smooth(320, 272)


def test_quant_tables_of_the_library():
    assert np.array_equal(hotpath.jpeg_quant_tables(50), np.stack([J.K1_LUMA, J.K2_CHROMA]))
    assert (hotpath.jpeg_quant_tables(100) == 1).all()
    assert (hotpath.jpeg_quant_tables(1) == 255).all()
    for q in (-3, 0, 1, 2, 10, 25, 49, 50, 51, 75, 90, 99, 100, 101, 1000):
        assert np.array_equal(hotpath.jpeg_quant_tables(q), J.quant_tables(q)), q
    assert hotpath.jpeg_header_bytes() == J.HEADER_BYTES == len(J.header(16, 16, 75, 1))


def test_transform_constants():
    M = J.dct_matrix()
    assert np.abs(M).sum(axis=1).max() == 46344                 # the bound the 32-bit argument rests on
    assert sorted(J.ZIGZAG.tolist()) == list(range(64)) and J.ZIGZAG[:6].tolist() == [0, 1, 8, 16, 9, 2]
    for blocks in (np.zeros((1, 8, 8), np.uint8), np.full((1, 8, 8), 255, np.uint8)):   # the extremes stay inside int32
        z = J.transform(blocks)
        assert abs(int(z[0, 0, 0])) + (255 << 19) < 2 ** 31
    ext = np.where(M[:, None, :] * M[0][None, :, None] >= 0, 255, 0).astype(np.uint8)   # sign patterns of every row
    J.transform(ext)


@pytest.mark.parametrize("quality", QUALITIES)
def test_model_against_its_decoder(quality):
    for w, h, R in ((16, 16, None), (40, 22, None), (2, 2, None), (80, 272, 1), (80, 272, 3), (80, 272, 85), (322, 182, None)):
        yuv = J.content(w, h, 3)
        data = J.encode(yuv, w, h, quality, R)
        d = J.decode_levels(data)
        assert (d["w"], d["h"], d["restart"]) == (w, h, R if R else (w + 15) // 16)
        assert np.array_equal(d["qt"], J.quant_tables(quality))
        assert np.array_equal(d["levels"], J.quantised(yuv, w, h, quality))


def test_model_against_the_exact_transform():
    """float64 DCT, round-to-nearest quantisation: no level differs by more than one; at most 1 % differ at all, at every
    quality on its own (measured: 0.0002 % at quality 1, 0.063 % at 50, 0.037 % at 75, 0.51 % at 100)"""
    u, x = np.arange(8)[:, None], np.arange(8)[None, :]
    C = np.where(u == 0, np.sqrt(0.5), 1.0) / 2 * np.cos((2 * x + 1) * u * np.pi / 16)
    differ = total = 0
    for quality in QUALITIES:
        qt = J.quant_tables(quality)
        q = np.stack([qt[0]] * 4 + [qt[1]] * 2).reshape(1, 6, 8, 8)
        d_q = t_q = 0
        for w, h, yuv in _inputs():
            blocks = J.mcu_blocks(yuv, w, h)
            exact = np.rint(np.einsum("vy,...yx,ux->...vu", C, blocks.astype(np.float64) - 128, C) / q)
            model = J.quantise(J.transform(blocks), qt)
            diff = np.abs(model - exact.reshape(-1, 6, 64)[:, :, J.ZIGZAG])
            assert diff.max() <= 1
            d_q += int((diff != 0).sum())
            t_q += diff.size
        print("quality %3d: %.4f %% of the levels differ from the exact transform" % (quality, 100.0 * d_q / t_q))
        assert d_q <= 0.01 * t_q, quality
        differ += d_q
        total += t_q
    print("all qualities: %.4f %%" % (100.0 * differ / total))
    assert differ <= 0.01 * total


def _psnr(a, b):
    return 10 * np.log10(255.0 ** 2 / np.mean((a.astype(np.float64) - b.astype(np.float64)) ** 2))


@pytest.mark.parametrize("quality", QUALITIES)
def test_model_against_pil(quality):
    """PIL opens the model's files, and their luma is as close to the source as PIL's own encode of the same plane with the
    same table (libjpeg-turbo), less 0.1 dB for rounding ties"""
    for w, h, yuv in _inputs():
        data = J.encode(yuv, w, h, quality)
        im = Image.open(io.BytesIO(data))
        assert im.size == (w, h) and im.format == "JPEG"
        im.draft("YCbCr", (w, h))
        assert im.mode == "YCbCr"
        got = np.asarray(im)[:, :, 0]
        src = yuv[:w * h].reshape(h, w)
        buf = io.BytesIO()
        Image.fromarray(src, "L").save(buf, "JPEG", qtables=[J.quant_tables(quality)[0].tolist()])
        own = Image.open(io.BytesIO(buf.getvalue()))
        assert [int(v) for v in own.quantization[0]] == J.quant_tables(quality)[0].tolist()
        a, b = _psnr(got, src), _psnr(np.asarray(own), src)
        print("quality %3d %dx%d: model %.3f dB, PIL %.3f dB, difference %+.3f dB" % (quality, w, h, a, b, a - b))
        assert a >= b - 0.1


def test_huffman_tables_are_those_of_libjpeg():
    """the DHT segments of the model equal the ones libjpeg writes by default (Annex K.3)"""
    buf = io.BytesIO()
    Image.fromarray(np.zeros((16, 16, 3), np.uint8)).save(buf, "JPEG", quality=50)
    theirs = buf.getvalue()

    def dht(d):
        out, i = {}, 2
        while d[i + 1] != 0xda:
            ln = (d[i + 2] << 8) | d[i + 3]
            if d[i + 1] == 0xc4:
                seg, p = d[i + 4:i + 2 + ln], 0
                while p < len(seg):
                    n = sum(seg[p + 1:p + 17])
                    out[seg[p]] = bytes(seg[p + 1:p + 17 + n])
                    p += 17 + n
            i += 2 + ln
        return out

    assert dht(J.header(16, 16, 50, 1)) == dht(theirs) and len(dht(theirs)) == 4


@pytest.mark.parametrize("w,h,restart,quality,intervals", X.INTERVAL_CASES + X.WIDE_CASES)
def test_extent_cases_have_their_interval_counts(w, h, restart, quality, intervals):
    """the model's file holds that many restart intervals (RSTm markers + 1: a 0xFF of the entropy-coded bytes is followed by
    0x00), and the API accepts the picture"""
    body = J.model_file(w, h, X.SEED, quality, restart)[J.HEADER_BYTES:]
    assert len(re.findall(rb"\xff[\xd0-\xd7]", body)) + 1 == intervals and body.endswith(b"\xff\xd9")
    assert w % 2 == 0 and h % 2 == 0 and 2 <= min(w, h) and max(w, h) <= 65534 and w * h <= 1 << 28


def test_extent_cases_straddle_the_chunks():
    counts = sorted(c[4] for c in X.INTERVAL_CASES)
    assert counts[0] == X.SCAN_CHUNK and counts[1] == X.SCAN_CHUNK + 1 and {4 * X.SCAN_CHUNK - 1, 4 * X.SCAN_CHUNK} <= set(counts)
    assert counts[-1] == 16 * X.SCAN_CHUNK
    assert X.BATCH_COUNTS[:2] == (X.PLACE_CHUNK, X.PLACE_CHUNK + 1) and X.BATCH_COUNTS[2] > 2 * X.PLACE_CHUNK


def test_batch_cycle_and_capacity_layout():
    """61 pictures of more than 30 lengths; under the chosen capacity the layout rule refuses exactly picture 2098, the noise
    picture in the third placement chunk, and with one byte less also the last one"""
    _, files = X.batch_pictures(X.BATCH_CYCLE)
    assert len({len(f) for f in files}) > 30
    _, files, cap = X.capacity_batch()
    assert len(files) == 2100 and X.BATCH_NOISE[1] > 2 * X.PLACE_CHUNK > X.BATCH_NOISE[0] > X.PLACE_CHUNK
    lens = [len(f) for f in files]
    assert lens[2098] > lens[2099] and lens[1500] > max(lens[:X.BATCH_CYCLE])
    for c, failed in ((cap, [2098]), (cap - 1, [2098, 2099])):
        lay = J.blob_layout(lens, c)
        assert [k for k, e in enumerate(lay) if e[2] == J.STATUS_TOO_BIG] == failed
        assert all(e[0] + e[1] <= c for e in lay)
    assert J.blob_layout(lens, cap)[2099][0] + lens[2099] == cap


def test_sign_blocks_reach_the_transforms_bound():
    """max |z| beyond 2^30 and within the bound the 32-bit argument rests on; DC levels reach -1024; AC levels stay within the
    +-1023 of the baseline categories (1020, three below)"""
    yuv = X.sign_blocks()
    zmax, ac, dc_lo, dc_hi = X.sign_block_figures(yuv)
    assert (zmax, ac, dc_lo, dc_hi) == (1073883168, 1020, -1024, 1016)
    assert 1 << 30 < zmax <= 46344 * 23173 and zmax + (255 << 19) < 1 << 31
    lv = J.quantised(yuv, 128, 64, 100)
    at = {divmod(int(J.ZIGZAG[k]), 8) for k in range(1, 64) if np.abs(lv[:, :, k]).max() == ac}
    assert (0, 4) in at
    for quality in (1, 50, 100):
        d = J.decode_levels(J.encode(yuv, 128, 64, quality))
        assert np.array_equal(d["levels"], J.quantised(yuv, 128, 64, quality))
