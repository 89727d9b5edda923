"""GPU: the JPEG encoder's chunked passes and its extents (jpeg_encode.hip), byte for byte against the NumPy restatement
(tests/jpeg_ref.py) with the helpers of tests/test_gpu_jpeg.py: pictures of more than 256 restart intervals (jpeg_scan_kernel
hands `carry` from chunk to chunk), calls of more than 1024 pictures (jpeg_place_kernel hands `s_pos` on and applies the
capacity rule per picture), the widest and tallest pictures the API accepts, blocks that reach the bound of the transform's
32-bit argument, and one tall picture through the decode engine.  tests/test_jpeg.py asserts on the model alone that the
cases below are what they claim to be."""
import numpy as np
import pytest

from minivideo_amd import HotPath, gen
from minivideo_amd.hotpath import JPEG_OK, JPEG_TOO_BIG, StreamParams
from oracle import loader
from tests import jpeg_ref as J
from tests.test_gpu_engine_jpeg import _decode
from tests.test_gpu_jpeg import _check, _encode, _one
from tests.util import Stream

pytestmark = pytest.mark.gpu

SCAN_CHUNK = 256        # intervals per pass of jpeg_scan_kernel
PLACE_CHUNK = 1024      # pictures per pass of jpeg_place_kernel

# (w, h, restart_mcus or None = one MCU row, quality, restart intervals per picture)
INTERVAL_CASES = [
    (256, 256, 1, 75, 256),         # exactly one chunk
    (272, 256, 1, 75, 272),
    (272, 272, 1, 100, 289),
    (528, 496, 1, 75, 1023),
    (16, 4112, None, 75, 257),
    (16, 4128, None, 75, 258),
    (16, 16384, None, 75, 1024),
    (2, 65534, None, 75, 4096),     # sixteen whole chunks, chroma planes one sample wide
]
WIDE_CASES = [
    (65534, 2, 64, 75, 64),         # chroma rows of 32 767 samples, 4096 MCUs in one row
    (65534, 2, 7, 75, 586),
    (16384, 16, 64, 75, 16),
    (18, 16384, None, 100, 1024),
]
SEED = 3

BATCH_COUNTS = (1024, 1025, 2100)
BATCH_CYCLE = 61                    # prime: picture k of a batch holds content(16, 16, k % 61)
BATCH_NOISE = (1500, 2098)          # pictures of dense noise at n = 2100: the longest files


@pytest.fixture(scope="module")
def torch_cuda():
    torch = pytest.importorskip("torch")
    assert torch.cuda.is_available(), "no HIP device"
    return torch


@pytest.fixture(scope="module")
def hot():
    h = HotPath(0)
    yield h
    h.close()


@pytest.mark.parametrize("w,h,restart,quality,intervals", INTERVAL_CASES)
def test_interval_counts_around_the_scan_chunk(hot, torch_cuda, w, h, restart, quality, intervals):
    _one(torch_cuda, hot, w, h, SEED, quality, restart)


def test_batch_of_tall_pictures(hot, torch_cuda):
    """five pictures of 258 intervals in one call: every scan workgroup carries its own sums"""
    w, h, n = 16, 4128, 5
    yuv = np.stack([J.content(w, h, 10 + k) for k in range(n)])
    files = [J.model_file(w, h, 10 + k, 75) for k in range(n)]
    assert len({len(f) for f in files}) == n
    table, blob = _encode(torch_cuda, hot, yuv, w, h, 75)
    _check(table, blob, files, blob.size)


@pytest.mark.parametrize("w,h,restart,quality,intervals", WIDE_CASES)
def test_widest_and_tallest_pictures(hot, torch_cuda, w, h, restart, quality, intervals):
    _one(torch_cuda, hot, w, h, SEED, quality, restart)


def batch_pictures(n):
    """(pictures (n, 384), the model's files) of a batch of n pictures of 16 x 16 at quality 75: picture k is one of 61, so a
    picture placed at another one's offset, or a chunk that starts again at offset 0, changes bytes"""
    base = np.stack([J.content(16, 16, s) for s in range(BATCH_CYCLE)])
    base_files = [J.model_file(16, 16, s, 75) for s in range(BATCH_CYCLE)]
    idx = np.arange(n) % BATCH_CYCLE
    return base[idx], [base_files[i] for i in idx]


def capacity_batch():
    """(pictures, files, cap) at n = 2100: pictures 1500 and 2098 hold dense noise; `cap` is exactly what the pictures other
    than 2098 need.  A file is never shorter than its header of 625 bytes and never longer than 838 here, so no picture can be
    refused while two or more follow it that fit: the refused one is the last but one, deep in the third placement chunk, and
    picture 1500 is a long file in the middle of the second."""
    n = 2100
    yuv, files = batch_pictures(n)
    yuv = yuv.copy()
    for k in BATCH_NOISE:
        yuv[k] = np.random.default_rng(k).integers(0, 256, yuv.shape[1], dtype=np.uint8)
        files[k] = J.encode(yuv[k], 16, 16, 75)
    others = J.blob_layout([len(f) for k, f in enumerate(files) if k != BATCH_NOISE[1]], 1 << 40)
    return yuv, files, others[-1][0] + others[-1][1]


@pytest.mark.parametrize("n", BATCH_COUNTS)
def test_batches_across_the_placement_chunk(hot, torch_cuda, n):
    yuv, files = batch_pictures(n)
    assert len({len(f) for f in files}) > 30
    table, blob = _encode(torch_cuda, hot, yuv, 16, 16, 75)
    assert all(int(e["status"]) == JPEG_OK for e in table)
    _check(table, blob, files, blob.size)


def test_capacity_rule_in_a_later_chunk(hot, torch_cuda):
    yuv, files, cap = capacity_batch()
    n, bad = len(files), BATCH_NOISE[1]
    assert bad > PLACE_CHUNK and len(files[bad]) > len(files[-1]) and all(len(files[bad]) > len(f) for f in files[:BATCH_CYCLE])
    room = cap + 3 * len(files[bad])
    for c, failed in ((cap, {bad}), (cap - 1, {bad, n - 1})):
        table, blob = _encode(torch_cuda, hot, yuv, 16, 16, 75, cap=c, room=room)
        status = [int(e["status"]) for e in table]
        assert {k for k in range(n) if status[k] == JPEG_TOO_BIG} == failed and all(int(table[k]["length"]) == 0 for k in failed)
        _check(table, blob, files, c)


def sign_blocks():
    """planar 128 x 64 picture of the 128 blocks sample = 255 where sign * M[v][y] * M[u][x] > 0, else 0 (every (v, u), both
    signs): the inputs that maximise |z[v][u]|.  Luma holds all of them, Cb every fourth, Cr the rows of Cb in reverse."""
    M = J.dct_matrix()
    blocks = np.array([np.where(s * M[v][:, None] * M[u][None, :] > 0, 255, 0) for v in range(8) for u in range(8) for s in (1, -1)],
                      dtype=np.uint8)
    Y = blocks.reshape(8, 16, 8, 8).transpose(0, 2, 1, 3).reshape(64, 128)
    Cb = blocks[::4].reshape(4, 8, 8, 8).transpose(0, 2, 1, 3).reshape(32, 64)
    return np.concatenate([Y.reshape(-1), Cb.reshape(-1), Cb[::-1].reshape(-1)])


def sign_block_figures(yuv):
    """(max |z|, largest |AC level|, least DC level, greatest DC level) of the model at quantisers of 1"""
    z = J.transform(J.mcu_blocks(yuv, 128, 64))
    lv = J.quantised(yuv, 128, 64, 100)
    return int(np.abs(z).max()), int(np.abs(lv[:, :, 1:]).max()), int(lv[:, :, 0].min()), int(lv[:, :, 0].max())


@pytest.mark.parametrize("quality", [1, 50, 100])
def test_blocks_at_the_transforms_bound(hot, torch_cuda, quality):
    yuv = sign_blocks()
    zmax, ac, dc_lo, dc_hi = sign_block_figures(yuv)
    assert 1 << 30 < zmax <= 46344 * 23173 and ac <= 1023 and dc_lo == -1024       # (else the content misses the bound)
    table, blob = _encode(torch_cuda, hot, yuv, 128, 64, quality)
    _check(table, blob, [J.encode(yuv, 128, 64, quality)], blob.size)


def test_tall_picture_through_the_engine():
    """1 x 258 macroblocks, MVHP_OUT_JPEG with default parameters: one MCU per row, 258 intervals -- how a user meets the carry"""
    W, H, F = 1, 258, 2
    stream, packed = gen.make_stream(W, H, F, seed=41, profile="high")
    planes = loader.recon(StreamParams(W, H, 0, 0, 0), packed, F)[0].reshape(F, -1)
    want = [J.encode(planes[k], 16 * W, 16 * H, 75) for k in range(F)]
    assert all(len(f) <= planes.shape[1] for f in want) and want[0] != want[1]
    with Stream(stream) as s:
        assert s.ok
        rc, st, got = _decode(s, list(range(F)), None, 75, contexts=1)
    assert rc == 1 and st["pictures_ok"] == F and st["pictures_failed"] == 0
    for k in range(F):
        assert got[k] == (1, "", (16 * W, 16 * H), want[k]), k
