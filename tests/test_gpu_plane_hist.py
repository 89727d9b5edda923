"""GPU: the plane-histogram kernel (plane_hist.hip, mvhp_plane_hist_dev) against the NumPy restatement (tests/hist_ref.py): every
record compared as its 3104 raw bytes (reserved words 0), with sentinel bytes before and after the records.  Rectangles whose
head and tail blocks straddle the 16-byte (chroma: 8-byte) boundaries of the source rows, flat pictures (a byte outside the
rectangle that was counted would land in a bin, and every lane adds to one bin), any band size, zero to 300 pictures, the widest
picture, a batch that one launch does not hold, two launches on two streams, and the refused arguments."""
import numpy as np
import pytest

from minivideo_amd import HotPath
from minivideo_amd.hotpath import (LUMA_STATS_DTYPE, PLANE_HIST_DTYPE, MiniVideoError, StreamParams, geometry, hist_stats,
                                   luma_score)
from tests import hist_ref as R, luma_ref as L

pytestmark = pytest.mark.gpu

GUARD = 4096
REC = 3104


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


def _launch(torch, hot, d_src, wmb, hmb, rect, n, stream=None):
    """-> the device buffer of the records between two guard bands (not yet synchronised)"""
    d = torch.full((GUARD + n * REC + GUARD,), 0xA5, dtype=torch.uint8, device=d_src.device)
    torch.cuda.synchronize(d_src.device)
    hot.plane_hist_dev(StreamParams(wmb, hmb, 0, 0, 0), geometry(*rect), d_src.data_ptr(), n, d.data_ptr() + GUARD, stream=stream)
    return d


def _records(d, n):
    raw = d.cpu().numpy()
    assert (raw[:GUARD] == 0xA5).all() and (raw[GUARD + n * REC:] == 0xA5).all(), "bytes around the records changed"
    return raw[GUARD:GUARD + n * REC]


def _device(torch, yuv):
    return torch.from_numpy(np.ascontiguousarray(yuv, dtype=np.uint8).reshape(-1)).to(torch.device("cuda", 0))


def _hist(torch, hot, yuv, wmb, hmb, rect, n=None):
    """yuv: n coded pictures (numpy or a device tensor) -> the raw bytes of the n records"""
    d_src = yuv if isinstance(yuv, torch.Tensor) else _device(torch, yuv)
    n = d_src.numel() // (wmb * hmb * 384) if n is None else n
    d = _launch(torch, hot, d_src, wmb, hmb, rect, n)
    hot.sync_check(None)
    return _records(d, n)


def _check(torch, hot, yuv, wmb, hmb, rect):
    yuv = np.ascontiguousarray(yuv, dtype=np.uint8).reshape(-1, wmb * hmb * 384)
    got = _hist(torch, hot, yuv, wmb, hmb, rect)
    want = R.records(yuv, yuv.shape[0], wmb, hmb, rect)
    if got.tobytes() != want.tobytes():
        g = got.view(PLANE_HIST_DTYPE)
        for k in range(len(want)):
            for p in ("y", "cb", "cr"):
                bad = np.nonzero(g[p][k] != want[p][k])[0]
                assert bad.size == 0, (rect, k, p, bad[:8], g[p][k][bad[:8]], want[p][k][bad[:8]])
        assert False, (rect, g["samples"], g["chroma_samples"], g["reserved"])
    rec = got.view(PLANE_HIST_DTYPE)
    cw, ch = rect[2], rect[3]
    assert (rec["y"].sum(axis=1) == cw * ch).all() and (rec["samples"] == cw * ch).all()
    assert (rec["cb"].sum(axis=1) == cw * ch // 4).all() and (rec["cr"].sum(axis=1) == cw * ch // 4).all()
    assert (rec["chroma_samples"] == cw * ch // 4).all() and not rec["reserved"].any()
    return rec


def _random(wmb, hmb, n, seed):
    return np.random.default_rng(seed).integers(0, 256, (n, wmb * hmb * 384), dtype=np.uint8)


def test_smallest_rectangles(hot, torch_cuda):
    """one macroblock: 2 x 2 at (0, 0) and at (14, 14), and the whole of it; two macroblocks side by side (one is 16 samples
    wide): 4 x 2 at x = 14, which spans two 16-byte blocks of luma and two 8-byte blocks of chroma"""
    yuv = _random(1, 1, 1, 1)
    for rect in ((0, 0, 2, 2), (14, 14, 2, 2), (0, 0, 16, 16), (6, 2, 2, 12)):
        _check(torch_cuda, hot, yuv, 1, 1, rect)
    yuv = _random(2, 1, 2, 2)
    for rect in ((14, 0, 4, 2), (14, 14, 4, 2), (14, 6, 18, 4), (0, 0, 32, 16)):
        _check(torch_cuda, hot, yuv, 2, 1, rect)


def test_rectangles_on_3_by_2(hot, torch_cuda):
    """widths 2, 2 mod 4 and 2 mod 16 (and others), all four sides cropped; crop_x = 2 mod 4 and crop_y = 2 mod 4 give odd chroma
    offsets"""
    yuv = _random(3, 2, 2, 3)
    k = 0
    for cx in (2, 6, 14, 16, 18, 30):
        for cw in (2, 6, 10, 18, 34, 46 - cx):
            if cw < 2 or cx + cw > 46:
                continue
            cy, ch = [(2, 2), (6, 10), (2, 28), (14, 4), (10, 20)][k % 5]
            k += 1
            _check(torch_cuda, hot, yuv, 3, 2, (cx, cy, cw, ch))
    assert k >= 25
    _check(torch_cuda, hot, yuv, 3, 2, (0, 0, 48, 32))


@pytest.mark.parametrize("value", [0, 255, 128])
def test_flat_pictures(hot, torch_cuda, value):
    """one value everywhere, crops that leave head and tail bytes of the rows' first and last blocks outside: a counted byte
    from outside lands in the one populated bin (value 0: the bin a zeroed byte would land in), and every lane adds to one bin"""
    for wmb, hmb, rects in ((5, 3, ((2, 2, 76, 44), (14, 4, 4, 6), (18, 0, 46, 48), (30, 10, 2, 2), (0, 0, 80, 48))),
                            (20, 17, ((6, 10, 300, 250), (0, 0, 320, 272)))):
        yuv = np.full((2, wmb * hmb * 384), value, dtype=np.uint8)
        for rect in rects:
            rec = _check(torch_cuda, hot, yuv, wmb, hmb, rect)
            assert (rec["y"][:, value] == rect[2] * rect[3]).all() and (rec["cb"][:, value] == rect[2] * rect[3] // 4).all()


@pytest.mark.parametrize("inside", [255, 0])
def test_only_the_rectangle_counts(hot, torch_cuda, inside):
    """one value inside the rectangle (in all three planes) and another outside it"""
    wmb, hmb = 5, 3
    for rect in ((2, 2, 76, 44), (14, 4, 4, 6), (18, 0, 46, 48), (0, 2, 80, 2), (30, 10, 2, 2), (16, 16, 48, 16)):
        yuv = np.full((2, wmb * hmb * 384), 255 - inside, dtype=np.uint8)
        cx, cy, cw, ch = rect
        for k in range(2):
            y, cb, cr = R.planes(yuv[k], wmb, hmb)
            y[cy:cy + ch, cx:cx + cw] = inside
            cb[cy // 2:(cy + ch) // 2, cx // 2:(cx + cw) // 2] = inside
            cr[cy // 2:(cy + ch) // 2, cx // 2:(cx + cw) // 2] = inside
        rec = _check(torch_cuda, hot, yuv, wmb, hmb, rect)
        assert (rec["y"][:, 255 - inside] == 0).all() and (rec["cb"][:, 255 - inside] == 0).all() and (rec["cr"][:, 255 - inside] == 0).all()


def test_random_pictures(hot, torch_cuda):
    yuv = _random(20, 17, 3, 5)
    for rect in ((0, 0, 320, 272), (2, 4, 310, 262), (6, 10, 300, 250), (0, 0, 320, 264)):
        _check(torch_cuda, hot, yuv, 20, 17, rect)
    yuv = _random(120, 68, 1, 6)                                      # 1080p: nine automatic bands, the last one short
    _check(torch_cuda, hot, yuv, 120, 68, (0, 0, 1920, 1080))


def test_every_value_once_per_row(hot, torch_cuda):
    """256 samples a luma row, a permutation of 0 .. 255 in every row: each bin of y holds exactly one count per row"""
    wmb, hmb = 16, 2
    rng = np.random.default_rng(8)
    yuv = _random(wmb, hmb, 2, 9)
    for k in range(2):
        y = R.planes(yuv[k], wmb, hmb)[0]
        for r in range(32):
            y[r] = rng.permutation(256)
    rec = _check(torch_cuda, hot, yuv, wmb, hmb, (0, 0, 256, 32))
    assert (rec["y"] == 32).all()
    rec = _check(torch_cuda, hot, yuv, wmb, hmb, (0, 6, 256, 22))
    assert (rec["y"] == 22).all()


def test_any_band_size_gives_the_same_records(hot, torch_cuda):
    """34, 22 and 250 rows are no multiple of most bands; odd bands split the chroma rows unevenly"""
    cases = [(_random(3, 3, 3, 21), 3, 3, (6, 10, 34, 34)), (_random(3, 3, 2, 22), 3, 3, (2, 2, 44, 22)),
             (_random(20, 17, 2, 23), 20, 17, (6, 10, 300, 250))]
    try:
        for yuv, wmb, hmb, rect in cases:
            want = R.records(yuv, yuv.shape[0], wmb, hmb, rect).tobytes()
            for rows in (0, 1, 2, 3, 4, 5, 7, 16, 64, 250, 4096):
                hot.set_hist_band(rows)
                assert _hist(torch_cuda, hot, yuv, wmb, hmb, rect).tobytes() == want, (rect, rows)
    finally:
        hot.set_hist_band(0)


@pytest.mark.parametrize("n", [1, 3, 300])
def test_counts(hot, torch_cuda, n):
    yuv = _random(3, 2, n, 100 + n)
    _check(torch_cuda, hot, yuv, 3, 2, (2, 6, 42, 22))
    _check(torch_cuda, hot, yuv, 3, 2, (0, 0, 48, 32))


def test_no_pictures(hot, torch_cuda):
    d = torch_cuda.full((GUARD,), 0xA5, dtype=torch_cuda.uint8, device=torch_cuda.device("cuda", 0))
    hot.plane_hist_dev(StreamParams(1, 1, 0, 0, 0), geometry(0, 0, 16, 16), d.data_ptr(), 0, d.data_ptr() + 64)
    hot.sync_check(None)
    assert (d.cpu().numpy() == 0xA5).all()


def test_the_widest_picture(hot, torch_cuda):
    yuv = _random(1024, 1, 1, 13)
    _check(torch_cuda, hot, yuv, 1024, 1, (2, 0, 16380, 16))
    _check(torch_cuda, hot, yuv, 1024, 1, (0, 2, 16384, 14))


def test_a_batch_that_one_launch_does_not_hold(hot, torch_cuda):
    """a launch holds 2^23 workgroups: with one-row bands, pictures of 1 x 1024 macroblocks (16384 rows) fill it at 512, so 513
    pictures take two launches.  Seven base pictures, tiled."""
    wmb, hmb, n, cycle = 1, 1024, 513, 7
    rect = (2, 0, 12, 16384)
    assert (1 << 23) // rect[3] == n - 1
    base = _random(wmb, hmb, cycle, 17)
    want = R.records(base, cycle, wmb, hmb, rect)
    reps = (n + cycle - 1) // cycle
    d_src = _device(torch_cuda, base).repeat(reps)[:n * wmb * hmb * 384]
    try:
        hot.set_hist_band(1)
        got = _hist(torch_cuda, hot, d_src, wmb, hmb, rect, n)
    finally:
        hot.set_hist_band(0)
    assert got.tobytes() == np.tile(want, reps)[:n].tobytes()


def test_hist_stats_equals_the_picture_score_record(hot, torch_cuda):
    dev = torch_cuda.device("cuda", 0)
    for yuv, wmb, hmb, rect in ((_random(20, 17, 3, 41), 20, 17, (6, 10, 300, 250)),
                                (np.full((2, 5 * 3 * 384), 255, np.uint8), 5, 3, (2, 2, 76, 44)),
                                (_random(1, 1, 1, 42), 1, 1, (14, 14, 2, 2))):
        n = yuv.shape[0]
        d_src = _device(torch_cuda, yuv)
        d_stats = torch_cuda.zeros(n * 32, dtype=torch_cuda.uint8, device=dev)
        hot.luma_stats_dev(StreamParams(wmb, hmb, 0, 0, 0), geometry(*rect), d_src.data_ptr(), n, d_stats.data_ptr())
        rec = _hist(torch_cuda, hot, d_src, wmb, hmb, rect, n).view(PLANE_HIST_DTYPE)
        stats = d_stats.cpu().numpy()
        for k in range(n):
            st = hist_stats(rec[k])
            assert bytes(st) == stats[32 * k:32 * k + 32].tobytes(), (rect, k)
            assert luma_score(st) == L.picture_score(yuv[k], wmb, hmb, rect)
        assert stats.view(LUMA_STATS_DTYPE)["samples"].tolist() == [rect[2] * rect[3]] * n


def test_two_streams(hot, torch_cuda):
    dev = torch_cuda.device("cuda", 0)
    a, b = _random(20, 17, 40, 31), _random(20, 17, 40, 32)
    da, db = _device(torch_cuda, a), _device(torch_cuda, b)
    s1, s2 = torch_cuda.cuda.Stream(device=dev), torch_cuda.cuda.Stream(device=dev)
    r1 = _launch(torch_cuda, hot, da, 20, 17, (2, 2, 316, 268), 40, stream=s1.cuda_stream)
    r2 = _launch(torch_cuda, hot, db, 20, 17, (0, 0, 320, 272), 40, stream=s2.cuda_stream)
    hot.sync_check(s1.cuda_stream)
    hot.sync_check(s2.cuda_stream)
    assert _records(r1, 40).tobytes() == R.records(a, 40, 20, 17, (2, 2, 316, 268)).tobytes()
    assert _records(r2, 40).tobytes() == R.records(b, 40, 20, 17, (0, 0, 320, 272)).tobytes()


def test_refused_arguments_launch_nothing(hot, torch_cuda):
    dev = torch_cuda.device("cuda", 0)
    d = torch_cuda.full((1 << 16,), 7, dtype=torch_cuda.uint8, device=dev)
    base = (d.data_ptr() + 15) & ~15
    p = StreamParams(2, 2, 0, 0, 0)
    bad = [(0, 0, 34, 16), (0, 0, 16, 34), (20, 0, 14, 16), (0, 30, 16, 4), (1, 0, 16, 16), (0, 1, 16, 16), (0, 0, 15, 16),
           (0, 0, 16, 15), (0, 0, 0, 16), (0, 0, 16, 0), (32, 0, 2, 2), (0xFFFFFFFE, 0, 4, 4)]
    for rect in bad:
        with pytest.raises(MiniVideoError):
            hot.plane_hist_dev(p, geometry(*rect), base, 1, base + 32768)
    whole = geometry(0, 0, 32, 32)
    with pytest.raises(MiniVideoError):
        hot.plane_hist_dev(p, whole, base, -1, base + 32768)
    for off in (4, 8):
        with pytest.raises(MiniVideoError):
            hot.plane_hist_dev(p, whole, base, 1, base + 32768 + off)   # records are 16-byte aligned
    with pytest.raises(MiniVideoError):
        hot.plane_hist_dev(p, whole, base + 8, 1, base + 32768)        # pictures too
    with pytest.raises(MiniVideoError):
        hot.plane_hist_dev(p, whole, None, 1, base + 32768)
    with pytest.raises(MiniVideoError):
        hot.plane_hist_dev(p, whole, base, 1, None)
    torch_cuda.cuda.synchronize(dev)
    assert (d.cpu().numpy() == 7).all()
