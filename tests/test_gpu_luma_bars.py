"""GPU: the black-bar kernels (luma_bars.hip, mvhp_luma_bars_dev) against the NumPy restatement (tests/bars_ref.py): every record
compared field by field and as its 32 raw bytes (reserved words 0), with guard bytes before and after the records.  The planes
are filled, never zero outside the rectangle, so a read outside it shows.  Rectangles whose head and tail blocks straddle the
16-byte boundaries of the source rows, any band size, the packed column counters at and beyond 255 rows, the level and the
need at their edges, the empty records, one to 65 537 pictures, stale scratch, planes that come from the reconstruction and
deblocking kernels, two streams, and the refused arguments."""
import numpy as np
import pytest

from minivideo_amd import HotPath, gen
from minivideo_amd.hotpath import LUMA_BARS_DTYPE, PARAM_DEBLOCK, STREAM_DEBLOCK, MiniVideoError, StreamParams, geometry
from oracle import loader
from tests import bars_ref as B
from tests import deblock_ref
from tests.test_deblock import DStream

pytestmark = pytest.mark.gpu

GUARD = 4096
FIELDS = ("x", "y", "w", "h", "rows", "cols")


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


def _launch(torch, hot, d_src, wmb, hmb, rect, n, level, stream=None):
    """-> the device buffer of the records between two guard bands (not yet synchronised)"""
    d = torch.full((GUARD + n * 32 + GUARD,), 0xA5, dtype=torch.uint8, device=d_src.device)
    torch.cuda.synchronize(d_src.device)
    hot.luma_bars_dev(StreamParams(wmb, hmb, 0, 0, 0), geometry(*rect), d_src.data_ptr(), n, level, d.data_ptr() + GUARD, stream=stream)
    return d


def _records(d, n):
    raw = d.cpu().numpy()
    assert (raw[:GUARD] == 0xA5).all() and (raw[GUARD + n * 32:] == 0xA5).all(), "bytes around the records changed"
    return raw[GUARD:GUARD + n * 32]


def _bars(torch, hot, yuv, wmb, hmb, rect, level=B.LEVEL, n=None):
    """yuv: n coded pictures (numpy or a device tensor) -> the raw bytes of the n records"""
    dev = torch.device("cuda", 0)
    d_src = yuv if isinstance(yuv, torch.Tensor) else torch.from_numpy(np.ascontiguousarray(yuv, dtype=np.uint8).reshape(-1)).to(dev)
    n = d_src.numel() // (wmb * hmb * 384) if n is None else n
    d = _launch(torch, hot, d_src, wmb, hmb, rect, n, level)
    hot.sync_check(None)
    return _records(d, n)


def _same(got, want, what):
    got, want = np.frombuffer(got.tobytes(), LUMA_BARS_DTYPE), np.frombuffer(want.tobytes(), LUMA_BARS_DTYPE)
    assert len(got) == len(want)
    for f in FIELDS:
        bad = np.flatnonzero(got[f] != want[f])
        assert len(bad) == 0, (what, f, int(bad[0]), got[bad[0]], want[bad[0]])
    assert got.tobytes() == want.tobytes(), what


def _six(rec):
    return [int(rec[f]) for f in FIELDS]


def _check(torch, hot, yuv, wmb, hmb, rect, level=B.LEVEL):
    yuv = np.ascontiguousarray(yuv, dtype=np.uint8).reshape(-1, wmb * hmb * 384)
    want = B.records(yuv, yuv.shape[0], wmb, hmb, rect, level)
    _same(_bars(torch, hot, yuv, wmb, hmb, rect, level), want, (rect, level))
    return want


def _filled(wmb, hmb, n, seed, fill=255):
    """n pictures whose luma is `fill` and whose chroma is random"""
    yuv = np.random.default_rng(seed).integers(1, 256, (n, wmb * hmb * 384), dtype=np.uint8)
    yuv[:, :256 * wmb * hmb] = fill
    return yuv


def _mixed(wmb, hmb, n, seed, dark=0.6):
    """random pictures of which about `dark` of the luma samples are at or below the default level"""
    rng = np.random.default_rng(seed)
    yuv = rng.integers(25, 256, (n, wmb * hmb * 384), dtype=np.uint8)
    low = rng.integers(0, 25, yuv.shape, dtype=np.uint8)
    return np.where(rng.random(yuv.shape) < dark, low, yuv)


def _planes(yuv, wmb, hmb):
    return [B.luma_plane(p, wmb, hmb) for p in yuv]


def test_one_macroblock(hot, torch_cuda):
    yuv = _mixed(1, 1, 2, 1)
    for rect in ((0, 0, 2, 2), (14, 14, 2, 2), (2, 6, 2, 2), (0, 0, 16, 16)):
        _check(torch_cuda, hot, yuv, 1, 1, rect)
    bright = _filled(1, 1, 1, 2)                               # bright everywhere but inside the rectangle
    for rect in ((0, 0, 2, 2), (14, 14, 2, 2), (2, 6, 2, 2)):
        y = bright.copy()
        cx, cy, cw, ch = rect
        B.luma_plane(y[0], 1, 1)[cy:cy + ch, cx:cx + cw] = 24
        assert _six(_check(torch_cuda, hot, y, 1, 1, rect)[0]) == [0, 0, 0, 0, 0, 0]


@pytest.mark.parametrize("cx", [2, 14, 16, 18])
def test_heads_and_tails(hot, torch_cuda, cx):
    """3 x 2 macroblocks: the heads and tails of the 16-byte blocks at every position; bright samples just outside every side of
    the rectangle must not count"""
    wmb, hmb = 3, 2
    k = 0
    for cw in (2, 6, 18, 30):
        for cy, ch in ((2, 28), (0, 32), (6, 2), (30, 2)):
            rect = (cx, cy, cw, ch)
            _check(torch_cuda, hot, _mixed(wmb, hmb, 2, 10 * cx + k), wmb, hmb, rect)
            y = _filled(wmb, hmb, 2, 3)                        # a frame of 255 around a rectangle that is dark but for one sample
            Y = _planes(y, wmb, hmb)
            Y[0][cy:cy + ch, cx:cx + cw] = 24
            Y[1][cy:cy + ch, cx:cx + cw] = 0
            Y[1][cy + ch - 1, cx + cw - 1] = 25
            want = _check(torch_cuda, hot, y, wmb, hmb, rect)
            assert _six(want[0]) == [0, 0, 0, 0, 0, 0]
            assert _six(want[1]) == [cx + cw - 1, cy + ch - 1, 1, 1, 1, 1]
            k += 1


def test_any_band_size_gives_the_same_records(hot, torch_cuda):
    wmb, hmb = 5, 20
    yuv = _mixed(wmb, hmb, 3, 21, dark=0.97)
    for Y in _planes(yuv, wmb, hmb):
        Y[:37] = 16
        Y[301:] = 7
    rect = (6, 10, 70, 306)
    want = B.records(yuv, 3, wmb, hmb, rect)
    assert 0 < want[0]["rows"] < 306
    try:
        for rows in (1, 2, 3, 16, 255, 256, 65536):
            hot.set_bars_band(rows)
            _same(_bars(torch_cuda, hot, yuv, wmb, hmb, rect), want, rows)
    finally:
        hot.set_bars_band(0)
    _same(_bars(torch_cuda, hot, yuv, wmb, hmb, rect), want, "default")
    for bad in (-1, 65537):
        with pytest.raises(MiniVideoError):
            hot.set_bars_band(bad)


@pytest.mark.parametrize("wmb,hmb", [(5, 65), (70, 40), (130, 20)])
def test_a_column_bright_in_every_row(hot, torch_cuda, wmb, hmb):
    """the packed byte counters: a lane adds one per row to a byte and must empty it before 256 -- a narrow picture keeps four
    rows in flight (a lane sees every fourth row), a wider one two, the widest a single row (a lane sees every row of its tile)"""
    W, H = 16 * wmb, 16 * hmb
    yuv = _filled(wmb, hmb, 1, 5, fill=16)
    Y = B.luma_plane(yuv[0], wmb, hmb)
    Y[:, 5] = 255
    Y[:, W - 3] = 30
    Y[:, 16:16 + W // 16] = 200                                # (enough of them to make every row content)
    Y[7, 40:44] = 90                                           # a few samples more, far below a column's need
    want = B.records(yuv, 1, wmb, hmb, (0, 0, W, H))
    assert _six(want[0]) == [5, 0, W - 7, H, H, 2 + W // 16]
    try:
        for rows in (255, 256, 1024, 65536, 0):
            hot.set_bars_band(rows)
            _same(_bars(torch_cuda, hot, yuv, wmb, hmb, (0, 0, W, H)), want, rows)
            _check(torch_cuda, hot, yuv, wmb, hmb, (4, 2, W - 6, H - 4))
    finally:
        hot.set_bars_band(0)


@pytest.mark.parametrize("level", [1, 24, 254])
def test_level(hot, torch_cuda, level):
    """samples exactly at the level do not count, samples one above do"""
    wmb, hmb = 4, 4
    yuv = _filled(wmb, hmb, 3, 6, fill=level)
    Y = _planes(yuv, wmb, hmb)
    Y[1][20:30, 8:50] = level + 1
    Y[2][:] = level - 1
    Y[2][3, 2:5] = level + 1
    Y[2][5, 2:5] = 255
    want = _check(torch_cuda, hot, yuv, wmb, hmb, (0, 0, 64, 64), level)
    assert _six(want[0]) == [0, 0, 0, 0, 0, 0]
    assert _six(want[1]) == [8, 20, 42, 10, 10, 42]
    assert _six(want[2]) == [2, 3, 3, 3, 2, 3]
    _check(torch_cuda, hot, yuv, wmb, hmb, (2, 2, 60, 58), level)


def test_refused_levels(hot, torch_cuda):
    dev = torch_cuda.device("cuda", 0)
    d = torch_cuda.full((1 << 16,), 7, dtype=torch_cuda.uint8, device=dev)
    base = (d.data_ptr() + 15) & ~15
    for level in (0, 255, -1, 256, 1000):
        with pytest.raises(MiniVideoError):
            hot.luma_bars_dev(StreamParams(2, 2, 0, 0, 0), geometry(0, 0, 32, 32), base, 1, level, base + 32768)
    torch_cuda.cuda.synchronize(dev)
    assert (d.cpu().numpy() == 7).all()


@pytest.mark.parametrize("cw,ch", [(64, 64), (96, 64), (64, 96)])
def test_need_minus_one_and_need(hot, torch_cuda, cw, ch):
    """rows and columns with exactly need - 1 and exactly need bright samples"""
    wmb, hmb = 7, 7
    nr, nc = B.need(cw), B.need(ch)
    assert (nr, nc) == (cw >> 5, ch >> 5) and nr >= 2 and nc >= 2
    cx, cy = 6, 10
    yuv = _filled(wmb, hmb, 2, 8)
    for k, Y in enumerate(_planes(yuv, wmb, hmb)):
        Y[cy:cy + ch, cx:cx + cw] = 16
        # rows: row 4 has need bright samples, row 9 one fewer; they sit in columns that stay below the column's need
        for j in range(nr):
            Y[cy + 4, cx + 3 * j] = 200
        for j in range(nr - 1):
            Y[cy + 9, cx + 40 + j] = 200
        # columns: column 30 has need bright samples, column 33 one fewer, each in a row of its own
        for j in range(nc):
            Y[cy + 20 + 2 * j, cx + 30] = 200
        for j in range(nc - 1):
            Y[cy + 40 + 2 * j, cx + 33] = 200
        if k == 1:
            Y[cy + 9, cx + 50] = 200                          # the second picture: row 9 reaches the need
    want = _check(torch_cuda, hot, yuv, wmb, hmb, (cx, cy, cw, ch))
    assert _six(want[0]) == [cx + 30, cy + 4, 1, 1, 1, 1]
    assert _six(want[1]) == [cx + 30, cy + 4, 1, 6, 2, 1]


def test_empty_records(hot, torch_cuda):
    wmb, hmb = 4, 4
    yuv = _filled(wmb, hmb, 3, 9, fill=16)
    Y = _planes(yuv, wmb, hmb)
    Y[1][3, 0:2] = 99                                          # a content row (need 2), its samples in columns with one each (need 2)
    Y[2][0:2, 3] = 99                                          # the transpose: a content column and no content row
    want = _check(torch_cuda, hot, yuv, wmb, hmb, (0, 0, 64, 64))
    assert _six(want[0]) == [0, 0, 0, 0, 0, 0]
    assert _six(want[1]) == [0, 0, 0, 0, 1, 0]
    assert _six(want[2]) == [0, 0, 0, 0, 0, 1]


def test_one_row_one_column_and_the_borders(hot, torch_cuda):
    wmb, hmb = 2, 2
    yuv = _filled(wmb, hmb, 6, 10, fill=16)
    Y = _planes(yuv, wmb, hmb)
    Y[0][13, 21] = 25                                          # 32 x 32: need is 1
    Y[1][0, :] = 200                                           # content touching each of the four borders
    Y[2][31, :] = 200
    Y[3][:, 0] = 200
    Y[4][:, 31] = 200
    Y[5][0, 0] = Y[5][31, 31] = 200
    want = _check(torch_cuda, hot, yuv, wmb, hmb, (0, 0, 32, 32))
    assert [_six(w) for w in want] == [[21, 13, 1, 1, 1, 1], [0, 0, 32, 1, 1, 32], [0, 31, 32, 1, 1, 32], [0, 0, 1, 32, 32, 1],
                                               [31, 0, 1, 32, 32, 1], [0, 0, 32, 32, 2, 2]]
    yuv = _filled(wmb, hmb, 4, 10)                             # the same inside a bright frame
    Y = _planes(yuv, wmb, hmb)
    for k in range(4):
        Y[k][2:30, 4:28] = 16
    Y[0][2, 4:28] = 200
    Y[1][29, 4:28] = 200
    Y[2][2:30, 4] = 200
    Y[3][2:30, 27] = 200
    want = _check(torch_cuda, hot, yuv, wmb, hmb, (4, 2, 24, 28))
    assert [_six(w)[:4] for w in want] == [[4, 2, 24, 1], [4, 29, 24, 1], [4, 2, 1, 28], [27, 2, 1, 28]]


def test_a_bright_line_inside_a_bar(hot, torch_cuda):
    wmb, hmb = 8, 6
    yuv = _filled(wmb, hmb, 2, 11, fill=16)
    Y = _planes(yuv, wmb, hmb)
    rng = np.random.default_rng(3)
    for k in range(2):
        Y[k][20:70, :] = rng.integers(30, 256, (50, 128), dtype=np.uint8)
    Y[1][5, 10:100] = 180                                      # a subtitle in the top bar: the box spans it, `rows` counts it
    want = _check(torch_cuda, hot, yuv, wmb, hmb, (0, 0, 128, 96))
    assert _six(want[0]) == [0, 20, 128, 50, 50, 128]
    assert _six(want[1]) == [0, 5, 128, 65, 51, 128]


@pytest.mark.parametrize("wmb,hmb", [(1024, 1), (1, 1024)])
@pytest.mark.parametrize("where", ["first", "last"])
def test_the_widest_and_the_tallest_picture(hot, torch_cuda, wmb, hmb, where):
    W, H = 16 * wmb, 16 * hmb
    yuv = _filled(wmb, hmb, 1, 12, fill=16)
    Y = B.luma_plane(yuv[0], wmb, hmb)
    if wmb > 1:
        x0 = 0 if where == "first" else W - 16
        Y[:, x0:x0 + 16] = 77
    else:
        y0 = 0 if where == "first" else H - 16
        Y[y0:y0 + 16, :] = 77
    # sixteen bright samples are no content in a line of 16384 (the need is 512): the long axis counts them, the box is empty
    want = _check(torch_cuda, hot, yuv, wmb, hmb, (0, 0, W, H))
    assert _six(want[0]) == ([0, 0, 0, 0, 0, 16] if wmb > 1 else [0, 0, 0, 0, 16, 0])
    _check(torch_cuda, hot, yuv, wmb, hmb, (2, 2, W - 4, H - 4))
    near = (0 if where == "first" else W - 32, 0, 32, 16) if wmb > 1 else (0, 0 if where == "first" else H - 32, 16, 32)
    want = _check(torch_cuda, hot, yuv, wmb, hmb, near)         # in a rectangle of 32 around it the block is content
    assert _six(want[0])[2:6] == [16, 16, 16, 16]
    Y[:] = 255
    assert _six(_check(torch_cuda, hot, yuv, wmb, hmb, (0, 0, W, H))[0]) == [0, 0, W, H, H, W]


def _varied(wmb, hmb, n, seed):
    """n letterboxed and pillarboxed pictures, every one with other bars"""
    rng = np.random.default_rng(seed)
    W, H = 16 * wmb, 16 * hmb
    yuv = _filled(wmb, hmb, n, seed, fill=16)
    for k, Y in enumerate(_planes(yuv, wmb, hmb)):
        if k % 11 == 10:
            continue                                           # (all black)
        x0, y0 = int(rng.integers(0, W // 3)), int(rng.integers(0, H // 3))
        x1, y1 = int(rng.integers(2 * W // 3, W + 1)), int(rng.integers(2 * H // 3, H + 1))
        Y[y0:y1, x0:x1] = rng.integers(0, 256, (y1 - y0, x1 - x0), dtype=np.uint8)
    return yuv


@pytest.mark.parametrize("n", [1, 5, 300])
def test_counts(hot, torch_cuda, n):
    yuv = _varied(20, 17, n, 100 + n)
    want = _check(torch_cuda, hot, yuv, 20, 17, (2, 4, 310, 262))
    assert n == 1 or len({w.tobytes() for w in want}) > n // 2
    _check(torch_cuda, hot, yuv, 20, 17, (0, 0, 320, 272))


def test_more_pictures_than_a_grid_dimension(hot, torch_cuda):
    n = 65537
    seven = _varied(1, 1, 7, 13)
    Y = _planes(seven, 1, 1)
    Y[3][:] = 16
    Y[5][4:9, 2:14] = 200
    rect = (2, 2, 12, 10)
    want7 = B.records(seven, 7, 1, 1, rect)
    assert len({w.tobytes() for w in want7}) == 7
    idx = np.arange(n) % 7
    _same(_bars(torch_cuda, hot, seven[idx], 1, 1, rect), want7[idx], "65537 pictures")


def test_no_pictures(hot, torch_cuda):
    d = torch_cuda.full((GUARD,), 0xA5, dtype=torch_cuda.uint8, device=torch_cuda.device("cuda", 0))
    hot.luma_bars_dev(StreamParams(1, 1, 0, 0, 0), geometry(0, 0, 16, 16), d.data_ptr(), 0, 24, d.data_ptr() + 64)
    hot.sync_check(None)
    assert (d.cpu().numpy() == 0xA5).all()


def test_stale_scratch(hot, torch_cuda):
    """two calls back to back on one context: the first bright everywhere on a larger geometry, the second a smaller letterboxed
    one -- its records are the model's only if the call zeroes the column counters"""
    big = _filled(20, 17, 6, 14)
    small = _filled(8, 6, 6, 15, fill=16)
    for k, Y in enumerate(_planes(small, 8, 6)):
        Y[20 + k:70, 8:120 - k] = 120
    for _ in range(2):
        assert _six(_check(torch_cuda, hot, big, 20, 17, (0, 0, 320, 272))[0]) == [0, 0, 320, 272, 272, 320]
        want = _check(torch_cuda, hot, small, 8, 6, (0, 0, 128, 96))
        assert _six(want[3]) == [8, 23, 109, 47, 47, 109]


def test_two_streams(hot, torch_cuda):
    dev = torch_cuda.device("cuda", 0)
    a, b = _filled(20, 17, 40, 31), _varied(8, 6, 40, 32)
    da, db = (torch_cuda.from_numpy(x.reshape(-1)).to(dev) for x in (a, b))
    s1, s2 = torch_cuda.cuda.Stream(device=dev), torch_cuda.cuda.Stream(device=dev)
    r1 = _launch(torch_cuda, hot, da, 20, 17, (2, 2, 316, 268), 40, 24, stream=s1.cuda_stream)
    r2 = _launch(torch_cuda, hot, db, 8, 6, (0, 0, 128, 96), 40, 24, stream=s2.cuda_stream)
    r3 = _launch(torch_cuda, hot, da, 20, 17, (0, 0, 320, 272), 40, 200, stream=s1.cuda_stream)
    hot.sync_check(s1.cuda_stream)
    hot.sync_check(s2.cuda_stream)
    _same(_records(r1, 40), B.records(a, 40, 20, 17, (2, 2, 316, 268)), "stream 1")
    _same(_records(r2, 40), B.records(b, 40, 8, 6, (0, 0, 128, 96)), "stream 2")
    _same(_records(r3, 40), B.records(a, 40, 20, 17, (0, 0, 320, 272), 200), "stream 1 again")


@pytest.mark.parametrize("deblock", [False, True])
def test_planes_from_the_device(hot, torch_cuda, deblock):
    W, H, F = 9, 7, 3
    dev = torch_cuda.device("cuda", 0)
    kw = dict(deblock=dict(idc=(0, 1, 2), offsets=(-6, 6))) if deblock else {}
    stream, packed, _ = gen.make_stream_ex(W, H, F, seed=23, profile="high", **kw)
    with DStream(stream, STREAM_DEBLOCK if deblock else 0) as s:
        assert s.ok
        p = s.params(0)
        assert bool(p.flags & PARAM_DEBLOCK) == deblock
        off = StreamParams.from_buffer_copy(p)
        off.flags = p.flags & ~PARAM_DEBLOCK
        ref = loader.recon(off, packed, F)[0]
        if deblock:
            ref = deblock_ref.deblock(ref, packed, p)
        ref = np.asarray(ref).reshape(F, -1)
        d_packed = torch_cuda.from_numpy(np.ascontiguousarray(packed).reshape(-1)).to(dev)
        d_yuv = torch_cuda.zeros(F * p.yuv_bytes, dtype=torch_cuda.uint8, device=dev)
        hot.recon_dev(p, d_packed.data_ptr(), F, d_yuv.data_ptr())
        levels = sorted(int(v) for v in np.percentile(ref[:, :256 * W * H], (10, 50, 97)))
        for rect in ((0, 0, 16 * W, 16 * H), (2, 6, 16 * W - 6, 16 * H - 8)):
            for level in [24] + [min(max(v, 1), 254) for v in levels]:
                d = torch_cuda.full((GUARD + F * 32 + GUARD,), 0xA5, dtype=torch_cuda.uint8, device=dev)
                hot.luma_bars_dev(p, geometry(*rect), d_yuv.data_ptr(), F, level, d.data_ptr() + GUARD)   # (behind the reconstruction)
                hot.sync_check(None)
                _same(_records(d, F), B.records(ref, F, W, H, rect, level), (rect, level))


def test_refused_arguments(hot, torch_cuda):
    dev = torch_cuda.device("cuda", 0)
    d = torch_cuda.full((1 << 16,), 7, dtype=torch_cuda.uint8, device=dev)
    base = (d.data_ptr() + 15) & ~15
    p = StreamParams(2, 2, 0, 0, 0)
    bad = [(0, 0, 34, 16), (0, 0, 16, 34), (20, 0, 14, 16), (0, 30, 16, 4), (1, 0, 16, 16), (0, 1, 16, 16), (0, 0, 15, 16),
           (0, 0, 16, 15), (0, 0, 0, 16), (0, 0, 16, 0), (32, 0, 2, 2), (0xFFFFFFFE, 0, 4, 4)]
    for rect in bad:
        with pytest.raises(MiniVideoError):
            hot.luma_bars_dev(p, geometry(*rect), base, 1, 24, base + 32768)
    with pytest.raises(MiniVideoError):
        hot.luma_bars_dev(p, geometry(0, 0, 32, 32), base, -1, 24, base + 32768)
    with pytest.raises(MiniVideoError):
        hot.luma_bars_dev(p, geometry(0, 0, 32, 32), base, 1, 24, base + 32768 + 4)      # records are 8-byte aligned
    with pytest.raises(MiniVideoError):
        hot.luma_bars_dev(p, geometry(0, 0, 32, 32), base + 8, 1, 24, base + 32768)      # pictures 16-byte aligned
    with pytest.raises(MiniVideoError):
        hot.luma_bars_dev(p, geometry(0, 0, 32, 32), None, 1, 24, base + 32768)
    with pytest.raises(MiniVideoError):
        hot.luma_bars_dev(p, geometry(0, 0, 32, 32), base, 1, 24, None)
    torch_cuda.cuda.synchronize(dev)
    assert (d.cpu().numpy() == 7).all()
