"""GPU: the JPEG encoder (jpeg_encode.hip, mvhp_jpeg_encode_dev) byte for byte against the NumPy restatement (tests/jpeg_ref.py):
picture sizes with partial MCUs, restart intervals, content that reaches every case of the entropy coder, qualities, batches,
the blob's layout and capacity rule, and planes that come from the reconstruction, deblocking and geometry kernels."""
import numpy as np
import pytest

from minivideo_amd import HotPath, gen
from minivideo_amd.hotpath import (JPEG_ENTRY_DTYPE, JPEG_OK, JPEG_TOO_BIG, PARAM_DEBLOCK, STREAM_DEBLOCK, MiniVideoError,
                                   StreamParams, geometry, output_geometry)
from oracle import loader
from tests import deblock_ref, jpeg_ref as J, resample_ref
from tests.test_deblock import DStream
from tests.util import Stream

pytestmark = pytest.mark.gpu

GUARD = 4096


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


def _encode(torch, hot, yuv, w, h, quality, restart=0, cap=None, room=None):
    """yuv (n, w * h * 3 / 2) -> (table, blob bytes [0, room)); the bytes before the blob, from `cap` on, and around the table
    must keep their fill"""
    dev = torch.device("cuda", 0)
    yuv = np.ascontiguousarray(yuv, dtype=np.uint8).reshape(-1, w * h * 3 // 2)
    n = yuv.shape[0]
    room = n * ((J.HEADER_BYTES + w * h * 3 + 64 + 15) & ~15) if room is None else room
    cap = room if cap is None else cap
    assert cap <= room
    d_src = torch.from_numpy(yuv.reshape(-1)).to(dev)
    d_blob = torch.full((GUARD + room + GUARD,), 0xA5, dtype=torch.uint8, device=dev)
    d_tab = torch.full((GUARD + n * 16 + GUARD,), 0x5A, dtype=torch.uint8, device=dev)
    torch.cuda.synchronize(dev)
    hot.jpeg_encode_dev(geometry(0, 0, w, h), d_src.data_ptr(), n, d_blob.data_ptr() + GUARD, cap, d_tab.data_ptr() + GUARD,
                        quality=quality, restart_mcus=restart)
    hot.sync_check(None)
    blob, tab = d_blob.cpu().numpy(), d_tab.cpu().numpy()
    assert (blob[:GUARD] == 0xA5).all() and (blob[GUARD + cap:] == 0xA5).all(), "bytes outside the blob's capacity changed"
    assert (tab[:GUARD] == 0x5A).all() and (tab[GUARD + n * 16:] == 0x5A).all(), "bytes around the table changed"
    return tab[GUARD:GUARD + n * 16].view(JPEG_ENTRY_DTYPE), blob[GUARD:GUARD + room]


def _check(table, blob, files, cap):
    """the table is the layout rule applied to the model's lengths, every file that fits is the model's, and no other byte of
    the blob changed"""
    want = J.blob_layout([len(f) for f in files], cap)
    assert [(int(e["offset"]), int(e["length"]), int(e["status"])) for e in table] == want
    expect = np.full(blob.size, 0xA5, dtype=np.uint8)
    for (off, ln, st), f in zip(want, files):
        assert off % 16 == 0
        if st == J.STATUS_OK:
            expect[off:off + ln] = np.frombuffer(f, dtype=np.uint8)
    bad = np.flatnonzero(blob != expect)
    assert bad.size == 0, "first differing byte of the blob: %d" % bad[0]


def _one(torch, hot, w, h, seed, quality, restart=None):
    table, blob = _encode(torch, hot, J.content(w, h, seed), w, h, quality, restart or 0)
    _check(table, blob, [J.model_file(w, h, seed, quality, restart)], blob.size)


@pytest.mark.parametrize("w,h", [(16, 16), (32, 16), (16, 32), (320, 272), (2, 2), (18, 18), (322, 182), (40, 22)])
def test_sizes(hot, torch_cuda, w, h):
    _one(torch_cuda, hot, w, h, 3, 100)


def test_content_reaches_every_case():
    """on the model's output: the pictures of test_sizes / test_restart_intervals make the entropy coder meet every case"""
    ev = J.events(J.content(320, 272, 3), 320, 272, 100)
    assert ev.dc_cat == set(range(12)) and ev.ac_cat == set(range(1, 11))
    assert {15, 16, 17, 33} <= ev.runs and max(ev.runs) >= 33
    assert ev.no_eob > 0 and ev.zero_blocks > 0 and ev.stuffed > 0
    ev = J.events(J.content(80, 272, 3), 80, 272, 100, 1)
    assert ev.stuffed_at_end > 0 and ev.dc_cat == set(range(12))


@pytest.mark.parametrize("rows", [9, 17])
@pytest.mark.parametrize("restart", [None, 1, 3, "all"])
def test_restart_intervals(hot, torch_cuda, rows, restart):
    """5 MCUs per row: RSTm passes 7 -> 0 (9 intervals and more), and 85 MCUs in intervals of 3 leave a last one of 1"""
    w, h = 80, rows * 16
    _one(torch_cuda, hot, w, h, 3, 100, 5 * rows if restart == "all" else restart)


@pytest.mark.parametrize("quality", [1, 50, 75, 100])
def test_qualities(hot, torch_cuda, quality):
    _one(torch_cuda, hot, 112, 144, 5, quality)
    _one(torch_cuda, hot, 322, 182, 3, quality)


def test_quality_is_clamped(hot, torch_cuda):
    for q, same in ((0, 1), (-7, 1), (101, 100), (1000, 100)):
        table, blob = _encode(torch_cuda, hot, J.content(40, 22, 1), 40, 22, q)
        _check(table, blob, [J.model_file(40, 22, 1, same)], blob.size)


@pytest.mark.parametrize("n", [1, 5, 300])
def test_batches(hot, torch_cuda, n):
    """pictures of differing content (and so of differing lengths) in one launch: offsets, density, sentinels"""
    w, h = 40, 22
    yuv = np.stack([J.content(w, h, 100 + k) for k in range(n)])
    files = [J.model_file(w, h, 100 + k, 75) for k in range(n)]
    assert n == 1 or len({len(f) for f in files}) > 1
    table, blob = _encode(torch_cuda, hot, yuv, w, h, 75)
    _check(table, blob, files, blob.size)


def test_capacity(hot, torch_cuda):
    """the third of five pictures does not fit: it is flagged, the other four are exact, no byte from the capacity on changes"""
    w, h = 48, 32
    rng = np.random.default_rng(9)
    yuv = np.stack([np.full(w * h * 3 // 2, 30 + 40 * k, dtype=np.uint8) for k in range(5)])      # flat pictures with a few
    for k in range(5):                                                                            # tiles of content: short files
        yuv[k].reshape(-1, w)[:8] = J.content(w, 8, 200 + k)[:w * 8].reshape(8, w)
    yuv[2] = rng.integers(0, 256, yuv.shape[1], dtype=np.uint8)      # dense noise: the longest file by far
    files = [J.encode(yuv[k], w, h, 100) for k in range(5)]
    al = [(len(f) + 15) & ~15 for f in files]
    cap = al[0] + al[1] + al[3] + len(files[4])                       # exactly what the other four need
    assert len(files[2]) > al[3] + len(files[4])
    table, blob = _encode(torch_cuda, hot, yuv, w, h, 100, cap=cap, room=cap + 3 * len(files[2]))
    assert [int(e["status"]) for e in table] == [JPEG_OK, JPEG_OK, JPEG_TOO_BIG, JPEG_OK, JPEG_OK]
    _check(table, blob, files, cap)
    table, blob = _encode(torch_cuda, hot, yuv, w, h, 100, cap=cap - 1, room=cap + 3 * len(files[2]))   # one byte less: the last one too
    assert [int(e["status"]) for e in table] == [JPEG_OK, JPEG_OK, JPEG_TOO_BIG, JPEG_OK, JPEG_TOO_BIG]
    _check(table, blob, files, cap - 1)
    table, blob = _encode(torch_cuda, hot, yuv, w, h, 100, cap=0, room=64)                              # nothing fits
    assert all(int(e["status"]) == JPEG_TOO_BIG and int(e["length"]) == 0 for e in table)
    _check(table, blob, files, 0)


def test_malformed_arguments_are_refused(hot, torch_cuda):
    dev = torch_cuda.device("cuda", 0)
    d = torch_cuda.full((1 << 16,), 7, dtype=torch_cuda.uint8, device=dev)
    base = (d.data_ptr() + 15) & ~15
    for g, restart, blob in ((geometry(0, 0, 16, 16, 17, 16), 0, base), (geometry(0, 0, 16, 16, 0, 16), 0, base),
                             (geometry(0, 0, 16, 16), 70000, base), (geometry(0, 0, 16, 16), 0, base + 4),
                             (geometry(0, 0, 16, 16, 32768, 16384), 0, base)):     # 2^29 samples: lengths are 32-bit
        with pytest.raises(MiniVideoError):
            hot.jpeg_encode_dev(g, base + 32768, 1, blob, 4096, base + 16384, restart_mcus=restart)   # refused before any launch
    torch_cuda.cuda.synchronize(dev)
    assert (d.cpu().numpy() == 7).all()


def test_write_stage_checks_a_stale_table(hot, torch_cuda):
    """the write stage on its own (a measurement hook) finds a table that names bytes beyond the capacity: nothing is stored"""
    from minivideo_amd.hotpath import JPEG_STAGE_WRITE
    dev = torch_cuda.device("cuda", 0)
    w, h, n, cap = 48, 32, 3, 8192
    d_src = torch_cuda.from_numpy(np.stack([J.content(w, h, 300 + k) for k in range(n)]).reshape(-1)).to(dev)
    d_blob = torch_cuda.full((GUARD + cap + GUARD,), 0xA5, dtype=torch_cuda.uint8, device=dev)
    d_tab = torch_cuda.zeros(n * 16, dtype=torch_cuda.uint8, device=dev)
    g = geometry(0, 0, w, h)
    hot.jpeg_encode_dev(g, d_src.data_ptr(), n, d_blob.data_ptr() + GUARD, cap, d_tab.data_ptr(), quality=75)
    hot.sync_check(None)
    good = d_blob.cpu().numpy().copy()
    stale = np.zeros(n, dtype=JPEG_ENTRY_DTYPE)
    stale["offset"] = [cap - 16, cap + 16, cap + 2048]      # (a regressed check would still write inside the guard band)
    stale["length"] = [1000, 700, 700]
    d_tab.copy_(torch_cuda.from_numpy(stale.view(np.uint8)))
    hot.jpeg_encode_dev(g, d_src.data_ptr(), n, d_blob.data_ptr() + GUARD, cap, d_tab.data_ptr(), quality=75, stages=JPEG_STAGE_WRITE)
    hot.sync_check(None)
    assert np.array_equal(d_blob.cpu().numpy(), good)


@pytest.mark.parametrize("deblock", [False, True])
@pytest.mark.parametrize("output", [None, "crop", (40, 40)])
def test_planes_from_the_device_chain(hot, torch_cuda, deblock, output):
    """generator streams reconstructed (and deblocked) on the device, passed through mvhp_resample_dev, encoded: the same bytes
    as the model on the reference chain oracle -> deblock_ref -> resample_ref"""
    W, H, F = 9, 7, 3
    dev = torch_cuda.device("cuda", 0)
    if deblock:
        stream, packed, _ = gen.make_stream_ex(W, H, F, seed=23, profile="high", deblock=dict(idc=(0, 1, 2), offsets=(-6, 6)))
        s = DStream(stream, STREAM_DEBLOCK)
    else:
        stream, packed = gen.make_stream_crop(W, H, F, [(0, 0, 0, 4), (1, 3, 2, 1), (5, 2, 7, 3)], seed=17, profile="high",
                                              sps_pps_every_frame=True)
        s = Stream(stream)
    with s:
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
        for k in range(F):
            g = output_geometry(s.h, k, output)
            want = resample_ref.resample(ref[k], W, H, (g.crop_x, g.crop_y, g.crop_w, g.crop_h, g.out_w, g.out_h)).reshape(-1)
            d_out = torch_cuda.zeros(g.yuv_bytes, dtype=torch_cuda.uint8, device=dev)
            d_blob = torch_cuda.zeros(g.yuv_bytes + 1024, dtype=torch_cuda.uint8, device=dev)
            d_tab = torch_cuda.zeros(16, dtype=torch_cuda.uint8, device=dev)
            hot.resample_dev(p, g, d_yuv.data_ptr() + k * p.yuv_bytes, 1, d_out.data_ptr(), None)
            hot.jpeg_encode_dev(g, d_out.data_ptr(), 1, d_blob.data_ptr(), d_blob.numel(), d_tab.data_ptr(), quality=75)
            hot.sync_check(None)
            e = d_tab.cpu().numpy().view(JPEG_ENTRY_DTYPE)[0]
            f = J.encode(want, g.out_w, g.out_h, 75)
            assert (int(e["offset"]), int(e["length"]), int(e["status"])) == (0, len(f), JPEG_OK), k
            assert d_blob.cpu().numpy()[:len(f)].tobytes() == f, k
