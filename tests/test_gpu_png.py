"""GPU: the PNG encoder (png_encode.hip, mvhp_png_encode_dev) byte for byte against the restatement of the format (tests/png_ref.py):
picture sizes around every change of the segment height, content that reaches every case of the filters and the code
construction, batches, the blob's layout at every 16-byte phase, the capacity rule, the refusals, and RGB that comes from the
reconstruction, geometry and orientation kernels."""
import numpy as np
import pytest

from minivideo_amd import HotPath, gen
from minivideo_amd.hotpath import (PNG_ENTRY_DTYPE, PNG_OK, PNG_STAGE_WRITE, PNG_TOO_BIG, MiniVideoError, geometry,
                                   output_geometry)
from oracle import loader
from tests import orient_ref, png_ref as P, resample_ref
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


def _encode(torch, hot, rgb, w, h, cap=None, room=None):
    """rgb (n, h, w, 3) -> (table, blob bytes [0, room)); the bytes before the blob, from `cap` on, and around the table must keep
    their fill"""
    dev = torch.device("cuda", 0)
    rgb = np.array(rgb, dtype=np.uint8).reshape(-1, w * h * 3)      # (a writable copy: the pictures are shared)
    n = rgb.shape[0]
    room = n * ((P.max_bytes(w, h) + 15) & ~15) if room is None else room
    cap = room if cap is None else cap
    assert cap <= room
    d_src = torch.from_numpy(rgb.reshape(-1)).to(dev)
    d_blob = torch.full((GUARD + room + GUARD,), 0xA5, dtype=torch.uint8, device=dev)
    d_tab = torch.full((GUARD + n * 16 + GUARD,), 0x5A, dtype=torch.uint8, device=dev)
    torch.cuda.synchronize(dev)
    hot.png_encode_dev(geometry(0, 0, w, h), d_src.data_ptr(), n, d_blob.data_ptr() + GUARD, cap, d_tab.data_ptr() + GUARD)
    hot.sync_check(None)
    blob, tab = d_blob.cpu().numpy(), d_tab.cpu().numpy()
    assert (blob[:GUARD] == 0xA5).all() and (blob[GUARD + cap:] == 0xA5).all(), "bytes outside the blob's capacity changed"
    assert (tab[:GUARD] == 0x5A).all() and (tab[GUARD + n * 16:] == 0x5A).all(), "bytes around the table changed"
    return tab[GUARD:GUARD + n * 16].view(PNG_ENTRY_DTYPE), blob[GUARD:GUARD + room]


def _check(table, blob, files, cap):
    """the table is the layout rule applied to the model's lengths, every file that fits is the model's, and no other byte of
    the blob changed"""
    want = P.blob_layout([len(f) for f in files], cap)
    got = np.stack([table["offset"].astype(np.int64), table["length"].astype(np.int64), table["status"].astype(np.int64)], axis=1)
    bad = np.flatnonzero((got != np.array(want, dtype=np.int64).reshape(-1, 3)).any(axis=1))
    assert bad.size == 0, "first differing table entry: %d: %s, expected %s" % (bad[0], got[bad[0]], want[bad[0]])
    expect = np.full(blob.size, 0xA5, dtype=np.uint8)
    for (off, ln, st), f in zip(want, files):
        assert off % 16 == 0
        if st == P.STATUS_OK:
            expect[off:off + ln] = np.frombuffer(f, dtype=np.uint8)
    bad = np.flatnonzero(blob != expect)
    assert bad.size == 0, "first differing byte of the blob: %d" % bad[0]


def _one(torch, hot, w, h, seed, kind="content"):
    table, blob = _encode(torch, hot, P.picture(w, h, seed, kind), w, h)
    _check(table, blob, [P.model_file(w, h, seed, kind)], blob.size)


# R = 32768 // (3 w + 1): 10922 wide gives exactly 1, 10924 a row longer than 32768 (10923 is odd, and refused), 5460 gives 2
@pytest.mark.parametrize("w,h", [(2, 2), (2, 4), (18, 6), (322, 182), (10922, 2), (10922, 4), (10924, 2), (5460, 4), (5460, 6),
                                 (16384, 2), (2, 16384), (21844, 2)])
def test_sizes(hot, torch_cuda, w, h):
    _one(torch_cuda, hot, w, h, 3)


# 606 wide: R = 18; 574 wide: R = 19.  Heights are even, so R and 2 R rows come from the first, R + 1 from the second, and the
# odd 2 R + 1 can only be refused (test_malformed_arguments_are_refused): 2 R + 2 stands in, a last segment of two rows
@pytest.mark.parametrize("w,h", [(606, 18), (606, 20), (606, 36), (606, 38), (574, 20), (574, 38), (574, 40)])
def test_segment_heights(hot, torch_cuda, w, h):
    assert P.segment_rows(w) == (18 if w == 606 else 19)
    _one(torch_cuda, hot, w, h, 5)
    _one(torch_cuda, hot, w, h, 6, "smooth")


@pytest.mark.parametrize("w,h,seed,kind", [(322, 182, 3, "content"), (322, 182, 1, "fib"), (16384, 2, 1, "fib"), (64, 64, 0, "flat"),
                                           (64, 64, 200, "flat"), (64, 64, 1, "noise"), (320, 180, 1, "smooth"),
                                           (16384, 2, 1, "smooth3"), (322, 182, 4, "content"), (322, 182, 2, "mixed")])
def test_content(hot, torch_cuda, w, h, seed, kind):
    """every filter type, ties, stored segments, a single literal, halved counts (tests/test_png.py asserts on the model's trace
    that these pictures reach them)"""
    _one(torch_cuda, hot, w, h, seed, kind)


@pytest.mark.parametrize("n", [1, 5, 300])
def test_batches(hot, torch_cuda, n):
    """pictures of differing content (and so of differing lengths) in one launch: offsets, density, sentinels"""
    w, h = 18, 6
    rgb = np.stack([P.picture(w, h, 100 + k) for k in range(n)])
    files = [P.model_file(w, h, 100 + k) for k in range(n)]
    assert n == 1 or len({len(f) for f in files}) > 1
    table, blob = _encode(torch_cuda, hot, rgb, w, h)
    _check(table, blob, files, blob.size)


def test_more_pictures_than_a_grid_dimension(hot, torch_cuda):
    """65 537 pictures of 2 x 2 that cycle through seven distinct ones: the launches are split at 65 535"""
    n, w, h = 65537, 2, 2
    kinds = [P.picture(w, h, k, "content" if k < 4 else "flat") for k in range(7)]
    one = [P.encode(p, w, h) for p in kinds]
    pick = np.arange(n) % 7
    rgb = np.stack(kinds)[pick]
    table, blob = _encode(torch_cuda, hot, rgb, w, h)
    _check(table, blob, [one[k] for k in pick], blob.size)


def test_blob_offsets_at_every_phase(hot, torch_cuda):
    """file lengths of every residue modulo 16: chunks of the files behind them start at every phase of the aligned stores"""
    w, h = 18, 6
    files, rgb, seen = [], [], set()
    for seed in range(400):
        f = P.model_file(w, h, seed)
        if len(f) % 16 not in seen:
            seen.add(len(f) % 16)
            files.append(f)
            rgb.append(P.picture(w, h, seed))
        if len(seen) == 16:
            break
    assert len(seen) == 16
    table, blob = _encode(torch_cuda, hot, np.stack(rgb), w, h)
    _check(table, blob, files, blob.size)
    # and chunks inside a file at every phase of a dword: several segments of differing lengths
    _one(torch_cuda, hot, 2, 16384, 9)


def test_capacity(hot, torch_cuda):
    """the third of five pictures does not fit: it is flagged, the other four are exact, no byte from the capacity on changes"""
    w, h = 48, 32
    rgb = np.stack([P.picture(w, h, 30 + 40 * k, "flat") for k in range(5)])     # flat pictures under a few rows of content:
    for k in range(5):                                                     # short files
        rgb[k][:4 + k] = P.picture(w, 4 + k, 20 + k, "smooth")
    rgb[2] = P.picture(w, h, 1, "noise")                                   # stored: the longest file by far
    files = [P.encode(rgb[k], w, h) for k in range(5)]
    al = [(len(f) + 15) & ~15 for f in files]
    cap = al[0] + al[1] + al[3] + len(files[4])                            # exactly what the other four need
    assert len(files[2]) > al[3] + len(files[4])
    room = cap + 3 * len(files[2])
    table, blob = _encode(torch_cuda, hot, rgb, w, h, cap=cap, room=room)
    assert [int(e["status"]) for e in table] == [PNG_OK, PNG_OK, PNG_TOO_BIG, PNG_OK, PNG_OK]
    assert int(table[2]["length"]) == 0
    _check(table, blob, files, cap)
    table, blob = _encode(torch_cuda, hot, rgb, w, h, cap=cap - 1, room=room)   # one byte less: the last one too
    assert [int(e["status"]) for e in table] == [PNG_OK, PNG_OK, PNG_TOO_BIG, PNG_OK, PNG_TOO_BIG]
    _check(table, blob, files, cap - 1)
    table, blob = _encode(torch_cuda, hot, rgb, w, h, cap=0, room=64)            # nothing fits
    assert all(int(e["status"]) == PNG_TOO_BIG and int(e["length"]) == 0 for e in table)
    _check(table, blob, files, 0)


def test_malformed_arguments_are_refused(hot, torch_cuda):
    dev = torch_cuda.device("cuda", 0)
    d = torch_cuda.full((1 << 16,), 7, dtype=torch_cuda.uint8, device=dev)
    base = (d.data_ptr() + 15) & ~15
    ok = geometry(0, 0, 16, 16)
    for g, n, blob, tab in ((geometry(0, 0, 16, 16, 17, 16), 1, base, base + 16384),       # odd width
                            (geometry(0, 0, 16, 16, 16, 17), 1, base, base + 16384),       # odd height
                            (geometry(0, 0, 16, 16, 0, 16), 1, base, base + 16384),        # zero sizes
                            (geometry(0, 0, 16, 16, 16, 0), 1, base, base + 16384),
                            (ok, -1, base, base + 16384),                                  # n < 0
                            (ok, 1, base + 4, base + 16384),                               # misaligned blob
                            (ok, 1, base, base + 16384 + 4),                               # misaligned table
                            (geometry(0, 0, 16, 16, 21846, 2), 1, base, base + 16384),     # a row that fits no stored block
                            (geometry(0, 0, 16, 16, 16384, 32768), 1, base, base + 16384)):   # 2^29 samples: lengths are 32-bit
        with pytest.raises(MiniVideoError):
            hot.png_encode_dev(g, base + 32768, n, blob, 4096, tab)        # refused before any launch
    hot.png_encode_dev(ok, base + 32768, 0, base, 4096, base + 16384)      # n = 0: nothing to do
    torch_cuda.cuda.synchronize(dev)
    assert (d.cpu().numpy() == 7).all()


def test_write_stage_checks_a_stale_table(hot, torch_cuda):
    """the write stage on its own (a measurement hook) finds a table that names bytes beyond the capacity, and an offset that is
    no multiple of 16: nothing is stored"""
    dev = torch_cuda.device("cuda", 0)
    w, h, n, cap = 48, 32, 4, 16384
    d_src = torch_cuda.from_numpy(np.stack([P.picture(w, h, 300 + k, "smooth") for k in range(n)]).reshape(-1)).to(dev)
    d_blob = torch_cuda.full((GUARD + cap + GUARD,), 0xA5, dtype=torch_cuda.uint8, device=dev)
    d_tab = torch_cuda.zeros(n * 16, dtype=torch_cuda.uint8, device=dev)
    g = geometry(0, 0, w, h)
    hot.png_encode_dev(g, d_src.data_ptr(), n, d_blob.data_ptr() + GUARD, cap, d_tab.data_ptr())
    hot.sync_check(None)
    good = d_blob.cpu().numpy().copy()
    assert (good[GUARD:GUARD + 8] == np.frombuffer(P.SIGNATURE, dtype=np.uint8)).all()
    stale = np.zeros(n, dtype=PNG_ENTRY_DTYPE)
    stale["offset"] = [cap - 16, cap + 16, cap + 2048, cap // 2 + 3]      # (a regressed check would still write inside the guard band)
    stale["length"] = [3000, 700, 700, 100]
    d_tab.copy_(torch_cuda.from_numpy(stale.view(np.uint8)))
    d_blob.fill_(0xA5)
    hot.png_encode_dev(g, d_src.data_ptr(), n, d_blob.data_ptr() + GUARD, cap, d_tab.data_ptr(), stages=PNG_STAGE_WRITE)
    hot.sync_check(None)
    assert (d_blob.cpu().numpy() == 0xA5).all()


def _coded_rgb(torch, hot, s, packed, F):
    """the fused epilogue's RGB of F coded pictures, and the oracle's planes and RGB"""
    dev = torch.device("cuda", 0)
    p = s.params(0)
    ref_yuv, ref_rgb = loader.recon(p, packed, F, want_rgb=True)
    d_packed = torch.from_numpy(np.ascontiguousarray(packed).reshape(-1)).to(dev)
    d_yuv = torch.zeros(F * p.yuv_bytes, dtype=torch.uint8, device=dev)
    d_rgb = torch.zeros(F * p.rgb_bytes, dtype=torch.uint8, device=dev)
    hot.recon_dev(p, d_packed.data_ptr(), F, d_yuv.data_ptr(), d_rgb.data_ptr())
    return p, d_yuv, d_rgb, np.asarray(ref_yuv).reshape(F, -1), np.asarray(ref_rgb).reshape(F, -1)


def _encode_dev(torch, hot, g, d_rgb_ptr, n):
    dev = torch.device("cuda", 0)
    room = n * ((P.max_bytes(g.out_w, g.out_h) + 15) & ~15)
    d_blob = torch.zeros(room, dtype=torch.uint8, device=dev)
    d_tab = torch.zeros(n * 16, dtype=torch.uint8, device=dev)
    hot.png_encode_dev(g, d_rgb_ptr, n, d_blob.data_ptr(), room, d_tab.data_ptr())
    hot.sync_check(None)
    tab = d_tab.cpu().numpy().view(PNG_ENTRY_DTYPE)
    blob = d_blob.cpu().numpy()
    return [blob[int(e["offset"]):int(e["offset"]) + int(e["length"])].tobytes() for e in tab], tab


def test_rgb_from_the_fused_epilogue(hot, torch_cuda):
    W, H, F = 9, 7, 3
    stream, packed = gen.make_stream_crop(W, H, F, [(0, 0, 0, 4), (1, 3, 2, 1), (5, 2, 7, 3)], seed=17, profile="high",
                                          sps_pps_every_frame=True)
    with Stream(stream) as s:
        assert s.ok
        p, d_yuv, d_rgb, ref_yuv, ref_rgb = _coded_rgb(torch_cuda, hot, s, packed, F)
        files, tab = _encode_dev(torch_cuda, hot, geometry(0, 0, W * 16, H * 16), d_rgb.data_ptr(), F)
        assert all(int(e["status"]) == PNG_OK for e in tab)
        for k in range(F):
            assert files[k] == P.encode(ref_rgb[k], W * 16, H * 16), k


@pytest.mark.parametrize("output", ["crop", (40, 40)])
def test_rgb_from_the_geometry_pass(hot, torch_cuda, output):
    W, H, F = 9, 7, 3
    dev = torch_cuda.device("cuda", 0)
    stream, packed = gen.make_stream_crop(W, H, F, [(0, 0, 0, 4), (1, 3, 2, 1), (5, 2, 7, 3)], seed=17, profile="high",
                                          sps_pps_every_frame=True)
    with Stream(stream) as s:
        assert s.ok
        p, d_yuv, d_rgb, ref_yuv, ref_rgb = _coded_rgb(torch_cuda, hot, s, packed, F)
        for k in range(F):
            g = output_geometry(s.h, k, output)
            rect = (g.crop_x, g.crop_y, g.crop_w, g.crop_h, g.out_w, g.out_h)
            want = resample_ref.to_rgb(resample_ref.resample(ref_yuv[k], W, H, rect), g.out_w, g.out_h)
            d_out = torch_cuda.zeros(g.rgb_bytes, dtype=torch_cuda.uint8, device=dev)
            hot.resample_dev(p, g, d_yuv.data_ptr() + k * p.yuv_bytes, 1, None, d_out.data_ptr())
            files, tab = _encode_dev(torch_cuda, hot, g, d_out.data_ptr(), 1)
            assert files[0] == P.encode(np.asarray(want).reshape(-1), g.out_w, g.out_h), k


@pytest.mark.parametrize("turns", [1, 2])
def test_rgb_from_the_orientation_pass(hot, torch_cuda, turns):
    W, H, F = 9, 7, 2
    dev = torch_cuda.device("cuda", 0)
    stream, packed = gen.make_stream_crop(W, H, F, [(0, 0, 0, 4), (1, 3, 2, 1)], seed=17, profile="high", sps_pps_every_frame=True)
    with Stream(stream) as s:
        assert s.ok
        p, d_yuv, d_rgb, ref_yuv, ref_rgb = _coded_rgb(torch_cuda, hot, s, packed, F)
        for k in range(F):
            g = output_geometry(s.h, k, "crop")
            rect = (g.crop_x, g.crop_y, g.crop_w, g.crop_h, g.out_w, g.out_h)
            planes = orient_ref.turn(resample_ref.resample(ref_yuv[k], W, H, rect), g.out_w, g.out_h, turns)
            ow, oh = (g.out_h, g.out_w) if turns & 1 else (g.out_w, g.out_h)
            want = resample_ref.to_rgb(planes, ow, oh)
            d_out = torch_cuda.zeros(g.rgb_bytes, dtype=torch_cuda.uint8, device=dev)
            hot.orient_dev(p, g, turns, d_yuv.data_ptr() + k * p.yuv_bytes, 1, None, d_out.data_ptr())
            files, tab = _encode_dev(torch_cuda, hot, geometry(0, 0, ow, oh), d_out.data_ptr(), 1)
            assert files[0] == P.encode(np.asarray(want).reshape(-1), ow, oh), k
