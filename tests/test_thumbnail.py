"""CPU: the output geometry (SPS crop, thumbnail size rule, area-average filter; DESIGN.md 3 "Output geometry").  The NumPy
restatement (tests/resample_ref.py) against plain loops and hand-checked answers, the tap header the kernel uses
(resample_taps.h) host-compiled against it, and mvhp_stream_crop / mvhp_output_geometry / mvhp_geometry_fit on generated
streams, Annex B and MP4."""
import ctypes as C
import os
import shutil
import subprocess

import numpy as np
import pytest

from minivideo_amd import gen
from minivideo_amd.hotpath import geometry_fit, lib, output_geometry, stream_crop
from tests import refdec
from tests import resample_ref as R
from tests.util import Stream

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


# ---- the size rule ----
FIT_KAT = [
    ((1920, 1080, 320, 320), (320, 180)),
    ((1920, 1088, 320, 320), (320, 182)),      # no crop: the coded 1088 rows
    ((1080, 1920, 320, 320), (180, 320)),      # portrait
    ((16, 16, 320, 320), (16, 16)),            # never enlarged
    ((1920, 1080, 4000, 3000), (1920, 1080)),  # box larger than the picture
    ((1920, 1080, 321, 999), (320, 180)),      # odd box sides are rounded down to even
    ((1920, 1080, 999, 181), (320, 180)),
    ((1280, 720, 322, 322), (322, 182)),       # 322 wide: odd chroma width (161)
    ((16, 2000, 100, 100), (2, 100)),          # a side never drops below 2
    ((2, 1000, 999, 998), (2, 998)),
]


@pytest.mark.parametrize("args,want", FIT_KAT)
def test_size_rule_known_answers(args, want):
    assert R.fit(*args) == want
    assert geometry_fit(*args) == want


def test_size_rule_refuses_malformed():
    for args in ((1920, 1080, 0, 0), (1920, 1080, 1, 1), (1920, 1080, 320, 1), (1921, 1080, 320, 320), (0, 0, 320, 320)):
        assert geometry_fit(*args) is None, args


def test_size_rule_random():
    rng = np.random.default_rng(3)
    for _ in range(3000):
        cw, ch = 2 * int(rng.integers(1, 2000)), 2 * int(rng.integers(1, 2000))
        bw, bh = int(rng.integers(2, 3000)), int(rng.integers(2, 3000))
        ow, oh = geometry_fit(cw, ch, bw, bh)
        assert (ow, oh) == R.fit(cw, ch, bw, bh)
        assert ow % 2 == 0 and oh % 2 == 0 and 2 <= ow <= cw and 2 <= oh <= ch and ow <= max(bw & ~1, 2) and oh <= max(bh & ~1, 2)


# ---- the weights ----
@pytest.mark.parametrize("S,D,first", [(2, 1, [8192, 8192]), (3, 1, [5461, 5462, 5461]), (7, 7, [16384]), (1920, 320, None),
                                       (1088, 2, None), (960, 160, None), (161, 80, None), (135, 134, None)])
def test_weights(S, D, first):
    W = R.taps(S, D)
    assert (W >= 0).all() and (W.sum(1) == 1 << 14).all()
    if first is not None:
        assert [int(v) for v in W[0] if v] == first
    for j in range(0, D, max(1, D // 7)):
        assert [R.weight_loop(S, D, j, i) for i in range(S)] == list(W[j])


_HARNESS = r"""
#include "resample_taps.h"
extern "C" int weight(int S, int D, int j, int i) { return mvrs::weight(S, D, j, i); }
extern "C" void span(int S, int D, int j, int *i0, int *n) { mvrs::span(S, D, j, *i0, *n); }
extern "C" int fit(unsigned cw, unsigned ch, unsigned bw, unsigned bh, unsigned *ow, unsigned *oh)
{ uint32_t w = 0, h = 0; int r = mvrs::fit(cw, ch, bw, bh, w, h); *ow = w; *oh = h; return r; }
"""


@pytest.fixture(scope="module")
def taps_lib(tmp_path_factory):
    cxx = shutil.which("g++") or shutil.which("c++")
    if cxx is None:
        pytest.fail("no host C++ compiler")
    d = tmp_path_factory.mktemp("taps")
    src, so = d / "h.cpp", d / "libtaps.so"
    src.write_text(_HARNESS)
    subprocess.run([cxx, "-O2", "-shared", "-fPIC", "-I" + os.path.join(ROOT, "minivideo_amd", "csrc", "hip"), str(src), "-o",
                    str(so)], check=True)
    L = C.CDLL(str(so))
    L.span.argtypes = [C.c_int, C.c_int, C.c_int, C.POINTER(C.c_int), C.POINTER(C.c_int)]
    return L


@pytest.mark.parametrize("S,D", [(2, 1), (3, 1), (1920, 320), (1088, 2), (960, 160), (1080, 180), (540, 90), (161, 80),
                                 (16, 2), (8, 1), (135, 134), (16384, 16382), (1920, 1920)])
def test_tap_header_matches_numpy(taps_lib, S, D):
    W = R.taps(S, D)
    i0, n = C.c_int(), C.c_int()
    for j in sorted(set(list(range(min(D, 40))) + [D - 1, D // 2])):
        taps_lib.span(S, D, j, C.byref(i0), C.byref(n))
        nz = np.nonzero(W[j])[0]
        assert i0.value <= nz[0] and nz[-1] < i0.value + n.value <= S            # every non-zero tap inside the span
        assert [taps_lib.weight(S, D, j, i) for i in range(i0.value, i0.value + n.value)] == list(W[j, i0.value:i0.value + n.value])


def test_tap_header_size_rule(taps_lib):
    ow, oh = C.c_uint(), C.c_uint()
    for args, want in FIT_KAT:
        assert taps_lib.fit(*args, C.byref(ow), C.byref(oh)) == 1 and (ow.value, oh.value) == want


# ---- hand-checked outputs ----
def test_two_to_one_is_rounded_mean_of_2x2():
    rng = np.random.default_rng(1)
    p = rng.integers(0, 256, (12, 20)).astype(np.uint8)
    p[:4, :] = 255
    p[4:6, :] = 0
    got = R.resample_plane(p, 0, 0, 20, 12, 10, 6)
    s = p.astype(int).reshape(6, 2, 10, 2).sum((1, 3))
    assert np.array_equal(got, ((s + 2) >> 2).astype(np.uint8))
    assert (got[:2] == 255).all() and (got[2] == 0).all()


def test_identity_is_a_copy():
    rng = np.random.default_rng(2)
    p = rng.integers(0, 256, (33, 48)).astype(np.uint8)
    assert np.array_equal(R.resample_plane(p, 6, 3, 30, 20, 30, 20), p[3:23, 6:36])


def test_three_to_one_hand():
    p = np.array([[10, 20, 31], [10, 20, 31], [10, 20, 31]], np.uint8)
    # vertical: 5461 + 5462 + 5461 = 2^14 on equal rows -> t = v * 256; horizontal: (5461*2560 + 5462*5120 + 5461*7936 + 2^21) >> 22
    want = (5461 * 2560 + 5462 * 5120 + 5461 * 7936 + (1 << 21)) >> 22
    assert R.resample_plane(p, 0, 0, 3, 3, 1, 1)[0, 0] == want == 20


@pytest.mark.parametrize("shape", [(6, 5, 3, 2), (7, 9, 2, 4), (8, 8, 8, 8), (11, 4, 1, 3), (5, 13, 5, 1)])
def test_numpy_form_matches_loops(shape):
    sh, sw, dh, dw = shape
    rng = np.random.default_rng(sum(shape))
    p = rng.integers(0, 256, (sh + 3, sw + 2)).astype(np.uint8)
    p[0] = 255
    assert np.array_equal(R.resample_plane(p, 1, 2, sw, sh, dw, dh), R.resample_plane_loop(p, 1, 2, sw, sh, dw, dh))


def test_extremes_stay_in_range():
    for v in (0, 255):
        p = np.full((40, 60), v, np.uint8)
        assert (R.resample_plane(p, 0, 0, 60, 40, 14, 6) == v).all()


# ---- the crop of generated streams ----
CROPS = [(0, 0, 0, 4), (1, 3, 2, 1), (0, 0, 0, 0), (7, 0, 0, 7)]


def _crop_of(s, idr):
    g = stream_crop(s.h, idr)
    return None if g is None else (g.crop_x, g.crop_y, g.crop_w, g.crop_h, g.out_w, g.out_h)


@pytest.mark.parametrize("profile", ["baseline", "high"])
def test_stream_crop_annexb(profile):
    W, H = 8, 6
    stream, _ = gen.make_stream_crop(W, H, 4, CROPS, seed=5, profile=profile, sps_pps_every_frame=True)
    with Stream(stream) as s:
        assert s.ok and s.idr_count == 4
        for k, (l, r, t, b) in enumerate(CROPS):
            cw, ch = 16 * W - 2 * (l + r), 16 * H - 2 * (t + b)
            assert _crop_of(s, k) == (2 * l, 2 * t, cw, ch, cw, ch)
            g = output_geometry(s.h, k, (20, 20))
            assert (g.out_w, g.out_h) == R.fit(cw, ch, 20, 20)
            g = output_geometry(s.h, k, None)
            assert (g.crop_x, g.crop_y, g.out_w, g.out_h) == (0, 0, 16 * W, 16 * H)


def test_stream_crop_mp4():
    from tests.mp4mux import mux
    W, H = 5, 4
    stream, _ = gen.make_stream_crop(W, H, 3, [(2, 1, 0, 3)], seed=9, profile="main")
    data = np.frombuffer(mux(stream, W * 16, H * 16), np.uint8)
    L = lib()
    h = C.c_void_p()
    L.mvhp_stream_open_mp4.restype = C.c_int
    L.mvhp_stream_open_mp4.argtypes = [C.c_void_p, C.c_size_t, C.POINTER(C.c_void_p)]
    assert L.mvhp_stream_open_mp4(data.ctypes.data, data.size, C.byref(h)) == 1
    try:
        for k in range(3):
            g = stream_crop(h, k)
            assert (g.crop_x, g.crop_y, g.crop_w, g.crop_h) == (4, 0, 80 - 6, 64 - 6)
    finally:
        L.mvhp_stream_close(h)


def test_stream_without_cropping_is_the_coded_size():
    stream, _ = gen.make_stream(3, 2, 1, seed=1)
    with Stream(stream) as s:
        assert _crop_of(s, 0) == (0, 0, 48, 32, 48, 32)


def test_invalid_crop_refused_but_default_mode_still_decodes():
    """a crop that leaves nothing: the geometry is refused with a message, the records still decode (the default mode
    ignores the crop, as the reference does)"""
    W, H = 4, 3
    stream, packed = gen.make_stream_crop(W, H, 2, [(16, 16, 0, 0), (0, 0, 30, 0)], seed=4, sps_pps_every_frame=True)
    with Stream(stream) as s:
        assert s.ok
        for k in range(2):
            assert _crop_of(s, k) is None and "leaves no picture" in s.error()
            assert output_geometry(s.h, k, "crop") is None
            assert output_geometry(s.h, k, None) is not None
            rc, rec = s.packed(k)
            assert rc == 1 and np.array_equal(rec.reshape(-1, 800), packed[k])


def test_cropped_generator_streams_have_the_plain_macroblocks():
    a, pa = gen.make_stream(6, 5, 3, seed=11, profile="high")
    b, pb = gen.make_stream_crop(6, 5, 3, [(1, 2, 3, 4)], seed=11, profile="high")
    assert np.array_equal(pa, pb) and not np.array_equal(a[:64], b[:64])


@pytest.mark.parametrize("fmt", ["yuv420", "bmp"])
def test_default_mode_ignores_the_crop_like_the_reference(fmt):
    """with neither variable set, a crop in the SPS changes nothing: the reference decoder's files for a cropped stream are the
    coded-size pictures the oracle reconstructs"""
    refdec.require()
    from oracle import loader
    W, H, F = 7, 5, 3
    stream, packed = gen.make_stream_crop(W, H, F, [(1, 2, 3, 1)], seed=21, profile="baseline")
    with Stream(stream) as s:
        p = s.params(0)
    files = refdec.pictures(stream, fmt, F)
    for k in range(F):
        yuv, rgb = loader.recon(p, packed[k], 1, want_rgb=True)
        if fmt == "yuv420":
            assert files[k] == yuv.tobytes()
        else:
            px, w, h = refdec.read_bmp(files[k])
            assert (w, h) == (16 * W, 16 * H) and np.array_equal(px, rgb)


@pytest.mark.parametrize("mode", ["crop_copy", "resample", "resample_1to1"])
def test_tiled_reference_of_the_split_launch_tests(mode):
    """tests/test_gpu_launch_splits.py computes the reference on 263 base pictures and tiles it: the same bytes as the direct
    reference on the first 300 pictures"""
    from tests import test_gpu_launch_splits as X
    g = X.MODES[mode][0]
    ow, oh = g[4:] if len(g) == 6 else g[2:4]
    base, want, want_rgb = X.resample_case(mode)
    yuv = X.tiled(base, 300, X.RESAMPLE_CYCLE)
    assert np.array_equal(yuv[X.RESAMPLE_CYCLE:], base[:300 - X.RESAMPLE_CYCLE]) and len({p.tobytes() for p in base}) == X.RESAMPLE_CYCLE
    direct = R.resample(yuv, 1, 1, g[:4] + (ow, oh))
    assert np.array_equal(direct, X.tiled(want, 300, X.RESAMPLE_CYCLE))
    assert np.array_equal(R.to_rgb(direct, ow, oh), X.tiled(want_rgb, 300, X.RESAMPLE_CYCLE))
    assert len({p.tobytes() for p in want}) == X.RESAMPLE_CYCLE        # a repeated or misplaced picture changes bytes
