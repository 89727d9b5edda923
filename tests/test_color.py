"""CPU: the display rules (DESIGN.md 3 "Display aspect and colour").  The colour coefficients of the library against exact
rationals and the issue's table; the integer equation against float64 and PIL over all 2^24 triples; mvhp_stream_display on
generated streams (every aspect_ratio_idc, extended and reserved ones, ranges, matrices, chroma locations, skipped tails, an SPS
cut off inside its VUI); the aspect rule of resample_taps.h host-compiled against tests/color_ref.py; mvhp_color_resolve, every
branch."""
import ctypes as C
import os
import shutil
import subprocess

import numpy as np
import pytest

from minivideo_amd import gen
from minivideo_amd.hotpath import (COLOR_MODES, DisplayInfo, color_coefficients, color_resolve, geometry_aspect, lib, output_geometry,
                                   stream_display)
from tests import color_ref as K
from tests import resample_ref as R
from tests.util import Stream

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

TABLE = {(K.BT601, 0): (19077, 26149, 33050, 6419, 13320, 16), (K.BT601, 1): (16384, 22970, 29032, 5638, 11700, 0),
         (K.BT709, 0): (19077, 29372, 34610, 3494, 8731, 16), (K.BT709, 1): (16384, 25802, 30402, 3069, 7670, 0)}
SETTINGS = sorted(TABLE)


# ---- coefficients and the equation ----
@pytest.mark.parametrize("matrix,full", SETTINGS)
def test_coefficients(matrix, full):
    assert K.coefficients(matrix, full) == TABLE[(matrix, full)]
    assert color_coefficients(matrix, full) == TABLE[(matrix, full)]


def test_coefficients_refuse_unknown_values():
    for matrix, full in ((2, 0), (-1, 0), (0, 2), (0, -1)):
        assert color_coefficients(matrix, full) is None


@pytest.fixture(scope="module")
def cube():
    """every (Y, Cb, Cr): three int64 arrays of 2^24"""
    v = np.arange(256, dtype=np.int64)
    return np.repeat(v, 65536), np.tile(np.repeat(v, 256), 256), np.tile(v, 65536)


@pytest.mark.parametrize("matrix,full", SETTINGS)
def test_equation_against_float64(cube, matrix, full):
    """NEAREST (c16 = 16 C): within 1 of the rounded, clamped float64 equations for every triple -- and within 0.51 unrounded"""
    Y, Cb, Cr = cube
    got = K.equation(Y, 16 * Cb, 16 * Cr, matrix, full)
    want = K.float_rgb(Y, Cb, Cr, matrix, full)
    for g, w in zip(got, want):
        clamped = np.clip(w, 0.0, 255.0)
        assert np.abs(g.astype(np.int64) - np.rint(clamped).astype(np.int64)).max() <= 1
        assert np.abs(g.astype(np.float64) - clamped).max() <= 0.51


def test_bt601_full_against_pil(cube):
    Image = pytest.importorskip("PIL.Image")
    Y, Cb, Cr = cube
    ycc = np.stack([Y, Cb, Cr], -1).astype(np.uint8).reshape(4096, 4096, 3)
    pil = np.asarray(Image.fromarray(ycc, "YCbCr").convert("RGB")).reshape(-1, 3).astype(np.int64)
    got = np.stack(K.equation(Y, 16 * Cb, 16 * Cr, K.BT601, 1), -1).astype(np.int64)
    assert np.abs(got - pil).max() <= 1


@pytest.mark.parametrize("siting", [K.NEAREST, K.LEFT, K.CENTER])
def test_chroma_blend_against_the_loop(siting):
    rng = np.random.default_rng(siting)
    for ch, cw in ((1, 1), (1, 3), (2, 1), (3, 5)):
        Cp = rng.integers(0, 256, (1, ch, cw), dtype=np.uint8)
        got = K.chroma16(Cp, siting)[0]
        for y in range(2 * ch):
            for x in range(2 * cw):
                assert got[y, x] == K.chroma16_loop(Cp[0], siting, x, y), (ch, cw, x, y)
    flat = np.full((1, 3, 4), 77, np.uint8)
    assert (K.chroma16(flat, siting) == 16 * 77).all()      # the weights sum to 16


# ---- mvhp_stream_display ----
W, H, F = 2, 2, 1


def _display(vui, keep_bits=-1, n=1, **kw):
    stream, packed = gen.make_stream_vui(W, H, n, vui if isinstance(vui, list) else [vui], keep_bits=keep_bits, seed=3,
                                         sps_pps_every_frame=True, **kw)
    with Stream(stream) as s:
        assert s.ok and s.idr_count == n
        return [stream_display(s.h, k).as_dict() for k in range(n)]


UNSPEC = {"sar_w": 0, "sar_h": 0, "vui_present": 1, "signal_present": 0, "full_range": 0, "matrix_coefficients": 2, "chroma_loc": 0}


def test_no_vui():
    stream, _ = gen.make_stream(W, H, 1, seed=3)
    with Stream(stream) as s:
        assert stream_display(s.h, 0).as_dict() == dict(UNSPEC, vui_present=0)
        assert stream_display(s.h, 1) is None and stream_display(s.h, -1) is None


@pytest.mark.parametrize("idc", list(range(0, 17)) + [17, 100, 254])
def test_aspect_ratio_idc(idc):
    d = _display(gen.vui_record(sar=idc))[0]
    assert (d["sar_w"], d["sar_h"]) == K.sar(idc) and d["vui_present"] == 1
    if 1 <= idc <= 16:
        assert d["sar_w"] > 0
    else:
        assert (d["sar_w"], d["sar_h"]) == (0, 0)


@pytest.mark.parametrize("ext,want", [((4, 3), (4, 3)), ((65535, 1), (65535, 1)), ((1, 65535), (1, 65535)), ((1920, 1080), (16, 9)),
                                      ((8, 6), (4, 3)), ((0, 5), (0, 0)), ((5, 0), (0, 0)), ((0, 0), (0, 0)), ((77, 77), (1, 1))])
def test_extended_sar(ext, want):
    d = _display(gen.vui_record(sar=ext))[0]
    assert (d["sar_w"], d["sar_h"]) == want == K.sar(255, ext)


@pytest.mark.parametrize("overscan,timing", [(None, False), (0, False), (1, True), (None, True)])
def test_signal_type_and_chroma_location(overscan, timing):
    """full range, the matrix and every chroma location, with and without the tails that are skipped"""
    vuis, want = [], []
    for full in (0, 1):
        for matrix in (None, 0, 1, 2, 5, 6, 9):
            for loc in (None, 0, 1, 2, 3, 4, 5, (1, 4)):
                vuis.append(gen.vui_record(sar=3, overscan=overscan, full_range=full, matrix=matrix, chroma_loc=loc, timing=timing))
                top = 0 if loc is None else loc[0] if isinstance(loc, tuple) else loc
                want.append(dict(sar_w=10, sar_h=11, vui_present=1, signal_present=1, full_range=full,
                                 matrix_coefficients=2 if matrix is None else matrix, chroma_loc=top))
    assert _display(vuis, n=len(vuis)) == want


def test_absent_signal_type():
    assert _display(gen.vui_record(chroma_loc=3, timing=True))[0] == dict(UNSPEC, chroma_loc=3)
    assert _display(gen.vui_record())[0] == UNSPEC
    # a matrix alone writes the signal type with video_full_range_flag 0
    assert _display(gen.vui_record(matrix=1))[0] == dict(UNSPEC, signal_present=1, matrix_coefficients=1)


@pytest.mark.parametrize("loc", [6, 7, 100, (6, 0)])
def test_chroma_location_out_of_range_is_unspecified(loc):
    assert _display(gen.vui_record(sar=14, full_range=1, matrix=1, chroma_loc=loc))[0] == UNSPEC
    # (the bottom field's type is not read for frames)
    assert _display(gen.vui_record(sar=14, chroma_loc=(2, 9)))[0] == dict(UNSPEC, sar_w=4, sar_h=3, chroma_loc=2)


@pytest.mark.parametrize("profile", ["baseline", "high"])
@pytest.mark.parametrize("keep_bits", [0, 1, 5, 9, 12, 25, 40, 41, 44, 50, 79, 80])
def test_sps_truncated_inside_the_vui(profile, keep_bits):
    """the stream opens, the display information is unspecified (also where the cut left the fields whole: the flags behind
    them are missing), and the pictures -- parameters and packed records -- are those of the stream without VUI, byte for byte"""
    rec = gen.vui_record(sar=(4, 3), overscan=1, full_range=1, matrix=1, chroma_loc=1, timing=True)
    kw = dict(seed=8, profile=profile, sps_pps_every_frame=True)
    stream, packed = gen.make_stream_vui(3, 2, 2, [rec], keep_bits=keep_bits, **kw)
    plain, packed0 = gen.make_stream(3, 2, 2, **kw)
    whole, _ = gen.make_stream_vui(3, 2, 2, [rec], **kw)
    assert np.array_equal(packed, packed0) and len(plain) <= len(stream) < len(whole)
    with Stream(stream) as s, Stream(plain) as s0:
        assert s.ok and s.idr_count == s0.idr_count == 2
        for k in range(2):
            assert bytes(s.params(k)) == bytes(s0.params(k))
            rc, got = s.packed(k)
            rc0, got0 = s0.packed(k)
            assert rc == rc0 == 1 and np.array_equal(got, got0) and np.array_equal(got.reshape(-1), packed0[k].reshape(-1))
            assert stream_display(s.h, k).as_dict() == UNSPEC
            g, g0 = output_geometry(s.h, k, "crop", aspect=True), output_geometry(s0.h, k, "crop")
            assert (g.out_w, g.out_h, g.crop_w, g.crop_h) == (g0.out_w, g0.out_h, g0.crop_w, g0.crop_h)


def test_whole_vui_changes_no_picture():
    rec = gen.vui_record(sar=(4, 3), overscan=1, full_range=1, matrix=1, chroma_loc=1, timing=True)
    kw = dict(seed=8, profile="main", sps_pps_every_frame=True)
    stream, packed = gen.make_stream_vui(3, 2, 2, [rec], **kw)
    plain, packed0 = gen.make_stream(3, 2, 2, **kw)
    assert np.array_equal(packed, packed0)
    with Stream(stream) as s, Stream(plain) as s0:
        for k in range(2):
            assert bytes(s.params(k)) == bytes(s0.params(k)) and np.array_equal(s.packed(k)[1], s0.packed(k)[1])
        assert stream_display(s.h, 0).as_dict() == dict(sar_w=4, sar_h=3, vui_present=1, signal_present=1, full_range=1,
                                                        matrix_coefficients=1, chroma_loc=1)


# ---- the aspect rule ----
ASPECT_KAT = [((1440, 1080, 4, 3), (1440, 810)), ((720, 576, 12, 11), (720, 528)), ((720, 480, 10, 11), (654, 480)),
              ((1920, 1080, 1, 1), (1920, 1080)), ((1920, 1080, 0, 0), (1920, 1080)), ((1920, 1080, 0, 7), (1920, 1080)),
              ((2, 2, 65535, 1), (2, 2)), ((2, 2, 1, 65535), (2, 2)), ((4096, 4096, 65535, 1), (4096, 2)), ((4096, 4096, 1, 65535), (2, 4096))]

_HARNESS = r"""
#include "resample_taps.h"
extern "C" int aspect(unsigned cw, unsigned ch, unsigned a, unsigned b, unsigned *ow, unsigned *oh)
{ uint32_t w = 0, h = 0; int r = mvrs::aspect(cw, ch, a, b, w, h); *ow = w; *oh = h; return r; }
"""


@pytest.fixture(scope="module")
def taps_lib(tmp_path_factory):
    cxx = shutil.which("g++") or shutil.which("c++")
    if cxx is None:
        pytest.fail("no host C++ compiler")
    d = tmp_path_factory.mktemp("aspect")
    src, so = d / "h.cpp", d / "libaspect.so"
    src.write_text(_HARNESS)
    subprocess.run([cxx, "-O2", "-shared", "-fPIC", "-I" + os.path.join(ROOT, "minivideo_amd", "csrc", "hip"), str(src), "-o",
                    str(so)], check=True)
    return C.CDLL(str(so))


def _header_aspect(L, *args):
    ow, oh = C.c_uint(), C.c_uint()
    assert L.aspect(*args, C.byref(ow), C.byref(oh)) == 1
    return ow.value, oh.value


@pytest.mark.parametrize("args,want", ASPECT_KAT)
def test_aspect_known_answers(taps_lib, args, want):
    assert K.aspect(*args) == want
    assert _header_aspect(taps_lib, *args) == want
    assert geometry_aspect(*args) == want


def test_aspect_refuses_malformed():
    for args in ((1441, 1080, 4, 3), (1440, 1081, 4, 3), (0, 1080, 4, 3), (1440, 0, 4, 3)):
        assert geometry_aspect(*args) is None, args


def test_aspect_sweep(taps_lib):
    rng = np.random.default_rng(11)
    sars = [K.SAR_TABLE[k] for k in sorted(K.SAR_TABLE)] + [(65535, 1), (1, 65535), (65535, 65534), (65534, 65535), (3, 65535)]
    for _ in range(4000):
        cw, ch = 2 * int(rng.integers(1, 2049)), 2 * int(rng.integers(1, 2049))
        a, b = sars[int(rng.integers(0, len(sars)))] if rng.integers(0, 2) else (int(rng.integers(1, 65536)), int(rng.integers(1, 65536)))
        want = K.aspect(cw, ch, a, b)
        assert _header_aspect(taps_lib, cw, ch, a, b) == want == geometry_aspect(cw, ch, a, b)
        ow, oh = want
        assert ow % 2 == 0 and oh % 2 == 0 and 2 <= ow <= cw and 2 <= oh <= ch and (ow == cw or oh == ch)      # one axis only, never enlarged


CROPS = [(0, 0, 0, 0), (1, 3, 2, 1), (0, 2, 0, 5)]


@pytest.mark.parametrize("sar", [14, 2, 3, (65535, 1), (1, 65535), None, 1])
def test_output_geometry_with_aspect(sar):
    """mvhp_output_geometry: the rule on the crop, then the box, then the turn's exchange of sides; crop_* never change"""
    Wm, Hm = 9, 7
    stream, _ = gen.make_stream_vui(Wm, Hm, len(CROPS), [gen.vui_record(sar=sar)], crops=CROPS, seed=2, sps_pps_every_frame=True)
    a, b = (0, 0) if sar is None else K.sar(255, sar) if isinstance(sar, tuple) else K.sar(sar)
    with Stream(stream) as s:
        for k, (l, r, t, bo) in enumerate(CROPS):
            cw, ch = 16 * Wm - 2 * (l + r), 16 * Hm - 2 * (t + bo)
            dw, dh = K.aspect(cw, ch, a, b)
            for output in (None, "crop", (40, 24), (24, 40), (3, 500), (500, 500)):
                for rotate in (None, 90, 180, 270):
                    g = output_geometry(s.h, k, output, rotate=rotate, aspect=True)
                    odd = rotate in (90, 270)
                    if isinstance(output, tuple):
                        bw, bh = (output[1], output[0]) if odd else output
                        ow, oh = R.fit(dw, dh, bw, bh)
                    else:
                        ow, oh = dw, dh
                    want = (2 * l, 2 * t, cw, ch) + ((oh, ow) if odd else (ow, oh))
                    assert (g.crop_x, g.crop_y, g.crop_w, g.crop_h, g.out_w, g.out_h) == want, (k, output, rotate)
                    # without the flag: today's geometry
                    g0 = output_geometry(s.h, k, output, rotate=rotate)
                    if a == b:
                        assert (g0.out_w, g0.out_h) == (g.out_w, g.out_h) or output is None


# ---- mvhp_color_resolve ----
def _info(**kw):
    d = DisplayInfo()
    for k, v in dict(UNSPEC, **kw).items():
        setattr(d, k, v)
    return d


def test_color_resolve_every_branch():
    sizes = [(1279, 576), (1280, 576), (1279, 577), (1280, 577), (16, 16), (1920, 1088), (720, 576), (704, 578)]
    for mode in range(5):
        for mc in (0, 1, 2, 4, 5, 6, 7, 9, 255):
            for signal in (0, 1):
                for full in (0, 1):
                    for loc in range(6):
                        for cw, ch in sizes:
                            d = _info(signal_present=signal, full_range=full, matrix_coefficients=mc, chroma_loc=loc)
                            want = K.resolve(d.as_dict(), cw, ch, mode)
                            assert color_resolve(d, cw, ch, mode).as_tuple() == want == color_resolve(d, cw, ch, COLOR_MODES[mode]).as_tuple()
    # the thresholds, spelled out: width 1280 or more, height above 576
    d = _info()
    assert [color_resolve(d, w, h).matrix for w, h in sizes[:4]] == [K.BT601, K.BT709, K.BT709, K.BT709]
    # full range only with the signal type present; forced modes ignore the stream but keep its siting
    assert color_resolve(_info(full_range=1), 16, 16).full_range == 0 and color_resolve(_info(full_range=1, signal_present=1), 16, 16).full_range == 1
    assert color_resolve(_info(matrix_coefficients=1, chroma_loc=1), 16, 16, "bt601-full").as_tuple() == (K.BT601, 1, K.CENTER)
    assert color_resolve(_info(matrix_coefficients=6, chroma_loc=2), 1920, 1088, "bt709").as_tuple() == (K.BT709, 0, K.LEFT)
    # no display information at all: the size decides, limited range, left siting
    assert color_resolve(None, 1920, 1088).as_tuple() == (K.BT709, 0, K.LEFT) and color_resolve(None, 640, 480).as_tuple() == (K.BT601, 0, K.LEFT)
    assert color_resolve(d, 16, 16, 5) is None and color_resolve(d, 16, 16, -1) is None


def test_exports():
    L = lib()
    for name in ("mvhp_stream_display", "mvhp_geometry_aspect", "mvhp_color_coefficients", "mvhp_color_resolve", "mvhp_color_dev"):
        assert hasattr(L, name), name
