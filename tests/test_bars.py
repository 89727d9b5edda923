"""CPU: black bars (DESIGN.md 3 "Black bars").  The NumPy restatement (tests/bars_ref.py) against a plain double loop, the host
rules of the library (mvhp_bars_need, mvhp_bars_union, mvhp_trim_rect) against known answers and against the restatement, and the
output geometry under MVHP_OUTPUT_TRIM (mvhp_stream_set_trim, mvhp_output_geometry) on generator streams.  Exact everywhere."""
import numpy as np
import pytest

from minivideo_amd import gen
from minivideo_amd.hotpath import (OUTPUT_CROP, OUTPUT_TRIM, LumaBars, OutputGeometry, OutputRequest, bars_need, bars_union, geometry,
                                   lib, output_geometry, stream_crop, stream_set_trim, stream_trim, trim_rect)
from tests import bars_ref as B
from tests import color_ref
from tests import resample_ref as R
from tests.util import Stream


def _rect(g):
    return int(g.crop_x), int(g.crop_y), int(g.crop_w), int(g.crop_h)


def _all(g):
    return _rect(g) + (int(g.out_w), int(g.out_h))


# ---- the restatement ----
@pytest.mark.parametrize("seed", [1, 2, 3, 4])
def test_ref_against_a_double_loop(seed):
    rng = np.random.default_rng(seed)
    H, W = 48, 96
    Y = rng.integers(0, 256, (H, W), dtype=np.uint8)
    if seed % 2 == 0:                        # bars, a bright line inside one of them, a dim column
        Y[:10] = 16
        Y[40:] = 3
        Y[44, 7:11] = 200
        Y[:, 20] = 24
    if seed == 3:
        Y[:] = rng.integers(0, 25, (H, W), dtype=np.uint8)      # nothing above the level
    for rect in ((0, 0, W, H), (2, 6, 70, 38), (14, 0, 64, 48), (30, 40, 2, 2)):
        for level in (1, 24, 254):
            assert B.record(Y, rect, level) == B.record_loops(Y, rect, level), (rect, level)


def test_ref_known_pictures():
    Y = np.full((64, 128), 16, dtype=np.uint8)
    Y[10:50, 32:96] = 120
    assert B.record(Y, (0, 0, 128, 64)) == (32, 10, 64, 40, 40, 64)
    assert B.record(Y, (40, 20, 20, 10)) == (40, 20, 20, 10, 10, 20)
    assert B.record(Y, (0, 0, 32, 64)) == (0, 0, 0, 0, 0, 0)
    Y[:] = 16
    Y[5, :3] = 255                           # three bright samples of 128: below need(128) = 4 for the row
    assert B.record(Y, (0, 0, 128, 64)) == (0, 0, 0, 0, 0, 0)
    Y[5, :4] = 255
    assert B.record(Y, (0, 0, 128, 64)) == (0, 0, 0, 0, 1, 0)    # need(64) = 2 per column: one row is not enough
    Y[6, :4] = 255
    assert B.record(Y, (0, 0, 128, 64)) == (0, 5, 4, 2, 2, 4)


# ---- the rules ----
@pytest.mark.parametrize("length,need", [(2, 1), (31, 1), (32, 1), (63, 1), (64, 2), (1920, 60), (16384, 512)])
def test_need(length, need):
    assert bars_need(length) == need
    assert B.need(length) == need


UNIONS = [
    ("no boxes", [], (0, (0, 0, 0, 0))),
    ("all empty", [(0, 0, 0, 0), (5, 5, 0, 7), (5, 5, 7, 0)], (0, (0, 0, 0, 0))),
    ("one box", [(4, 6, 10, 20)], (1, (4, 6, 10, 20))),
    ("one box among empty ones", [(0, 0, 0, 0), (4, 6, 10, 20), (0, 0, 0, 0)], (1, (4, 6, 10, 20))),
    ("disjoint", [(0, 0, 10, 10), (100, 50, 20, 30)], (2, (0, 0, 120, 80))),
    ("nested", [(10, 10, 100, 100), (20, 30, 5, 5)], (2, (10, 10, 100, 100))),
    ("overlapping", [(10, 20, 30, 40), (0, 30, 20, 50), (35, 0, 10, 25)], (3, (0, 0, 45, 80))),
]


@pytest.mark.parametrize("name,boxes,want", UNIONS, ids=[u[0] for u in UNIONS])
def test_union(name, boxes, want):
    assert B.union(boxes) == want
    for order in (boxes, boxes[::-1]):                           # commutative
        n, u = bars_union(order)
        assert (n, u.as_tuple()[:4]) == want
        assert (u.rows, u.cols, u.reserved[0], u.reserved[1]) == (0, 0, 0, 0)
    recs = [LumaBars(*b, 7, 9) for b in boxes]                  # rows / cols of the inputs are not carried over
    n, u = bars_union(recs)
    assert (n, u.as_tuple()) == (want[0], want[1] + (0, 0))


def test_union_null_arguments():
    L = lib()
    assert L.mvhp_bars_union(None, 0, None) == 0
    out = LumaBars(1, 2, 3, 4, 5, 6)
    assert L.mvhp_bars_union(None, 3, out) == 0 and out.as_tuple() == (0, 0, 0, 0, 0, 0)


TRIMS = [
    # name, crop, union, accepted, rectangle
    ("letterbox 1080p", (0, 0, 1920, 1080), (0, 140, 1920, 800), 1, (0, 140, 1920, 800)),
    ("odd edges round outward", (0, 0, 640, 360), (11, 21, 599, 301), 1, (10, 20, 600, 302)),
    ("odd left, even right", (0, 0, 640, 360), (11, 20, 589, 300), 1, (10, 20, 590, 300)),
    ("exactly half of the width", (0, 0, 640, 360), (100, 0, 320, 360), 1, (100, 0, 320, 360)),
    ("two samples less than half of the width", (0, 0, 640, 360), (100, 0, 318, 360), 0, (0, 0, 640, 360)),
    ("exactly half of the height", (0, 0, 640, 360), (0, 90, 640, 180), 1, (0, 90, 640, 180)),
    ("two samples less than half of the height", (0, 0, 640, 360), (0, 90, 640, 178), 0, (0, 0, 640, 360)),
    ("half of an odd half: (cw + 1) / 2", (0, 0, 642, 362), (0, 0, 322, 182), 1, (0, 0, 322, 182)),
    ("one step below it", (0, 0, 642, 362), (0, 0, 320, 182), 0, (0, 0, 642, 362)),
    ("rounding outward reaches half", (0, 0, 640, 360), (101, 0, 318, 360), 1, (100, 0, 320, 360)),
    ("union outside the crop", (0, 0, 640, 360), (700, 400, 100, 100), 0, (0, 0, 640, 360)),
    ("union touching the crop from outside", (16, 16, 640, 360), (0, 0, 16, 400), 0, (16, 16, 640, 360)),
    ("empty union", (0, 0, 640, 360), (0, 0, 0, 0), 0, (0, 0, 640, 360)),
    ("union larger than the crop", (8, 4, 640, 360), (0, 0, 2000, 2000), 1, (8, 4, 640, 360)),
    ("crop at an offset", (8, 4, 640, 352), (0, 47, 700, 271), 1, (8, 46, 640, 272)),
    ("crop at an offset, pillarbox", (8, 4, 640, 352), (89, 0, 481, 400), 1, (88, 4, 482, 352)),
    ("crop at an offset, the union mostly outside", (320, 0, 320, 360), (0, 0, 400, 360), 0, (320, 0, 320, 360)),
    ("the smallest crop", (0, 0, 2, 2), (1, 1, 1, 1), 1, (0, 0, 2, 2)),
]


@pytest.mark.parametrize("name,crop,u,ok,want", TRIMS, ids=[t[0] for t in TRIMS])
def test_trim_rect(name, crop, u, ok, want):
    assert B.trim_rect(crop, u) == (ok, want)
    rc, g = trim_rect(geometry(*crop, 6, 8), u)                  # (out_w / out_h of the crop are not read)
    assert (rc, _all(g)) == (ok, want + want[2:])
    assert (g.reserved[0], g.reserved[1]) == (0, 0)
    x, y, w, h = _rect(g)
    assert x % 2 == y % 2 == w % 2 == h % 2 == 0
    assert crop[0] <= x and crop[1] <= y and x + w <= crop[0] + crop[2] and y + h <= crop[1] + crop[3]


def test_trim_rect_null_union_and_in_place():
    crop = geometry(4, 6, 100, 80)
    rc, g = trim_rect(crop, None)
    assert (rc, _all(g)) == (0, (4, 6, 100, 80, 100, 80))
    u = LumaBars(10, 10, 80, 60)
    assert lib().mvhp_trim_rect(crop, u, crop) == 1              # out may be crop
    assert _all(crop) == (10, 10, 80, 60, 80, 60)


def test_trim_rect_random_against_ref():
    rng = np.random.default_rng(9)
    for _ in range(2000):
        cx, cy = (int(v) * 2 for v in rng.integers(0, 40, 2))
        cw, ch = (int(v) * 2 for v in rng.integers(1, 200, 2))
        u = tuple(int(v) for v in rng.integers(0, 300, 4))
        rc, g = trim_rect(geometry(cx, cy, cw, ch), u)
        assert (rc, _rect(g)) == B.trim_rect((cx, cy, cw, ch), u), ((cx, cy, cw, ch), u)


# ---- the stream's box and the geometry ----
CROPS = [(0, 0, 0, 4), (1, 3, 2, 1), (0, 0, 0, 0)]


def test_set_trim_and_read_back():
    stream, _ = gen.make_stream_crop(8, 6, 1, [CROPS[0]], seed=5)
    with Stream(stream) as s:
        assert stream_trim(s.h) == (0, 0, 0, 0)
        before = bytes(output_geometry(s.h, 0, "crop"))
        stream_set_trim(s.h, (10, 20, 90, 50))
        assert stream_trim(s.h) == (10, 20, 90, 50)
        assert bytes(output_geometry(s.h, 0, "crop")) == before            # setting it changes nothing by itself
        assert bytes(output_geometry(s.h, 0, None)) == bytes(geometry(0, 0, 128, 96))
        stream_set_trim(s.h, (10, 20, 0, 50))                              # an empty box clears it
        assert stream_trim(s.h) == (0, 0, 0, 0)
        stream_set_trim(s.h, LumaBars(1, 2, 3, 4, 5, 6))
        assert stream_trim(s.h) == (1, 2, 3, 4)
        stream_set_trim(s.h, None)
        assert stream_trim(s.h) == (0, 0, 0, 0)
    assert lib().mvhp_stream_set_trim(None, None) == 0 and lib().mvhp_stream_trim(None, None) == 0


def test_trim_without_a_box_is_the_crop():
    stream, _ = gen.make_stream_crop(8, 6, 3, CROPS, seed=5, sps_pps_every_frame=True)
    with Stream(stream) as s:
        for k in range(3):
            for output in (None, "crop", (40, 24), (33, 500)):
                for rotate in (None, 90, 180):
                    want = output_geometry(s.h, k, "crop" if output is None else output, rotate)
                    got = output_geometry(s.h, k, output, rotate, trim=True)
                    assert bytes(got) == bytes(want), (k, output, rotate)
        g = OutputGeometry()                                               # the flag alone
        assert lib().mvhp_output_geometry(s.h, 1, OutputRequest(OUTPUT_TRIM, 0, 0, 0), g) == 1
        assert bytes(g) == bytes(output_geometry(s.h, 1, "crop"))
        assert lib().mvhp_output_geometry(s.h, 1, OutputRequest(OUTPUT_TRIM | 0x40, 0, 0, 0), g) == 0     # 0x40 stays unknown


def test_trim_geometry_with_box_and_turns():
    stream, _ = gen.make_stream_crop(8, 6, 3, CROPS, seed=5, sps_pps_every_frame=True)
    box = (3, 17, 110, 55)                                                 # odd edges: rounded outward inside every crop
    with Stream(stream) as s:
        stream_set_trim(s.h, box)
        for k in range(3):
            crop = _rect(stream_crop(s.h, k))
            ok, rect = B.trim_rect(crop, box)
            assert ok == 1 and rect != crop
            g = output_geometry(s.h, k, None, trim=True)
            assert _all(g) == rect + rect[2:]
            assert bytes(g) == bytes(output_geometry(s.h, k, "crop", trim=True))
            for bw, bh in ((40, 24), (24, 40), (33, 33), (500, 500), (2, 2)):
                assert _all(output_geometry(s.h, k, (bw, bh), trim=True)) == rect + R.fit(rect[2], rect[3], bw, bh)
                for turns in (1, 2, 3):                                    # the sides are exchanged last
                    fw, fh = R.fit(rect[2], rect[3], *((bh, bw) if turns & 1 else (bw, bh)))
                    want = rect + ((fh, fw) if turns & 1 else (fw, fh))
                    assert _all(output_geometry(s.h, k, (bw, bh), 90 * turns, trim=True)) == want
            assert _all(output_geometry(s.h, k, None, 90, trim=True)) == rect + (rect[3], rect[2])
            assert bytes(output_geometry(s.h, k, "crop")) == bytes(geometry(*crop))        # without the flag: the SPS crop


def test_trim_geometry_with_aspect():
    vui = gen.vui_record(sar=(4, 3))
    stream, _ = gen.make_stream_vui(8, 6, 1, [vui], crops=[(0, 0, 0, 4)], seed=5)
    box = (0, 12, 128, 60)
    with Stream(stream) as s:
        stream_set_trim(s.h, box)
        ok, rect = B.trim_rect((0, 0, 128, 88), box)
        assert (ok, rect) == (1, (0, 12, 128, 60))
        a = color_ref.aspect(rect[2], rect[3], 4, 3)
        assert a == (128, 46)
        assert _all(output_geometry(s.h, 0, None, aspect=True, trim=True)) == rect + a
        assert _all(output_geometry(s.h, 0, (64, 64), aspect=True, trim=True)) == rect + R.fit(a[0], a[1], 64, 64)
        assert _all(output_geometry(s.h, 0, (64, 64), 270, aspect=True, trim=True)) == rect + R.fit(a[0], a[1], 64, 64)[::-1]


def test_a_picture_the_rule_refuses_keeps_its_crop():
    """a stream whose second SPS has another size: the box found on the first pictures leaves less than half of the second kind"""
    a, _ = gen.make_stream(20, 12, 2, seed=3)
    b, _ = gen.make_stream(8, 6, 2, seed=4)
    stream = np.concatenate([a, b, np.zeros(64, np.uint8)])
    box = (160, 20, 160, 150)                                              # the right half of 320 x 192
    with Stream(stream) as s:
        assert s.idr_count == 4
        sizes = [(s.params(k).width_mbs * 16, s.params(k).height_mbs * 16) for k in range(4)]
        assert sizes == [(320, 192)] * 2 + [(128, 96)] * 2
        stream_set_trim(s.h, box)
        for k in range(2):
            assert _all(output_geometry(s.h, k, None, trim=True)) == (160, 20, 160, 150, 160, 150)
        for k in (2, 3):                                                   # outside the smaller picture: its crop, no failure
            assert B.trim_rect((0, 0, 128, 96), box) == (0, (0, 0, 128, 96))
            assert _all(output_geometry(s.h, k, None, trim=True)) == (0, 0, 128, 96, 128, 96)
            assert _all(output_geometry(s.h, k, (64, 64), trim=True)) == (0, 0, 128, 96) + R.fit(128, 96, 64, 64)
        stream_set_trim(s.h, (0, 0, 70, 96))                               # inside both: accepted for the small, refused for the large
        assert _all(output_geometry(s.h, 0, None, trim=True)) == (0, 0, 320, 192, 320, 192)
        assert _all(output_geometry(s.h, 2, None, trim=True)) == (0, 0, 70, 96, 70, 96)


def test_request_flag_values():
    assert (OUTPUT_CROP, OUTPUT_TRIM) == (1, 0x2000)
