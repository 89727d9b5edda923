"""CPU: display orientation (DESIGN.md 3 "Orientation").  The tkhd matrix of an MP4's video track as quarter turns
(mvhp_stream_rotation), the output geometry under a request that turns (mvhp_output_geometry, mvhp_output_turns), and the NumPy
restatement of the turn (tests/orient_ref.py) against a plain per-sample loop."""
import numpy as np
import pytest

from minivideo_amd import gen
from minivideo_amd.hotpath import (OUTPUT_BOX, OUTPUT_CROP, OUTPUT_ORIENT, OutputGeometry, OutputRequest, lib, output_geometry,
                                   output_turns, stream_rotation)
from tests import orient_ref as O
from tests import resample_ref as R
from tests.mp4mux import mux
from tests.orient_streams import (NEG, ONE, ROTATIONS, W1, Mp4Stream, patch_matrix, patch_matrix_v1, rotated_mp4, tkhd_version1,
                                  truncate_tkhd)
from tests.util import Stream


@pytest.fixture(scope="module")
def clip():
    stream, _ = gen.make_stream(4, 3, 2, seed=3, profile="baseline")
    return stream, mux(stream, 64, 48)


def _rotation(mp4):
    with Mp4Stream(mp4) as s:
        assert s.ok
        return stream_rotation(s.h)


# ---- the matrix ----
@pytest.mark.parametrize("turns", [0, 1, 2, 3])
def test_the_four_rotations(clip, turns):
    assert _rotation(patch_matrix(clip[1], ROTATIONS[turns])) == 90 * turns
    v1 = tkhd_version1(clip[1])
    assert _rotation(v1) == 0                                   # (the muxer's identity, moved 12 bytes)
    assert _rotation(patch_matrix_v1(v1, ROTATIONS[turns])) == 90 * turns


def test_version1_file_still_decodes(clip):
    with Mp4Stream(tkhd_version1(clip[1])) as s:
        assert s.ok and s.L.mvhp_stream_idr_count(s.h) == 2


@pytest.mark.parametrize("name,words", [
    ("mirror x", (NEG, 0, 0, 0, ONE, 0, 0, 0, W1)),
    ("mirror y", (ONE, 0, 0, 0, NEG, 0, 0, 0, W1)),
    ("transpose", (0, ONE, 0, ONE, 0, 0, 0, 0, W1)),
    ("scale 2", (2 * ONE, 0, 0, 0, 2 * ONE, 0, 0, 0, W1)),
    ("turned and scaled", (0, 2 * ONE, 0, -2 * ONE, 0, 0, 0, 0, W1)),
    ("shear", (ONE, ONE // 2, 0, 0, ONE, 0, 0, 0, W1)),
    ("u", (0, ONE, 1, NEG, 0, 0, 0, 0, W1)),
    ("v", (0, ONE, 0, NEG, 0, 7, 0, 0, W1)),
    ("w", (0, ONE, 0, NEG, 0, 0, 0, 0, ONE)),
    ("all zero", (0,) * 9),
])
def test_everything_else_is_no_rotation(clip, name, words):
    assert _rotation(patch_matrix(clip[1], words)) == 0, name


def test_translation_is_ignored(clip):
    a, b, u, c, d, v, _, _, w = ROTATIONS[1]
    assert _rotation(patch_matrix(clip[1], (a, b, u, c, d, v, 48 * ONE, 0, w))) == 90
    a, b, u, c, d, v, _, _, w = ROTATIONS[2]
    assert _rotation(patch_matrix(clip[1], (a, b, u, c, d, v, 64 * ONE, 48 * ONE, w))) == 180


def test_truncated_box_is_identity(clip):
    turned = patch_matrix(clip[1], ROTATIONS[1])
    assert _rotation(turned) == 90
    cut = truncate_tkhd(turned, keep=20)          # a, b, u, c and d are still there; the box is too short for the matrix
    with Mp4Stream(cut) as s:
        assert s.ok and stream_rotation(s.h) == 0 and s.L.mvhp_stream_idr_count(s.h) == 2


def test_annexb_has_no_rotation(clip):
    with Stream(clip[0]) as s:
        assert s.ok and stream_rotation(s.h) == 0
        assert output_turns(s.h, None, "auto") == 0 and output_turns(s.h, None, 270) == 3
    assert stream_rotation(None) == 0


def test_turns_are_the_sum_modulo_four(clip):
    for own in range(4):
        with Mp4Stream(patch_matrix(clip[1], ROTATIONS[own])) as s:
            for q in range(4):
                req = OutputRequest(OUTPUT_ORIENT | (q << 4), 0, 0, 0)
                assert lib().mvhp_output_turns(s.h, req) == (own + q) % 4
                assert output_turns(s.h, None, 90 * q) == q          # an explicit angle is the field alone
            assert output_turns(s.h, None, "auto") == own
            assert output_turns(s.h, None, None) == 0


# ---- the geometry ----
def _geom(h, output, rotate):
    g = output_geometry(h, 0, output, rotate)
    return None if g is None else (g.crop_x, g.crop_y, g.crop_w, g.crop_h, g.out_w, g.out_h)


@pytest.fixture(scope="module")
def hd():
    """1920 x 1088 coded, cropped to 1080 rows, as MP4 files of each rotation"""
    stream, _ = gen.make_stream_crop(120, 68, 1, [(0, 0, 0, 4)], seed=2, profile="baseline")
    plain = mux(stream, 1920, 1080)
    return stream, {t: patch_matrix(plain, ROTATIONS[t]) for t in range(4)}


def test_full_hd_in_a_square_box(hd):
    with Mp4Stream(hd[1][0]) as s:
        assert _geom(s.h, (320, 320), "auto") == _geom(s.h, (320, 320), None) == (0, 0, 1920, 1080, 320, 180)
        assert _geom(s.h, (320, 320), 90) == (0, 0, 1920, 1080, 180, 320)
        assert _geom(s.h, (320, 320), 270) == (0, 0, 1920, 1080, 180, 320)
        assert _geom(s.h, (320, 320), 180) == (0, 0, 1920, 1080, 320, 180)
    with Mp4Stream(hd[1][1]) as s:
        assert _geom(s.h, (320, 320), "auto") == (0, 0, 1920, 1080, 180, 320)
        assert _geom(s.h, (320, 320), None) == (0, 0, 1920, 1080, 320, 180)       # nothing turns unless asked
        # the box is the box of the TURNED picture: 200 wide and 320 high lets the portrait picture keep 180 x 320
        assert _geom(s.h, (200, 320), "auto") == (0, 0, 1920, 1080, 180, 320)
        assert _geom(s.h, (320, 200), "auto") == (0, 0, 1920, 1080, 112, 200)


def test_crop_at_90(hd):
    with Mp4Stream(hd[1][1]) as s:
        assert _geom(s.h, "crop", "auto") == (0, 0, 1920, 1080, 1080, 1920)
        assert _geom(s.h, None, "auto") == (0, 0, 1920, 1088, 1088, 1920)          # without the crop: the coded rows, turned
    with Mp4Stream(hd[1][3]) as s:
        assert _geom(s.h, "crop", "auto") == (0, 0, 1920, 1080, 1080, 1920)
        assert _geom(s.h, "crop", 90) == (0, 0, 1920, 1080, 1080, 1920)            # an explicit angle is the field alone ...
        g = OutputGeometry()
        assert lib().mvhp_output_geometry(s.h, 0, OutputRequest(OUTPUT_CROP | OUTPUT_ORIENT | (1 << 4), 0, 0, 0), g) == 1
        assert (g.out_w, g.out_h) == (1920, 1080)                                  # ... and auto plus 90 on a 270 file sums to 0


def test_odd_box(hd):
    with Mp4Stream(hd[1][1]) as s:
        for bw, bh in ((321, 199), (199, 321), (3, 1001), (1001, 3), (77, 77)):
            ow, oh = R.fit(1920, 1080, bh, bw)                                    # formed against the box turned back ...
            assert _geom(s.h, (bw, bh), "auto") == (0, 0, 1920, 1080, oh, ow)      # ... and exchanged
            assert oh <= bw and ow <= bh and ow % 2 == 0 and oh % 2 == 0


def test_zero_turns_is_the_request_without_the_flags():
    stream, _ = gen.make_stream_crop(8, 6, 4, [(0, 0, 0, 4), (1, 3, 2, 1), (0, 0, 0, 0), (7, 0, 0, 7)], seed=5, sps_pps_every_frame=True)
    boxes = [None, "crop"] + [(w, h) for w in (2, 3, 20, 63, 64, 128, 500) for h in (2, 17, 48, 96, 500)]
    with Stream(stream) as s:
        for k in range(4):
            for output in boxes:
                want = output_geometry(s.h, k, output)
                for rotate in ("auto", 0):
                    got = output_geometry(s.h, k, output, rotate)
                    assert bytes(got) == bytes(want), (k, output, rotate)
    with Mp4Stream(rotated_mp4(stream, 128, 96, 3)) as s:      # 270 + 90: the sum is what counts
        for k in range(4):
            for output in boxes:
                assert bytes(output_geometry(s.h, k, output, None)) == bytes(output_geometry(s.h, k, output, None))
                req = OutputRequest(OUTPUT_ORIENT | (1 << 4), 0, 0, 0)
                if output is not None:
                    req.flags |= OUTPUT_CROP
                if isinstance(output, tuple):
                    req.flags |= OUTPUT_BOX
                    req.box_w, req.box_h = output
                g = OutputGeometry()
                assert lib().mvhp_output_geometry(s.h, k, req, g) == 1
                assert bytes(g) == bytes(output_geometry(s.h, k, output)), (k, output)


def test_bytes_do_not_change_with_the_turn():
    stream, _ = gen.make_stream_crop(8, 6, 2, [(1, 3, 2, 1), (0, 0, 0, 0)], seed=6, sps_pps_every_frame=True)
    L = lib()
    with Stream(stream) as s:
        for k in range(2):
            for output in (None, "crop", (40, 24), (24, 40), (33, 33)):
                for turns in (1, 2, 3):
                    t = output_geometry(s.h, k, output, 90 * turns)
                    # the unturned picture it is made of: the same request against the box turned back
                    back = output if not (turns & 1 and isinstance(output, tuple)) else (output[1], output[0])
                    u = output_geometry(s.h, k, back)
                    assert (t.out_w, t.out_h) == O.turned_size(u.out_w, u.out_h, turns)
                    assert (t.crop_x, t.crop_y, t.crop_w, t.crop_h) == (u.crop_x, u.crop_y, u.crop_w, u.crop_h)
                    assert L.mvhp_geometry_yuv_bytes(t) == L.mvhp_geometry_yuv_bytes(u)
                    assert L.mvhp_geometry_rgb_bytes(t) == L.mvhp_geometry_rgb_bytes(u)


# ---- the restatement ----
@pytest.mark.parametrize("shape", [(2, 2), (4, 6), (6, 4), (5, 3), (1, 7), (8, 8)])
@pytest.mark.parametrize("turns", [0, 1, 2, 3])
def test_numpy_form_matches_the_loop(shape, turns):
    h, w = shape
    p = np.random.default_rng(h * 16 + w + turns).integers(0, 256, (h, w)).astype(np.uint8)
    assert np.array_equal(O.turn_plane(p, turns), O.turn_plane_loop(p, turns))


def test_pictures_turn_plane_by_plane():
    w, h, n = 6, 4, 3
    planes = np.random.default_rng(1).integers(0, 256, (n, w * h * 3 // 2), dtype=np.uint8)
    for turns in range(4):
        t = O.turn(planes, w, h, turns)
        tw, th = O.turned_size(w, h, turns)
        for f in range(n):
            assert np.array_equal(t[f, :w * h].reshape(th, tw), O.turn_plane_loop(planes[f, :w * h].reshape(h, w), turns))
            cb = planes[f, w * h:w * h * 5 // 4].reshape(h // 2, w // 2)
            assert np.array_equal(t[f, w * h:w * h * 5 // 4].reshape(th // 2, tw // 2), O.turn_plane_loop(cb, turns))
            cr = planes[f, w * h * 5 // 4:].reshape(h // 2, w // 2)
            assert np.array_equal(t[f, w * h * 5 // 4:].reshape(th // 2, tw // 2), O.turn_plane_loop(cr, turns))
    # four quarter turns, and two half turns, give the source back
    cur, cw, ch = planes, w, h
    for _ in range(4):
        cur = O.turn(cur, cw, ch, 1)
        cw, ch = ch, cw
    assert np.array_equal(cur, planes) and np.array_equal(O.turn(O.turn(planes, w, h, 2), w, h, 2), planes)


def test_rgb_of_the_turned_planes_is_the_turned_rgb():
    """all sides are even, so a 2 x 2 chroma cell stays a 2 x 2 cell"""
    w, h, n = 10, 6, 2
    planes = np.random.default_rng(2).integers(0, 256, (n, w * h * 3 // 2), dtype=np.uint8)
    rgb = R.to_rgb(planes, w, h).reshape(n, h, w, 3)
    for turns in range(4):
        tw, th = O.turned_size(w, h, turns)
        got = O.to_rgb(O.turn(planes, w, h, turns), w, h, turns).reshape(n, th, tw, 3)
        for f in range(n):
            assert np.array_equal(got[f], np.rot90(rgb[f], O.ROT90_K[turns]))
