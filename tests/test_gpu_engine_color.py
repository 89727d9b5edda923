"""GPU: the decode engine under MVHP_OUTPUT_ASPECT and MVHP_OUTPUT_COLOR (Engine.decode(..., aspect=True, color=...)) on streams of
5 x 3 macroblocks with an SPS crop and a VUI.  Expected pictures, byte for byte: the oracle's reconstruction of the generator's
records (oracle/loader.py), tests/resample_ref.py on a geometry worked out here from the crop offsets, the aspect rule and the box
(tests/color_ref.py, not the library), tests/orient_ref.py, and tests/color_ref.py with the parameters resolved here from the VUI
record the test wrote -- centred chroma where the pass scaled.  The planes of the same call without the colour flag are those of
the chain, PNG files decode to its RGB, a stream whose SPSs alternate between two VUIs gets each picture its own setting, and
without the flags nothing moves: the bytes and launch counts of a stream without VUI, and of the reference decoder where it is
built."""
import io

import numpy as np
import pytest

from minivideo_amd import Engine, gen
from minivideo_amd.hotpath import StreamParams
from oracle import loader
from tests import color_ref as K
from tests import orient_ref as O
from tests import refdec
from tests import resample_ref as R
from tests.util import Stream

pytestmark = pytest.mark.gpu

W, H, F = 5, 3, 6
CROP = (1, 2, 0, 3)                       # 74 x 42 visible
SAR = (4, 3)                              # -> 74 x 32 with square samples
DISPLAY = dict(signal_present=1, full_range=1, matrix_coefficients=1, chroma_loc=0)      # BT.709 full range, left-sited chroma
SHAPES = {"coded": dict(), "crop": dict(output="crop"), "box": dict(output=(40, 24)), "aspect": dict(aspect=True),
          "aspect+box": dict(aspect=True, output=(40, 24)), "aspect+rotate": dict(aspect=True, rotate=90)}
KINDS = {"rgb": dict(want_rgb=1), "rgb_only": dict(want_rgb=3), "png": dict(png=True)}


@pytest.fixture(scope="module")
def clip():
    """(stream with crop and VUI, the same macroblocks without VUI, oracle planes per picture)"""
    kw = dict(seed=23, profile="high", sps_pps_every_frame=True, qp_range=(20, 40))
    rec = gen.vui_record(sar=SAR, full_range=1, matrix=1, chroma_loc=0, overscan=0, timing=True)
    stream, packed = gen.make_stream_vui(W, H, F, [rec], crops=[CROP], **kw)
    plain, packed0 = gen.make_stream_crop(W, H, F, [CROP], **kw)
    assert np.array_equal(packed, packed0)
    planes = loader.recon(StreamParams(W, H, 0, 0, 1), packed, F)[0].reshape(F, -1)
    return stream, plain, planes


def chain(planes_k, shape, sar=SAR, crop=CROP):
    """-> (delivered geometry, planes, scaled): the geometry from the crop offsets, the aspect rule, the box (turned back for an
    odd turn), then the turn"""
    kw = SHAPES[shape] if isinstance(shape, str) else shape
    turns = (kw.get("rotate") or 0) // 90
    l, r, t, b = crop
    if not kw:
        g = (0, 0, 16 * W, 16 * H, 16 * W, 16 * H)
    else:
        cw, ch = 16 * W - 2 * (l + r), 16 * H - 2 * (t + b)
        dw, dh = K.aspect(cw, ch, *sar) if kw.get("aspect") else (cw, ch)
        if isinstance(kw.get("output"), tuple):
            bw, bh = kw["output"][::-1] if turns & 1 else kw["output"]
            dw, dh = R.fit(dw, dh, bw, bh)
        g = (2 * l, 2 * t, cw, ch, dw, dh)
    out = O.turn(R.resample(planes_k, W, H, g), g[4], g[5], turns)
    return g[:4] + O.turned_size(g[4], g[5], turns), out.reshape(-1), (g[4], g[5]) != (g[2], g[3])


def expected_rgb(planes, geom, scaled, color, display=DISPLAY):
    matrix, full, siting = K.resolve(display, 16 * W, 16 * H, color)
    if scaled:
        siting = K.CENTER
    return K.to_rgb(planes, geom[4], geom[5], matrix, full, siting).reshape(-1)


def run(handle, order, batch_pictures=3, **kw):
    got = {}

    def sink(seq, idr, rc, err, p, *rest):
        geom, yuv, rgb = rest if len(rest) == 3 else (None,) + rest      # (a call without any request: the plain sink)
        g = geom and (geom.crop_x, geom.crop_y, geom.crop_w, geom.crop_h, geom.out_w, geom.out_h)
        got[seq] = (idr, rc, err, g, None if yuv is None else yuv.copy(), None if rgb is None else rgb.copy())
        return 1 if rc == 1 else 0

    eng = Engine(contexts=kw.pop("contexts", 2), chunk_pictures=2, batch_pictures=batch_pictures)
    try:
        rc, st = eng.decode(handle, order, sink=sink, **kw)
    finally:
        eng.close()
    assert rc == 1 and sorted(got) == list(range(len(order))) and st["pictures_ok"] == len(order), st
    return st, got


def png_pixels(data):
    Image = pytest.importorskip("PIL.Image")
    im = Image.open(io.BytesIO(bytes(data)))
    assert im.mode == "RGB"
    return np.asarray(im).reshape(-1), im.size


@pytest.mark.parametrize("color", ["auto", "bt709-full", "bt601"])
@pytest.mark.parametrize("shape", list(SHAPES))
@pytest.mark.parametrize("kind", list(KINDS))
def test_rgb_is_the_colour_pass_over_the_final_planes(clip, kind, shape, color):
    stream, _, planes = clip
    order = list(range(F))
    with Stream(stream) as s:
        st, got = run(s.h, order, color=color, **KINDS[kind], **SHAPES[shape])
        st0, got0 = run(s.h, order, **KINDS[kind], **SHAPES[shape])      # the same call without the colour flag
    for k in order:
        geom, wy, scaled = chain(planes[k], shape)
        wr = expected_rgb(wy, geom, scaled, color)
        assert got[k][0] == k and got[k][3] == geom, (k, got[k][3], geom)
        if kind == "png":
            assert got[k][4] is None and got0[k][4] is None
            px, size = png_pixels(got[k][5])
            assert size == (geom[4], geom[5]) and np.array_equal(px, wr), k
            assert np.array_equal(png_pixels(got0[k][5])[0], R.to_rgb(wy, geom[4], geom[5]).reshape(-1))
        else:
            assert np.array_equal(got[k][5], wr), k
            assert np.array_equal(got0[k][5], R.to_rgb(wy, geom[4], geom[5]).reshape(-1)), k      # (without the flag: today's formula)
            if kind == "rgb":
                assert np.array_equal(got[k][4], wy) and np.array_equal(got0[k][4], wy), k
            else:
                assert got[k][4] is None
    assert st["batches"] == st0["batches"] and st["geometry_launches"] == st0["geometry_launches"]      # one setting: no split
    if kind != "png":
        assert st["d2h_bytes"] == st0["d2h_bytes"]


@pytest.mark.parametrize("sar,want", [((4, 3), (74, 32)), ((10, 11), (68, 42)), (14, (74, 32)), (None, (74, 42)), ((1, 1), (74, 42))])
def test_aspect_alone(sar, want):
    """the geometry is the rule's, and the pictures are the area average on the anisotropic geometry: one axis shrinks"""
    kw = dict(seed=29, profile="main", sps_pps_every_frame=True)
    stream, packed = gen.make_stream_vui(W, H, 4, [gen.vui_record(sar=sar)], crops=[CROP], **kw)
    planes = loader.recon(StreamParams(W, H, 0, 0, 0), packed, 4)[0].reshape(4, -1)
    ab = (0, 0) if sar is None else K.sar(255, sar) if isinstance(sar, tuple) else K.sar(sar)
    with Stream(stream) as s:
        st, got = run(s.h, list(range(4)), want_rgb=1, aspect=True)
    for k in range(4):
        geom, wy, scaled = chain(planes[k], "aspect", sar=ab)
        assert geom[4:] == want and got[k][3] == geom
        assert np.array_equal(got[k][4], wy), k
        assert np.array_equal(got[k][5], R.to_rgb(wy, *want).reshape(-1)), k


def test_every_picture_gets_its_own_setting(clip):
    """SPSs alternate between BT.709 full range / centred and BT.601 limited / left: batches split at every picture under "auto";
    a forced matrix still splits on the siting; crops and sizes do not differ"""
    kw = dict(seed=31, profile="baseline", sps_pps_every_frame=True)
    a = gen.vui_record(sar=SAR, full_range=1, matrix=1, chroma_loc=1)
    b = gen.vui_record(sar=SAR, full_range=0, matrix=6, chroma_loc=2, timing=True)
    stream, packed = gen.make_stream_vui(W, H, F, [a, b], crops=[CROP], **kw)
    planes = loader.recon(StreamParams(W, H, 0, 0, 0), packed, F)[0].reshape(F, -1)
    shows = [dict(signal_present=1, full_range=1, matrix_coefficients=1, chroma_loc=1),
             dict(signal_present=1, full_range=0, matrix_coefficients=6, chroma_loc=2)]
    order = list(range(F))
    with Stream(stream) as s:
        for shape, color, batches in (("crop", "auto", F), ("crop", "bt601", F), ("aspect", "auto", F), ("aspect", "bt709", 2), ("crop", None, 2)):
            st, got = run(s.h, order, batch_pictures=4, contexts=1, want_rgb=3, color=color, **SHAPES[shape])
            for k in order:
                geom, wy, scaled = chain(planes[k], shape)
                want = expected_rgb(wy, geom, scaled, color, shows[k & 1]) if color else R.to_rgb(wy, geom[4], geom[5]).reshape(-1)
                assert got[k][3] == geom and np.array_equal(got[k][5], want), (shape, color, k)
                if color == "auto":      # (the other record's setting gives another picture: the case tests what it says)
                    assert not np.array_equal(want, expected_rgb(wy, geom, scaled, color, shows[(k + 1) & 1]))
            assert st["batches"] == batches, (shape, color, st["batches"])      # (2: six pictures in batches of four)


@pytest.mark.parametrize("kind", list(KINDS))
@pytest.mark.parametrize("shape", ["coded", "crop", "box"])
def test_without_the_flags_nothing_moves(clip, kind, shape):
    """the VUI is read and nothing else happens: the outputs and the launch counts of the stream without VUI"""
    stream, plain, planes = clip
    order = list(range(F))
    with Stream(stream) as s, Stream(plain) as s0:
        st, got = run(s.h, order, aspect=False, color=None, **KINDS[kind], **SHAPES[shape])
        st0, got0 = run(s0.h, order, **KINDS[kind], **SHAPES[shape])
    for k in order:
        assert got[k][:4] == got0[k][:4]
        for i in (4, 5):
            assert (got[k][i] is None and got0[k][i] is None) or np.array_equal(got[k][i], got0[k][i]), (k, i)
    for key in ("batches", "geometry_launches", "d2h_bytes", "launches_by_layout", "launches_wide", "pictures_issued"):
        assert st[key] == st0[key], key


def test_color_where_no_rgb_is_delivered_changes_nothing(clip):
    stream, _, planes = clip
    order = list(range(F))
    with Stream(stream) as s:
        st, got = run(s.h, order, want_rgb=0, color="auto", output="crop")
        st0, got0 = run(s.h, order, want_rgb=0, output="crop")
        stj, gotj = run(s.h, order, jpeg=90, color="bt709-full")
        stj0, gotj0 = run(s.h, order, jpeg=90)
    for k in order:
        assert got[k][5] is None and np.array_equal(got[k][4], got0[k][4]) and np.array_equal(got[k][4], chain(planes[k], "crop")[1])
        assert np.array_equal(gotj[k][5], gotj0[k][5])
    for key in ("batches", "geometry_launches", "d2h_bytes"):
        assert st[key] == st0[key] and stj[key] == stj0[key], key


def test_reference_decoder_reads_the_vui_and_decodes_the_same_planes(clip):
    """the reference parses these VUI fields and traces them: its planes of the VUI stream are ours, which have not moved"""
    refdec.require()
    stream, _, planes = clip
    ref = refdec.pictures(stream, "yuv420", F)
    with Stream(stream) as s:
        st, got = run(s.h, list(range(F)), want_rgb=0)
    for k in range(F):
        assert np.array_equal(np.frombuffer(ref[k], np.uint8), planes[k]) and np.array_equal(got[k][4], planes[k]), k
