"""GPU: the decode engine with MVHP_OUTPUT_BARS (Engine.decode(..., bars=...)) and MVHP_OUTPUT_TRIM (stream_set_trim() +
Engine.decode(..., trim=True)).  The generator has no black macroblocks to offer, so the bars are made with its existing means:
the level is a parameter, and at a level near the top of the samples only a few of them are bright -- the pictures then have
boxes of their own (inside the rectangle, the whole rectangle, none at all), as letterboxed pictures have at the default level.  Boxes: equal
to the restatement (tests/bars_ref.py) on the oracle's planes over the geometry's rectangle, whatever the batch size, the pictures
byte-identical to the call without the flag.  Trimming: planes, RGB, JPEG and PNG equal resample_ref / orient_ref / jpeg_ref /
png_ref on the trimmed rectangle, and a box the trust rule refuses gives the pictures of output="crop"."""
import numpy as np
import pytest

from minivideo_amd import Engine, gen
from minivideo_amd.hotpath import StreamParams, output_geometry, stream_set_trim
from oracle import loader
from tests import bars_ref as B
from tests import jpeg_ref as J
from tests import orient_ref as O
from tests import png_ref as P
from tests import resample_ref as R
from tests.util import Stream

pytestmark = pytest.mark.gpu

W, H, F = 9, 7, 6
CROP = (1, 3, 2, 1)
RECT = (2, 4, 16 * W - 8, 16 * H - 6)


@pytest.fixture(scope="module")
def clip():
    """(Annex-B bytes, oracle planes per picture, a level at which the pictures have boxes of their own): computed once"""
    stream, packed = gen.make_stream_crop(W, H, F, [CROP], seed=43, profile="high", qp_range=(20, 44))
    yuv = loader.recon(StreamParams(W, H, 0, 0, 1), packed, F)[0].reshape(F, -1)
    luma = yuv[:, :256 * W * H]
    level = min(int(np.percentile(luma, 95)), 254)
    return stream, yuv, level


def _run(handle, order, **kw):
    got = {}

    def sink(seq, idr, rc, err, p, *rest):
        g, yuv, rgb = rest if len(rest) == 3 else (None,) + rest      # (a call without any request: the plain sink, no geometry)
        got[seq] = (idr, rc, g and (g.crop_x, g.crop_y, g.crop_w, g.crop_h, g.out_w, g.out_h), g and g.bars,
                    (g.reserved[0], g.reserved[1]) if g else (0, 0), None if yuv is None else yuv.tobytes(),
                    None if rgb is None else rgb.tobytes(), err)
        return 1 if rc == 1 else 0

    opts = {k: kw.pop(k) for k in ("contexts", "fail_context", "batch_pictures") if k in kw}
    opts.setdefault("batch_pictures", 3)
    eng = Engine(chunk_pictures=2, **opts)
    try:
        rc, st = eng.decode(handle, order, sink=sink, **kw)
    finally:
        eng.close()
    assert sorted(got) == list(range(len(order)))
    return rc, st, got


def test_the_content_has_boxes(clip):
    _, planes, level = clip
    boxes = [B.record(B.luma_plane(planes[k], W, H), RECT, level)[:4] for k in range(F)]
    assert len(set(boxes)) >= 4, boxes
    assert any(b == (0, 0, 0, 0) for b in boxes) and any(b[2] > 0 and b != RECT for b in boxes), boxes
    assert all(B.record(B.luma_plane(planes[k], W, H), RECT)[:4] == RECT for k in range(F))     # at the default level: no bars


@pytest.mark.parametrize("batch,contexts", [(1, 1), (64, 1), (3, 3)])
@pytest.mark.parametrize("output", [None, "crop", (40, 24)])
def test_boxes_and_unchanged_pictures(clip, output, batch, contexts):
    stream, planes, level = clip
    order = list(range(F)) * 2
    rect = (0, 0, 16 * W, 16 * H) if output is None else RECT
    with Stream(stream) as s:
        assert s.ok
        rc0, st0, off = _run(s.h, order, output=output, want_rgb=1, batch_pictures=batch, contexts=contexts)
        for bars, lv in ((True, B.LEVEL), (level, level)):
            rc1, st1, on = _run(s.h, order, output=output, want_rgb=1, bars=bars, batch_pictures=batch, contexts=contexts,
                                fail_context=0 if contexts == 3 else -1)
            assert rc0 == 1 and rc1 == 1 and st1["pictures_ok"] == len(order) and st1["pictures_failed"] == 0
            assert st1["batches_requeued"] == (1 if contexts == 3 else 0)
            for seq, k in enumerate(order):
                want = B.record(B.luma_plane(planes[k], W, H), rect, lv)[:4]
                assert on[seq][3] == want, (seq, lv, on[seq][3], want)
                assert off[seq][2] in (None, on[seq][2]) and off[seq][4] == (0, 0), seq   # the same geometry; without the flag the words are 0
                assert on[seq][5] == off[seq][5] and on[seq][6] == off[seq][6], seq        # the same pictures, byte for byte
            assert st1["d2h_bytes"] == st0["d2h_bytes"] + 32 * len(order)
            if output is None:
                assert st1["geometry_launches"] == 0


def test_refusals(clip):
    stream, _, _ = clip
    eng = Engine(contexts=1)
    try:
        with Stream(stream) as s:
            for kw in (dict(jpeg=75), dict(png=True), dict(score=True)):
                with pytest.raises(ValueError):
                    eng.decode(s.h, [0], sink=lambda *a: 1, bars=True, **kw)
            with pytest.raises(ValueError):
                eng.decode(s.h, [0], bars=True)                                          # no sink: nowhere to deliver the boxes
            for bad in (0, 255, -3):
                with pytest.raises(ValueError):
                    eng.decode(s.h, [0], sink=lambda *a: 1, bars=bad)
            rc, st = eng.decode(s.h, [0, 1])                                              # (and the engine still works)
            assert rc == 1 and st["pictures_ok"] == 2
    finally:
        eng.close()


BOX = (21, 13, 101, 71)      # odd edges: rounded outward, inside the crop rectangle


def _want(planes_k, rect, output, turns):
    """-> (delivered geometry, planes, RGB) of the rectangle `rect` under a box and a turn"""
    size = rect[2:] if output in (None, "crop") else R.fit(rect[2], rect[3], *((output[1], output[0]) if turns & 1 else output))
    g = tuple(rect) + tuple(size)
    t = O.turn(R.resample(planes_k, W, H, g), g[4], g[5], turns)
    return g[:4] + O.turned_size(g[4], g[5], turns), t.reshape(-1), O.to_rgb(t, g[4], g[5], turns).reshape(-1)


@pytest.mark.parametrize("output,angle", [(None, None), ("crop", None), ((40, 24), None), (None, 90), ((40, 24), 90), ((24, 40), 270)])
def test_trimmed_pictures(clip, output, angle):
    stream, planes, _ = clip
    ok, rect = B.trim_rect(RECT, BOX)
    assert ok == 1 and rect == (20, 12, 102, 72)
    order = list(range(F))
    turns = (angle or 0) // 90
    with Stream(stream) as s:
        stream_set_trim(s.h, BOX)
        g = output_geometry(s.h, 0, output, angle, trim=True)
        rc, st, got = _run(s.h, order, output=output, rotate=angle, trim=True, want_rgb=1)
        # (JPEG not for the 16 x 24 pictures of a box and a turn: their files are longer than the raw pictures the blob has room for)
        with_jpeg = not (turns and isinstance(output, tuple))
        jpg = _run(s.h, order, output=output, rotate=angle, trim=True, jpeg=75)[2] if with_jpeg else None
        rcp, _, png = _run(s.h, order, output=output, rotate=angle, trim=True, png=True)
    assert rc == 1 and rcp == 1 and st["geometry_launches"] == st["batches"]
    for k in order:
        wg, wy, wr = _want(planes[k], rect, output, turns)
        assert (g.crop_x, g.crop_y, g.crop_w, g.crop_h, g.out_w, g.out_h) == wg
        assert got[k][1] == 1 and got[k][2] == wg, (k, got[k][2], wg)
        assert got[k][5] == wy.tobytes() and got[k][6] == wr.tobytes(), k
        if with_jpeg:
            assert jpg[k][6] == bytes(J.encode(wy, wg[4], wg[5], 75)), k
        assert png[k][6] == bytes(P.encode(wr, wg[4], wg[5])), k


@pytest.mark.parametrize("box", [(0, 0, 60, 200), (30, 30, 130, 40), (300, 300, 10, 10), None])
def test_a_refused_box_is_the_crop(clip, box):
    """less than half of a side left, a box outside the picture, no box: the pictures of output="crop" """
    stream, _, _ = clip
    assert B.trim_rect(RECT, box) == (0, RECT)
    order = list(range(F))
    with Stream(stream) as s:
        rc0, st0, crop = _run(s.h, order, output="crop", want_rgb=1)
        stream_set_trim(s.h, box)
        rc1, st1, trim = _run(s.h, order, trim=True, want_rgb=1)
        rc2, _, boxed = _run(s.h, order, output=(40, 24), trim=True, want_rgb=1)
        stream_set_trim(s.h, None)
        rc3, _, boxed0 = _run(s.h, order, output=(40, 24), want_rgb=1)
    assert rc0 == rc1 == rc2 == rc3 == 1 and st0["d2h_bytes"] == st1["d2h_bytes"]
    for k in order:
        assert trim[k][:7] == crop[k][:7] and boxed[k][:7] == boxed0[k][:7], k
