"""GPU: the decode engine with MVHP_OUTPUT_HIST (Engine.decode(..., hist=True), Engine.picture_hist(seq) inside the sink) on
generator streams: every delivered picture's record equals the restatement's (tests/hist_ref.py) on the oracle's coded planes
over the geometry's crop rectangle, all 3104 bytes, for planes, RGB only and JPEG output, at the coded size, cropped and boxed,
with one and three contexts, small batches and a failed context re-queued; the pictures are byte-identical to the same call
without the flag, d2h_bytes differs by exactly 3104 per picture, the flag alone runs no geometry launch, and the record's
mvhp_hist_stats score is the score MVHP_OUTPUT_SCORE delivers beside it."""
import numpy as np
import pytest

from minivideo_amd import Engine
from minivideo_amd.hotpath import PLANE_HIST_DTYPE, hist_stats, luma_score, output_geometry
from tests import blank_streams as B, hist_ref as R, luma_ref as L
from tests.util import Stream

pytestmark = pytest.mark.gpu

W, H = 20, 17
CROP = (1, 3, 2, 1)
BUSY = [0, 1, 0, 0, 1, 0, 1, 1]
F = len(BUSY)
KINDS = {"planes": dict(), "rgb_only": dict(want_rgb=3), "jpeg": dict(jpeg=75)}


@pytest.fixture(scope="module")
def content():
    """(stream, the oracle's coded planes per picture): computed once"""
    stream, _, planes, _ = B.mixed(W, H, BUSY, seed=5, profile="high", crop=CROP)
    return stream, planes


def _decode(s, order, output, kind, hist, score=False, **opts):
    got = {}
    eng = Engine(**opts)

    def sink(seq, idr, rc, err, p, *rest):
        g = rest[0] if len(rest) == 3 else None
        yuv, rgb = rest[-2], rest[-1]
        rec = eng.picture_hist(seq)
        others = [eng.picture_hist(k) for k in (seq - 1, seq + 1, -1, len(order))]
        got[seq] = (rc, err, None if g is None else (g.crop_x, g.crop_y, g.crop_w, g.crop_h, g.out_w, g.out_h, g.reserved[0]),
                    0 if g is None else g.score, None if yuv is None else yuv.tobytes(), None if rgb is None else rgb.tobytes(),
                    None if rec is None else rec.tobytes(), all(o is None for o in others))
        return 1 if rc == 1 else 0

    try:
        rc, st = eng.decode(s.h, order, sink=sink, output=output, hist=hist, score=score, **KINDS[kind])
        after = eng.picture_hist(0)
    finally:
        eng.close()
    assert after is None                                                           # the call is over
    return rc, st, got


def _want(s, planes, output):
    out = []
    for k in range(planes.shape[0]):
        g = output_geometry(s.h, k, output)
        out.append(R.record(planes[k], W, H, (g.crop_x, g.crop_y, g.crop_w, g.crop_h)))
    return out


def test_the_rectangle_matters(content):
    stream, planes = content
    with Stream(stream) as s:
        assert s.ok and s.idr_count == F
        coded, crop = _want(s, planes, None), _want(s, planes, "crop")
    assert all(a.tobytes() != b.tobytes() for a, b in zip(coded, crop))
    assert len({r.tobytes() for r in coded}) == F                                  # the pictures differ: a mix-up shows
    assert all(int(r["samples"][0]) == 256 * W * H for r in coded) and all(int(r["samples"][0]) < 256 * W * H for r in crop)


@pytest.mark.parametrize("contexts", [1, 3])
@pytest.mark.parametrize("output", [None, "crop", (40, 40)])
@pytest.mark.parametrize("kind", ["planes", "rgb_only", "jpeg"])
def test_records_and_unchanged_pictures(content, kind, output, contexts):
    stream, planes = content
    order = list(range(F)) * 2
    with Stream(stream) as s:
        assert s.ok
        want = _want(s, planes, output)
        opts = dict(contexts=contexts, batch_pictures=3, chunk_pictures=2)
        rc0, st0, off = _decode(s, order, output, kind, False, **opts)
        rc1, st1, on = _decode(s, order, output, kind, True, fail_context=0 if contexts == 3 else -1, **opts)
    assert rc0 == 1 and rc1 == 1 and st1["pictures_ok"] == len(order) and st1["pictures_failed"] == 0
    assert st1["batches_requeued"] == (1 if contexts == 3 else 0)
    for seq, idr in enumerate(order):
        assert on[seq][0] == 1 and on[seq][7] and off[seq][7]
        assert off[seq][6] is None                                                  # without the flag there is no record
        if on[seq][6] != want[idr].tobytes():
            got = np.frombuffer(on[seq][6], PLANE_HIST_DTYPE)[0]
            for p in ("y", "cb", "cr"):
                bad = np.nonzero(got[p] != want[idr][p][0])[0]
                assert bad.size == 0, (seq, idr, p, bad[:8], got[p][bad[:8]], want[idr][p][0][bad[:8]])
            assert False, (seq, idr, got["samples"], got["chroma_samples"], got["reserved"])
        assert on[seq][4] == off[seq][4] and on[seq][5] == off[seq][5], seq           # the same pictures, byte for byte
        assert on[seq][3] == 0                                                      # reserved[1] stays 0: no score was asked for
        if off[seq][2] is not None:
            assert on[seq][2] == off[seq][2], seq                                     # the same geometry and JPEG length
    assert st1["d2h_bytes"] == st0["d2h_bytes"] + 3104 * len(order)
    if output is None:
        assert st1["geometry_launches"] == 0
    if contexts < 3:
        assert st1["geometry_launches"] == st0["geometry_launches"]


@pytest.mark.parametrize("output", [None, "crop"])
def test_beside_the_score(content, output):
    """MVHP_OUTPUT_HIST with MVHP_OUTPUT_SCORE: both records travel, and the histogram's own score is the delivered one"""
    stream, planes = content
    order = list(range(F))
    with Stream(stream) as s:
        assert s.ok
        want = _want(s, planes, output)
        rects = [output_geometry(s.h, k, output) for k in range(F)]
        rc0, st0, off = _decode(s, order, output, "planes", False, contexts=2, batch_pictures=3, chunk_pictures=2)
        rc1, st1, on = _decode(s, order, output, "planes", True, score=True, contexts=2, batch_pictures=3, chunk_pictures=2)
    assert rc0 == 1 and rc1 == 1
    for k in range(F):
        g = rects[k]
        assert on[k][6] == want[k].tobytes() and on[k][4] == off[k][4]
        score = L.picture_score(planes[k], W, H, (g.crop_x, g.crop_y, g.crop_w, g.crop_h))
        assert on[k][3] == score == luma_score(hist_stats(np.frombuffer(on[k][6], PLANE_HIST_DTYPE)))
    assert st1["d2h_bytes"] == st0["d2h_bytes"] + (3104 + 32) * F


def test_hist_with_bars_is_refused(content):
    stream, _ = content
    with Stream(stream) as s:
        eng = Engine(contexts=1)
        try:
            with pytest.raises(ValueError):
                eng.decode(s.h, [0], sink=lambda *a: 1, bars=True, hist=True)
        finally:
            eng.close()
