"""GPU: the decode engine with MVHP_OUTPUT_SCORE (Engine.decode(..., score=True)) on streams that mix busy and blank pictures:
every delivered picture's score equals the restatement's (tests/luma_ref.py) on the expected coded planes -- oracle
reconstruction, deblock_ref where the stream asks for it -- over the geometry's crop rectangle, for planes, RGB only, crop, box
and JPEG output, with one to three contexts, small batches and a failed context re-queued; the pictures are byte-identical to the
same call without the flag, d2h_bytes differs by 32 per picture, and the flag alone runs no geometry launch."""
import numpy as np
import pytest

from minivideo_amd import Engine, gen
from minivideo_amd.hotpath import PARAM_DEBLOCK, STREAM_DEBLOCK, StreamParams, output_geometry
from oracle import loader
from tests import blank_streams as B, deblock_ref, luma_ref as L
from tests.test_deblock import DStream
from tests.util import Stream

pytestmark = pytest.mark.gpu

W, H = 20, 17
CROP = (1, 3, 2, 1)
BUSY = [0, 1, 0, 0, 1, 0, 1, 1]
F = len(BUSY)
KINDS = {"planes": dict(), "rgb_only": dict(want_rgb=3), "jpeg": dict(jpeg=75)}


@pytest.fixture(scope="module")
def content():
    """(stream, coded planes per picture): computed once"""
    stream, _, planes, _ = B.mixed(W, H, BUSY, seed=5, profile="high", crop=CROP)
    return stream, planes


def _decode(s, order, output, kind, score, wmb=W, hmb=H, **opts):
    got = {}

    def sink(seq, idr, rc, err, p, *rest):
        g = rest[0] if len(rest) == 3 else None
        yuv, rgb = rest[-2], rest[-1]
        got[seq] = (rc, err, None if g is None else (g.crop_x, g.crop_y, g.crop_w, g.crop_h, g.out_w, g.out_h, g.reserved[0]),
                    0 if g is None else g.score, None if yuv is None else yuv.tobytes(), None if rgb is None else rgb.tobytes())
        return 1 if rc == 1 else 0

    eng = Engine(**opts)
    try:
        rc, st = eng.decode(s.h, order, sink=sink, output=output, score=score, **KINDS[kind])
    finally:
        eng.close()
    return rc, st, got


def _want_scores(s, planes, output, wmb=W, hmb=H):
    out = []
    for k in range(planes.shape[0]):
        g = output_geometry(s.h, k, output)
        out.append(L.picture_score(planes[k], wmb, hmb, (g.crop_x, g.crop_y, g.crop_w, g.crop_h)))
    return out


def test_the_content_has_two_classes(content):
    stream, planes = content
    with Stream(stream) as s:
        assert s.ok and s.idr_count == F
        for output in (None, "crop"):
            sc = _want_scores(s, planes, output)
            assert all((v > B.MIN_SCORE) == bool(b) for v, b in zip(sc, BUSY)), sc
            assert all(v > B.BUSY_ABOVE if b else v < B.BLANK_BELOW for v, b in zip(sc, BUSY)), sc
        assert _want_scores(s, planes, None) != _want_scores(s, planes, "crop")     # the rectangle matters


@pytest.mark.parametrize("contexts", [1, 2, 3])
@pytest.mark.parametrize("output", [None, "crop", (40, 40)])
@pytest.mark.parametrize("kind", ["planes", "rgb_only", "jpeg"])
def test_scores_and_unchanged_pictures(content, kind, output, contexts):
    stream, planes = content
    order = list(range(F)) * 2
    with Stream(stream) as s:
        assert s.ok
        want = _want_scores(s, planes, output)
        opts = dict(contexts=contexts, batch_pictures=3, chunk_pictures=2)
        rc0, st0, off = _decode(s, order, output, kind, False, **opts)
        rc1, st1, on = _decode(s, order, output, kind, True, fail_context=0 if contexts == 3 else -1, **opts)
    assert rc0 == 1 and rc1 == 1 and st1["pictures_ok"] == len(order) and st1["pictures_failed"] == 0
    assert st1["batches_requeued"] == (1 if contexts == 3 else 0)
    for seq, idr in enumerate(order):
        assert on[seq][0] == 1 and on[seq][3] == want[idr], (seq, on[seq][3], want[idr])
        assert on[seq][4] == off[seq][4] and on[seq][5] == off[seq][5], seq           # the same pictures, byte for byte
        if off[seq][2] is not None:
            assert on[seq][2] == off[seq][2], seq                                       # the same geometry and JPEG length
            assert off[seq][3] == 0                                                     # without the flag reserved[1] stays 0
    assert st1["d2h_bytes"] == st0["d2h_bytes"] + 32 * len(order)
    if output is None:
        assert st1["geometry_launches"] == 0
    if contexts < 3:
        assert st1["geometry_launches"] == st0["geometry_launches"]


def test_large_pictures():
    wmb, hmb, busy = 120, 68, [1, 0, 1]
    stream, _, planes, _ = B.mixed(wmb, hmb, busy, seed=5, profile="high")
    with Stream(stream) as s:
        assert s.ok
        for output in (None, (320, 320)):
            want = _want_scores(s, planes, output, wmb, hmb)
            assert all((v > B.MIN_SCORE) == bool(b) for v, b in zip(want, busy)), want
            rc, st, got = _decode(s, [0, 1, 2], output, "planes", True, wmb, hmb, contexts=2, batch_pictures=2)
            assert rc == 1 and [got[k][3] for k in range(3)] == want
            if output is None:
                assert st["geometry_launches"] == 0
                assert [got[k][4] for k in range(3)] == [planes[k].tobytes() for k in range(3)]


def test_deblocked_stream():
    """the scores are those of the planes AFTER the deblocking filter"""
    w, h, n = 9, 7, 4
    stream, packed, _ = gen.make_stream_ex(w, h, n, seed=23, profile="high", deblock=dict(idc=(0, 1, 2), offsets=(-6, 6)))
    with DStream(stream, STREAM_DEBLOCK) as s:
        assert s.ok
        p = s.params(0)
        assert p.flags & PARAM_DEBLOCK
        off = StreamParams.from_buffer_copy(p)
        off.flags = p.flags & ~PARAM_DEBLOCK
        plain = np.asarray(loader.recon(off, packed, n)[0]).reshape(n, -1)
        planes = np.asarray(deblock_ref.deblock(plain.reshape(-1), packed, p)).reshape(n, -1)
        for output, kind in ((None, "planes"), ((40, 40), "rgb_only"), (None, "jpeg")):
            want = _want_scores(s, planes, output, w, h)
            assert want != _want_scores(s, plain, output, w, h)
            rc, st, got = _decode(s, list(range(n)), output, kind, True, w, h, contexts=2, batch_pictures=2)
            assert rc == 1 and [got[k][3] for k in range(n)] == want, (output, kind)
