"""GPU: the decode engine with a request that turns (Engine.decode(..., rotate=...) = MVHP_OUTPUT_ORIENT / MVHP_OUTPUT_ROTATE):
"auto" on MP4 files of each rotation, an explicit angle on Annex B, auto plus an angle that sum to 0; alone, with the crop, with a
box and with deblocking; planes, RGB, RGB only, JPEG and scores; 1 to 3 contexts and a re-queued batch.  Expected pictures: the
oracle's reconstruction of the generator's records (oracle/loader.py), tests/deblock_ref.py where deblocking is on,
tests/resample_ref.py with the geometry BEFORE the turn -- worked out here from the crop offsets and the box turned back, not by
the library -- then tests/orient_ref.py.  Byte for byte."""
import numpy as np
import pytest

from minivideo_amd import Engine, gen
from minivideo_amd.hotpath import PARAM_DEBLOCK, STREAM_DEBLOCK, StreamParams
from oracle import loader
from tests import deblock_ref as D
from tests import jpeg_ref as J
from tests import luma_ref as L
from tests import orient_ref as O
from tests import resample_ref as R
from tests.orient_streams import Mp4Stream, rotated_mp4
from tests.test_deblock import DStream

pytestmark = pytest.mark.gpu

W, H, F = 9, 7, 8
CROPS = [(1, 3, 2, 1), (1, 3, 2, 1), (1, 3, 2, 1), (0, 0, 0, 0), (5, 2, 7, 3), (5, 2, 7, 3), (0, 0, 0, 4), (0, 0, 0, 4)]
MP4_CROPS = [CROPS[0]] * F      # (tests/mp4mux.py writes the first SPS into avcC: every picture of the file carries its crop)
OUTPUTS = [None, "crop", (40, 24)]


@pytest.fixture(scope="module")
def clip():
    """(Annex-B bytes, records, oracle planes per picture, the same deblocked): computed once"""
    stream, packed = gen.make_stream_crop(W, H, F, CROPS, seed=41, profile="high", sps_pps_every_frame=True, qp_range=(20, 44))
    p = StreamParams(W, H, 0, 0, 1)
    yuv = loader.recon(p, packed, F)[0].reshape(F, -1)
    q = StreamParams(W, H, 0, 0, 1 | PARAM_DEBLOCK)
    dbk = np.stack([D.deblock(yuv[k], packed[k], q).reshape(-1) for k in range(F)])
    return stream, packed, yuv, dbk


def geom_before(crop, output, turns):
    """(cx, cy, cw, ch, ow, oh) before the turn: the box of an odd turn is applied turned back"""
    l, r, t, b = crop
    if output is None:
        return 0, 0, 16 * W, 16 * H, 16 * W, 16 * H
    cx, cy, cw, ch = 2 * l, 2 * t, 16 * W - 2 * (l + r), 16 * H - 2 * (t + b)
    if output == "crop":
        return cx, cy, cw, ch, cw, ch
    bw, bh = (output[1], output[0]) if turns & 1 else output
    return (cx, cy, cw, ch) + R.fit(cw, ch, bw, bh)


def expected(planes_k, crop, output, turns):
    """-> (delivered geometry, planes, RGB)"""
    g = geom_before(crop, output, turns)
    unturned = R.resample(planes_k, W, H, g)
    t = O.turn(unturned, g[4], g[5], turns)
    return g[:4] + O.turned_size(g[4], g[5], turns), t.reshape(-1), O.to_rgb(t, g[4], g[5], turns).reshape(-1)


def run(handle, order, **kw):
    got = {}

    def sink(seq, idr, rc, err, p, *rest):
        geom, yuv, rgb = rest if len(rest) == 3 else (None,) + rest      # (a call without any request: the plain sink)
        g = geom and (geom.crop_x, geom.crop_y, geom.crop_w, geom.crop_h, geom.out_w, geom.out_h)
        got[seq] = (idr, rc, err, g, None if yuv is None else yuv.copy(), None if rgb is None else rgb.copy(), geom and geom.score)
        return 1 if rc == 1 else 0

    opts = {k: kw.pop(k) for k in ("contexts", "fail_context") if k in kw}
    eng = Engine(chunk_pictures=2, batch_pictures=3, **opts)
    try:
        rc, st = eng.decode(handle, order, sink=sink, **kw)
    finally:
        eng.close()
    assert sorted(got) == list(range(len(order)))
    return rc, st, got


def check(got, st, order, planes, output, turns, want_rgb=1, crops=CROPS):
    d2h = 0
    for seq, k in enumerate(order):
        g, wy, wr = expected(planes[k], crops[k], output, turns)
        assert got[seq][0] == k and got[seq][1] == 1 and got[seq][3] == g, (seq, got[seq][:4], g)
        if want_rgb != 3:
            assert np.array_equal(got[seq][4], wy), seq
            d2h += wy.size
        else:
            assert got[seq][4] is None
        if want_rgb:
            assert np.array_equal(got[seq][5], wr), seq
            d2h += wr.size
    assert st["d2h_bytes"] == d2h      # the turned pictures only


@pytest.mark.parametrize("output", OUTPUTS)
@pytest.mark.parametrize("turns,contexts", [(0, 1), (1, 1), (2, 2), (3, 3), (1, 3)])
def test_auto_on_mp4(clip, turns, contexts, output):
    stream, _, planes, _ = clip
    order = list(range(F)) * 2
    with Mp4Stream(rotated_mp4(stream, 16 * W, 16 * H, turns, inband_params=False)) as s:
        assert s.ok and s.L.mvhp_stream_idr_count(s.h) == F
        rc, st, got = run(s.h, order, want_rgb=1, output=output, rotate="auto", contexts=contexts,
                          fail_context=0 if contexts == 3 else -1)
    assert rc == 1 and st["pictures_ok"] == len(order) and st["pictures_failed"] == 0, st
    assert st["batches_requeued"] == (1 if contexts == 3 else 0)
    check(got, st, order, planes, output, turns, crops=MP4_CROPS)
    if turns:
        assert st["geometry_launches"] == st["batches"]      # every batch of a call that turns has the pass
    elif output is None:
        assert st["geometry_launches"] == 0                   # zero turns: today's path


@pytest.mark.parametrize("want_rgb", [0, 1, 3])
@pytest.mark.parametrize("output", OUTPUTS)
@pytest.mark.parametrize("angle", [90, 180, 270])
def test_explicit_angle_on_annexb(clip, angle, output, want_rgb):
    stream, _, planes, _ = clip
    order = list(range(F))
    with DStream(stream, 0) as s:
        assert s.ok
        rc, st, got = run(s.h, order, want_rgb=want_rgb, output=output, rotate=angle, contexts=2)
    assert rc == 1 and st["pictures_ok"] == F, st
    check(got, st, order, planes, output, angle // 90, want_rgb)
    assert st["geometry_launches"] == st["batches"]


@pytest.mark.parametrize("output", OUTPUTS)
def test_auto_plus_angle_summing_to_zero(clip, output):
    """a 270-degree file, auto plus 90: the pictures, launches and bytes of the request without either"""
    stream, _, planes, _ = clip
    order = list(range(F))
    with Mp4Stream(rotated_mp4(stream, 16 * W, 16 * H, 3)) as s:
        rc, st, got = run(s.h, order, want_rgb=1, output=output, rotate=("auto", 90), contexts=1)
        rc0, st0, got0 = run(s.h, order, want_rgb=1, output=output, contexts=1)
    assert rc == rc0 == 1
    check(got, st, order, planes, output, 0, crops=MP4_CROPS)
    for seq in order:
        assert got0[seq][3] in (None, got[seq][3]) and np.array_equal(got[seq][4], got0[seq][4]) and np.array_equal(got[seq][5], got0[seq][5])
    assert (st["batches"], st["geometry_launches"], st["d2h_bytes"]) == (st0["batches"], st0["geometry_launches"], st0["d2h_bytes"])
    if output is None:
        assert st["geometry_launches"] == 0


@pytest.mark.parametrize("output", OUTPUTS)
def test_with_deblocking(clip, output):
    stream, _, planes, dbk = clip
    order = list(range(F))
    with DStream(stream, STREAM_DEBLOCK) as s:
        assert s.ok
        rc, st, got = run(s.h, order, want_rgb=1, output=output, rotate=90, contexts=2)
    assert rc == 1 and st["pictures_ok"] == F
    check(got, st, order, dbk, output, 1)
    assert not np.array_equal(dbk, planes)      # (the filter changed something: the case tests what it says)


# (a box large enough for every file to fit into its raw picture's bytes: the header alone is 625; what does not fit fails by design)
@pytest.mark.parametrize("output", [None, "crop", (64, 96)])
@pytest.mark.parametrize("angle", [90, 180])
def test_jpeg_of_the_turned_planes(clip, angle, output):
    stream, _, planes, _ = clip
    order = list(range(F))
    files = {}

    def sink(seq, idr, rc, err, p, g, yuv, data):
        assert yuv is None
        files[seq] = (rc, (g.out_w, g.out_h), None if data is None else data.tobytes())
        return 1 if rc == 1 else 0

    eng = Engine(contexts=2, chunk_pictures=2, batch_pictures=3)
    try:
        with DStream(stream, 0) as s:
            rc, st = eng.decode(s.h, order, sink=sink, output=output, jpeg=80, rotate=angle)
    finally:
        eng.close()
    assert rc == 1 and st["pictures_ok"] == F
    total = 0
    for k in order:
        g, wy, _ = expected(planes[k], CROPS[k], output, angle // 90)
        want = J.encode(wy, g[4], g[5], 80, None)
        assert files[k] == (1, (g[4], g[5]), want), k
        total += 16 + len(want)
    assert st["d2h_bytes"] == total


@pytest.mark.parametrize("output", OUTPUTS)
def test_scores_do_not_turn(clip, output):
    """the scores are those of the coded planes over the crop rectangle, with or without the turn"""
    stream, _, planes, _ = clip
    order = list(range(F))
    with DStream(stream, 0) as s:
        rc, st, got = run(s.h, order, want_rgb=0, output=output, rotate=270, score=True, contexts=2)
        rc0, st0, got0 = run(s.h, order, want_rgb=0, output=output, score=True, contexts=2)
    assert rc == rc0 == 1
    for k in order:
        g = geom_before(CROPS[k], output, 3)
        assert got[k][6] == got0[k][6] == L.picture_score(planes[k], W, H, g[:4]), k
        assert np.array_equal(got[k][4], expected(planes[k], CROPS[k], output, 3)[1])
    # the turned planes and 32 bytes of score record per picture (a box is applied to the turned picture: another size than unturned)
    assert st["d2h_bytes"] == sum(got[k][4].size + 32 for k in order)
    if output != OUTPUTS[2]:
        assert st["d2h_bytes"] == st0["d2h_bytes"]
