"""GPU: the decode engine's PNG output kind (Engine.decode(..., png=True) = MVHP_OUT_PNG): pictures of the coded size (the fused
epilogue's RGB), cropped, boxed, turned, and cropped under the deblocking filter; 1 to 3 contexts and a re-queued batch; `wanted`,
scores, the exact download, and the refusals.  Expected files: the oracle's reconstruction of the generator's records ->
tests/deblock_ref.py -> tests/resample_ref.py -> tests/orient_ref.py -> the RGB of those planes -> tests/png_ref.py.  Byte for
byte."""
import ctypes as C

import numpy as np
import pytest

from minivideo_amd import Engine, gen
from minivideo_amd.hotpath import OUT_JPEG, OUT_PNG, PARAM_DEBLOCK, STREAM_DEBLOCK, StreamParams
from oracle import loader
from tests import deblock_ref as D
from tests import luma_ref as L
from tests import png_ref as P
from tests.test_deblock import DStream
from tests.test_gpu_engine_orient import CROPS, F, H, OUTPUTS, W, expected, geom_before

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def clip():
    """(Annex-B bytes, oracle planes per picture, the same deblocked): computed once"""
    stream, packed = gen.make_stream_crop(W, H, F, CROPS, seed=41, profile="high", sps_pps_every_frame=True, qp_range=(20, 44))
    yuv = loader.recon(StreamParams(W, H, 0, 0, 1), packed, F)[0].reshape(F, -1)
    q = StreamParams(W, H, 0, 0, 1 | PARAM_DEBLOCK)
    dbk = np.stack([D.deblock(yuv[k], packed[k], q).reshape(-1) for k in range(F)])
    return stream, yuv, dbk


def run(handle, order, **kw):
    files = {}

    def sink(seq, idr, rc, err, p, g, yuv, data):
        assert yuv is None
        files[seq] = (idr, rc, (g.out_w, g.out_h), None if data is None else data.tobytes(), g.score, err)
        return 1 if rc == 1 else 0

    opts = {k: kw.pop(k) for k in ("contexts", "fail_context") if k in kw}
    eng = Engine(chunk_pictures=2, batch_pictures=3, **opts)
    try:
        rc, st = eng.decode(handle, order, sink=sink, png=True, **kw)
    finally:
        eng.close()
    return rc, st, files


def want_file(planes_k, crop, output, turns):
    g, _, rgb = expected(planes_k, crop, output, turns)
    return (g[4], g[5]), P.encode(rgb, g[4], g[5])


@pytest.mark.parametrize("output", OUTPUTS)
@pytest.mark.parametrize("angle,contexts,deblock", [(None, 1, False), (None, 3, False), (90, 2, False), (180, 1, False), (None, 2, True)])
def test_files(clip, output, angle, contexts, deblock):
    stream, planes, dbk = clip
    order = list(range(F)) * 2
    with DStream(stream, STREAM_DEBLOCK if deblock else 0) as s:
        assert s.ok
        rc, st, files = run(s.h, order, output=output, rotate=angle, contexts=contexts, fail_context=0 if contexts == 3 else -1)
    assert rc == 1 and st["pictures_ok"] == len(order) and st["pictures_failed"] == 0, st
    assert st["batches_requeued"] == (1 if contexts == 3 else 0)
    assert sorted(files) == list(range(len(order)))
    total = 0
    for seq, k in enumerate(order):
        size, want = want_file((dbk if deblock else planes)[k], CROPS[k], output, (angle or 0) // 90)
        assert files[seq][:3] == (k, 1, size), (seq, files[seq][:3], files[seq][5])
        assert files[seq][3] == want, seq
        total += 16 + len(want)
    assert st["d2h_bytes"] == total                     # a table entry and exactly the file per picture
    if output is None and not angle:
        assert st["geometry_launches"] == 0            # the coded size: the fused epilogue's RGB, no pass in between
    if deblock:
        assert not np.array_equal(dbk, planes)


def test_wanted_and_scores(clip):
    stream, planes, _ = clip
    order = list(range(F))
    with DStream(stream, 0) as s:
        rc, st, files = run(s.h, order, wanted=3, output="crop", score=True, contexts=1)
        rc0, st0, files0 = run(s.h, order, wanted=3, output="crop", contexts=1)
    assert rc == rc0 == 1 and st["pictures_ok"] == 3 and sorted(files) == [0, 1, 2]
    for k in range(3):
        size, want = want_file(planes[k], CROPS[k], "crop", 0)
        assert files[k][2:4] == (size, want) and files0[k][3] == want
        assert files[k][4] == L.picture_score(planes[k], W, H, geom_before(CROPS[k], "crop", 0)[:4]) and files0[k][4] == 0
    assert st["d2h_bytes"] == st0["d2h_bytes"] + 32 * 3 == sum(16 + 32 + len(files[k][3]) for k in range(3))


def test_refusals(clip):
    """the plain sink cannot carry a file's length; PNG and JPEG are two kinds"""
    from minivideo_amd.hotpath import SINK_EX_T, SINK_T, DecodeStats
    stream, _, _ = clip
    eng = Engine(contexts=1, chunk_pictures=2, batch_pictures=3)
    try:
        with DStream(stream, 0) as s:
            order = (C.c_int * 2)(0, 1)
            st = DecodeStats()
            cb = SINK_T(lambda *a: 1)
            assert eng._L.mvhp_engine_decode(eng._h, s.h, order, 2, 2, OUT_PNG, cb, None, C.byref(st)) != 1
            assert eng._L.mvhp_engine_decode_ex(eng._h, s.h, order, 2, 2, OUT_PNG | OUT_JPEG, None, C.cast(None, SINK_EX_T), None, C.byref(st)) != 1
            with pytest.raises(ValueError):
                eng.decode(s.h, [0], png=True, jpeg=75)
            rc, st2 = eng.decode(s.h, [0, 1], png=True)     # (and the engine still works)
            assert rc == 1 and st2["pictures_ok"] == 2
    finally:
        eng.close()
