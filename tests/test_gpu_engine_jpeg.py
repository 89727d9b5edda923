"""GPU: the decode engine with MVHP_OUT_JPEG (Engine.decode(..., jpeg=quality)): every delivered file equals the model's
(tests/jpeg_ref.py) of the expected picture -- oracle reconstruction, deblock_ref where the stream asks for it, resample_ref under
an output request -- with one to three contexts, a failed context re-queued, a stream whose crop changes, `wanted` capping, files
that do not fit, and d2h_bytes = table entries + delivered bytes."""
import numpy as np
import pytest

from minivideo_amd import Engine, gen
from minivideo_amd.hotpath import PARAM_DEBLOCK, STREAM_DEBLOCK, StreamParams, output_geometry
from oracle import loader
from tests import deblock_ref, jpeg_ref as J, resample_ref
from tests.test_deblock import DStream
from tests.util import Stream

pytestmark = pytest.mark.gpu

W, H = 9, 7
CROPS = [(0, 0, 0, 4), (0, 0, 0, 4), (1, 3, 2, 1), (0, 0, 0, 0), (0, 0, 0, 0), (5, 2, 7, 3), (1, 3, 2, 1), (1, 3, 2, 1)]
F = len(CROPS)


@pytest.fixture(scope="module")
def cropped():
    """(stream bytes, oracle planes per picture): computed once"""
    stream, packed = gen.make_stream_crop(W, H, F, CROPS, seed=29, profile="high", sps_pps_every_frame=True)
    yuv = loader.recon(StreamParams(W, H, 0, 0, 0), packed, F)[0].reshape(F, -1)
    return stream, yuv


def _expected(s, planes, output, quality, restart=None):
    files = []
    for k in range(planes.shape[0]):
        g = output_geometry(s.h, k, output)
        out = resample_ref.resample(planes[k], W, H, (g.crop_x, g.crop_y, g.crop_w, g.crop_h, g.out_w, g.out_h)).reshape(-1)
        files.append((J.encode(out, g.out_w, g.out_h, quality, restart), (g.out_w, g.out_h)))
    return files


def _decode(s, order, output, quality, wanted=None, restart=0, **opts):
    got = {}

    def sink(seq, idr, rc, err, p, g, yuv, data):
        assert yuv is None
        got[seq] = (rc, err, (g.out_w, g.out_h), None if data is None else data.tobytes())
        return 1 if rc == 1 else 0

    eng = Engine(**opts)
    try:
        rc, st = eng.decode(s.h, order, wanted=wanted, sink=sink, output=output, jpeg=quality, restart_mcus=restart)
    finally:
        eng.close()
    return rc, st, got


@pytest.mark.parametrize("contexts", [1, 2, 3])
@pytest.mark.parametrize("output", [None, "crop", (40, 40)])
def test_every_file_equals_the_model(cropped, contexts, output):
    stream, planes = cropped
    order = list(range(F)) * 2
    with Stream(stream) as s:
        assert s.ok
        want = _expected(s, planes, output, 75)
        opts = dict(contexts=contexts, batch_pictures=3, chunk_pictures=2, fail_context=0 if contexts == 3 else -1)
        rc, st, got = _decode(s, order, output, 75, **opts)
    assert rc == 1 and st["pictures_ok"] == len(order) and st["pictures_failed"] == 0
    assert st["batches_requeued"] == (1 if contexts == 3 else 0)
    for seq, idr in enumerate(order):
        assert got[seq] == (1, "", want[idr][1], want[idr][0]), seq
    assert st["d2h_bytes"] == sum(16 + len(want[idr][0]) for idr in order)
    if output is None:
        assert st["geometry_launches"] == 0


def test_quality_restart_and_wanted(cropped):
    stream, planes = cropped
    with Stream(stream) as s:
        want = _expected(s, planes, "crop", 93, restart=2)
        rc, st, got = _decode(s, list(range(F)), "crop", 93, wanted=3, restart=2, contexts=1, batch_pictures=2)
    assert rc == 1 and st["pictures_ok"] == 3 and sorted(got) == [0, 1, 2]
    for k in range(3):
        assert got[k][3] == want[k][0], k


def test_deblocked_stream():
    n = 4
    stream, packed, _ = gen.make_stream_ex(W, H, n, seed=23, profile="high", deblock=dict(idc=(0, 1, 2), offsets=(-6, 6)))
    with DStream(stream, STREAM_DEBLOCK) as s:
        assert s.ok
        p = s.params(0)
        assert p.flags & PARAM_DEBLOCK
        off = StreamParams.from_buffer_copy(p)
        off.flags = p.flags & ~PARAM_DEBLOCK
        planes = np.asarray(deblock_ref.deblock(loader.recon(off, packed, n)[0], packed, p)).reshape(n, -1)
        for output in (None, (40, 40)):
            want = _expected(s, planes, output, 75)
            rc, st, got = _decode(s, list(range(n)), output, 75, contexts=2, batch_pictures=2)
            assert rc == 1 and st["pictures_ok"] == n
            for k in range(n):
                assert got[k][3] == want[k][0], (output, k)


def test_files_that_do_not_fit(cropped):
    """a batch's blob has room for its raw pictures: a 16x12 thumbnail (288 bytes) is smaller than a JPEG header, so every
    picture fails with a message and decoding goes on; at 40x40 and quality 100, one picture per batch, exactly the files
    longer than the raw picture fail"""
    stream, planes = cropped
    with Stream(stream) as s:
        rc, st, got = _decode(s, list(range(F)), (16, 16), 75, contexts=2, batch_pictures=3)
        assert st["pictures_ok"] == 0 and st["pictures_failed"] == F and len(got) == F
        assert all(g[0] != 1 and "does not fit" in g[1] and g[3] is None for g in got.values())
        assert st["d2h_bytes"] == 16 * F
        want = _expected(s, planes, (40, 40), 100)
        rc, st, got = _decode(s, list(range(F)), (40, 40), 100, contexts=1, batch_pictures=1)
    delivered = 0
    for k in range(F):
        data, (w, h) = want[k]
        if len(data) <= w * h * 3 // 2:
            assert got[k][0] == 1 and got[k][3] == data, k
            delivered += 16 + len(data)
        else:
            assert got[k][0] != 1 and "does not fit" in got[k][1], k
            delivered += 16
    assert st["d2h_bytes"] == delivered
