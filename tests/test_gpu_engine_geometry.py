"""GPU: the decode engine with an output request (Engine.decode(output=...) = mvhp_engine_decode_ex): crop, box and crop +
deblocking; Baseline and High; 1 to 3 contexts; an injected device failure; RGB only; kept pictures; on generator streams with
one SPS crop throughout and with a crop that changes every picture.  Expected pictures: the oracle's reconstruction of the
generator's records (oracle/loader.py), tests/deblock_ref.py where deblocking is on, then tests/resample_ref.py -- with the
geometry worked out here from the crop offsets, not by the library.  Byte for byte."""
import ctypes as C

import numpy as np
import pytest

from minivideo_amd import Engine, gen
from minivideo_amd.hotpath import PARAM_DEBLOCK, STREAM_DEBLOCK, StreamParams
from oracle import loader
from tests import deblock_ref as D
from tests import resample_ref as R
from tests.test_deblock import DStream

pytestmark = pytest.mark.gpu

W, H = 9, 7
ONE = [(1, 3, 2, 1)]
CHANGING = [(0, 0, 0, 4), (1, 3, 2, 1), (0, 0, 0, 0), (5, 2, 7, 3), (1, 3, 2, 1), (1, 3, 2, 1)]


def geom_of(crop, output):
    """(cx, cy, cw, ch, ow, oh) of a W x H macroblock picture with SPS crop offsets (left, right, top, bottom)"""
    l, r, t, b = crop
    cx, cy, cw, ch = 2 * l, 2 * t, 16 * W - 2 * (l + r), 16 * H - 2 * (t + b)
    if output is None:
        return 0, 0, 16 * W, 16 * H, 16 * W, 16 * H
    ow, oh = (cw, ch) if output == "crop" else R.fit(cw, ch, *output)
    return cx, cy, cw, ch, ow, oh


def expected(p, packed_k, g, deblock=False):
    yuv, _ = loader.recon(p, packed_k, 1)
    if deblock:
        q = StreamParams(W, H, 0, 0, int(p.flags) | PARAM_DEBLOCK)
        yuv = D.deblock(yuv, packed_k, q)
    planes = R.resample(yuv, W, H, g)
    return planes.reshape(-1), R.to_rgb(planes, g[4], g[5]).reshape(-1)


def run(eng, stream, n, output, want_rgb=1, flags=0, keep=False):
    got, seqs = {}, []

    def sink(seq, idr, rc, err, p, geom, yuv, rgb):
        seqs.append(seq)
        g = (geom.crop_x, geom.crop_y, geom.crop_w, geom.crop_h, geom.out_w, geom.out_h)
        if rc != 1:
            got[seq] = (idr, rc, err, g, None, None)
            return 0
        if keep:   # the views stay valid until the release
            got[seq] = (idr, rc, err, g, yuv, rgb)
            return 2
        got[seq] = (idr, rc, err, g, None if yuv is None else yuv.copy(), None if rgb is None else rgb.copy())
        return 1

    with DStream(stream, flags) as s:
        assert s.ok and s.L.mvhp_stream_idr_count(s.h) == n
        rc, st = eng.decode(s.h, list(range(n)), want_rgb=want_rgb, sink=sink, output=output)
    assert seqs == list(range(len(seqs)))
    return rc, st, got


def d2h_expected(geoms, want_rgb):
    yuv = sum(g[4] * g[5] * 3 // 2 for g in geoms) if want_rgb != 3 else 0
    rgb = sum(g[4] * g[5] * 3 for g in geoms) if want_rgb else 0
    return yuv + rgb


@pytest.mark.parametrize("changing", [False, True])
@pytest.mark.parametrize("output", ["crop", (40, 40)])
@pytest.mark.parametrize("contexts", [1, 2, 3])
@pytest.mark.parametrize("profile", ["baseline", "high"])
def test_engine_geometry(profile, contexts, output, changing):
    F = 13
    crops = CHANGING if changing else ONE
    stream, packed = gen.make_stream_crop(W, H, F, crops, seed=31 + contexts, profile=profile, sps_pps_every_frame=changing)
    p = StreamParams(W, H, 0, 0, 1 if profile == "high" else 0)
    eng = Engine(contexts=contexts, chunk_pictures=2, batch_pictures=4)
    rc, st, got = run(eng, stream, F, output)
    eng.close()
    geoms = [geom_of(crops[k % len(crops)], output) for k in range(F)]
    assert rc == 1 and st["pictures_ok"] == F and st["pictures_failed"] == 0, st
    for k in range(F):
        wy, wr = expected(p, packed[k], geoms[k])
        assert got[k][0] == k and got[k][3] == geoms[k], (k, got[k][3], geoms[k])
        assert np.array_equal(got[k][4], wy) and np.array_equal(got[k][5], wr), k
    assert st["d2h_bytes"] == d2h_expected(geoms, 1)
    coded = (0, 0, 16 * W, 16 * H, 16 * W, 16 * H)
    runs = sum(1 for k in range(F) if k == 0 or geoms[k] != geoms[k - 1])
    geom_runs = sum(1 for k in range(F) if (k == 0 or geoms[k] != geoms[k - 1]) and geoms[k] != coded)
    if changing and contexts == 1:
        # one batch per run of equal geometry (no run is longer than a batch); the uncropped picture under "crop" is of the
        # coded size: the plain path.  (Several contexts share out the last pictures one by one: a run may split there.)
        assert st["batches"] == runs and st["geometry_launches"] == geom_runs, st
    elif changing:
        assert st["batches"] >= runs and geom_runs <= st["geometry_launches"] <= st["batches"] - (runs - geom_runs), st
    else:
        assert st["batches"] == st["geometry_launches"] >= (F + 3) // 4, st


@pytest.mark.parametrize("output", ["crop", (40, 40)])
@pytest.mark.parametrize("profile", ["baseline", "high"])
def test_engine_geometry_with_deblocking(profile, output):
    F = 6
    stream, packed = gen.make_stream_crop(W, H, F, CHANGING, seed=5, profile=profile, sps_pps_every_frame=True, qp_range=(20, 44))
    p = StreamParams(W, H, 0, 0, 1 if profile == "high" else 0)
    eng = Engine(contexts=2, chunk_pictures=2, batch_pictures=4)
    rc, st, got = run(eng, stream, F, output, flags=STREAM_DEBLOCK)
    eng.close()
    assert rc == 1 and st["pictures_ok"] == F
    differs = 0
    for k in range(F):
        g = geom_of(CHANGING[k], output)
        wy, wr = expected(p, packed[k], g, deblock=True)
        assert got[k][3] == g and np.array_equal(got[k][4], wy) and np.array_equal(got[k][5], wr), k
        differs += not np.array_equal(wy, expected(p, packed[k], g)[0])
    assert differs > 0   # (the filter changed something: the case tests what it says)


def test_engine_geometry_requeues_a_failed_batch():
    F = 24
    stream, packed = gen.make_stream_crop(W, H, F, CHANGING, seed=8, profile="high", sps_pps_every_frame=True)
    p = StreamParams(W, H, 0, 0, 1)
    eng = Engine(contexts=3, chunk_pictures=2, batch_pictures=4, fail_context=0)
    rc, st, got = run(eng, stream, F, (40, 40))
    eng.close()
    assert rc == 1 and st["batches_requeued"] == 1 and st["pictures_ok"] == F and st["pictures_issued"] > F, st
    geoms = [geom_of(CHANGING[k % len(CHANGING)], (40, 40)) for k in range(F)]
    for k in range(F):
        wy, wr = expected(p, packed[k], geoms[k])
        assert got[k][3] == geoms[k] and np.array_equal(got[k][4], wy) and np.array_equal(got[k][5], wr), k
    assert st["d2h_bytes"] == d2h_expected(geoms, 1)   # (the failed launch downloaded nothing)


def test_engine_geometry_single_context_failure_is_reported():
    F = 12
    stream, _ = gen.make_stream_crop(W, H, F, ONE, seed=9, profile="baseline")
    eng = Engine(contexts=1, chunk_pictures=2, batch_pictures=4, fail_context=0)
    rc, st, got = run(eng, stream, F, "crop")
    eng.close()
    g = geom_of(ONE[0], "crop")
    assert rc == 1 and st["pictures_failed"] == 4 and st["pictures_ok"] == F - 4
    assert all(got[k][1] != 1 and "injected" in got[k][2] for k in range(4))
    assert st["d2h_bytes"] == d2h_expected([g] * (F - 4), 1)


@pytest.mark.parametrize("output", ["crop", (40, 40)])
def test_engine_geometry_rgb_only_and_planes_only(output):
    F = 7
    stream, packed = gen.make_stream_crop(W, H, F, CHANGING, seed=12, profile="baseline", sps_pps_every_frame=True)
    p = StreamParams(W, H, 0, 0, 0)
    geoms = [geom_of(CHANGING[k % len(CHANGING)], output) for k in range(F)]
    eng = Engine(contexts=2, chunk_pictures=2, batch_pictures=4)
    for want_rgb in (3, 0):
        rc, st, got = run(eng, stream, F, output, want_rgb=want_rgb)
        assert rc == 1 and st["pictures_ok"] == F
        for k in range(F):
            wy, wr = expected(p, packed[k], geoms[k])
            if want_rgb == 3:
                assert got[k][4] is None and np.array_equal(got[k][5], wr), k
            else:
                assert got[k][5] is None and np.array_equal(got[k][4], wy), k
        assert st["d2h_bytes"] == d2h_expected(geoms, want_rgb)
    eng.close()


def test_engine_geometry_kept_pictures():
    """the sink keeps every picture (verdict 2); another thread compares and releases them while the call is still running"""
    import queue
    import threading
    F = 30
    stream, packed = gen.make_stream_crop(W, H, F, CHANGING, seed=14, profile="baseline", sps_pps_every_frame=True)
    p = StreamParams(W, H, 0, 0, 0)
    geoms = [geom_of(CHANGING[k % len(CHANGING)], (40, 40)) for k in range(F)]
    eng = Engine(contexts=2, chunk_pictures=2, batch_pictures=4)
    q, bad, released = queue.Queue(), [], []

    def sink(seq, idr, rc, err, pr, geom, yuv, rgb):
        if rc != 1:
            bad.append(seq)
            return 0
        q.put((seq, yuv, rgb))
        return 2

    def releaser():
        while True:
            item = q.get()
            if item is None:
                return
            seq, yuv, rgb = item
            wy, wr = expected(p, packed[seq], geoms[seq])
            if not (np.array_equal(yuv, wy) and np.array_equal(rgb, wr)):
                bad.append(seq)
            released.append(seq)
            eng.release_picture(seq)

    t = threading.Thread(target=releaser)
    t.start()
    with DStream(stream, 0) as s:
        rc, st = eng.decode(s.h, list(range(F)), want_rgb=1, sink=sink, output=(40, 40))
    n_released_at_return = len(released)
    q.put(None)
    t.join()
    eng.close()
    assert rc == 1 and st["pictures_ok"] == F and not bad
    assert n_released_at_return == F   # the call does not return before the last kept picture is back


def test_engine_coded_size_takes_the_plain_path():
    """an uncropped stream with "crop", or with a box that already contains the picture: geometry_launches = 0 and the pictures
    mvhp_engine_decode delivers; with a smaller box it is resampled"""
    F = 9
    stream, packed = gen.make_stream(W, H, F, seed=21, profile="high")
    p = StreamParams(W, H, 0, 0, 1)
    coded = (0, 0, 16 * W, 16 * H, 16 * W, 16 * H)
    eng = Engine(contexts=2, chunk_pictures=2, batch_pictures=4)
    plain = {}

    def sink(seq, idr, rc, err, pr, yuv, rgb):
        plain[seq] = (yuv.copy(), rgb.copy())
        return 1

    with DStream(stream, 0) as s:
        rc, st0 = eng.decode(s.h, list(range(F)), want_rgb=1, sink=sink)
    assert rc == 1 and st0["geometry_launches"] == 0
    for output in ("crop", (16 * W, 16 * H), (4096, 4096)):
        rc, st, got = run(eng, stream, F, output)
        assert rc == 1 and st["geometry_launches"] == 0 and st["batches"] == st0["batches"], st
        assert st["d2h_bytes"] == st0["d2h_bytes"] == F * (p.yuv_bytes + p.rgb_bytes)
        for k in range(F):
            ref_yuv, ref_rgb = loader.recon(p, packed[k], 1, want_rgb=True)
            assert got[k][3] == coded
            assert np.array_equal(got[k][4], plain[k][0]) and np.array_equal(got[k][5], plain[k][1]), k
            assert np.array_equal(got[k][4], ref_yuv) and np.array_equal(got[k][5], ref_rgb), k
    rc, st, got = run(eng, stream, F, (40, 40))
    eng.close()
    g = geom_of((0, 0, 0, 0), (40, 40))
    assert rc == 1 and st["geometry_launches"] == st["batches"] > 0
    for k in range(F):
        wy, wr = expected(p, packed[k], g)
        assert got[k][3] == g and np.array_equal(got[k][4], wy) and np.array_equal(got[k][5], wr), k


def test_engine_crop_that_leaves_nothing_fails_in_place():
    F = 6
    crops = [(1, 3, 2, 1), (40, 40, 0, 0), (1, 3, 2, 1), (1, 3, 2, 1), (0, 0, 30, 30), (0, 0, 0, 4)]
    stream, packed = gen.make_stream_crop(W, H, F, crops, seed=4, profile="baseline", sps_pps_every_frame=True)
    p = StreamParams(W, H, 0, 0, 0)
    eng = Engine(contexts=2, chunk_pictures=2, batch_pictures=4)
    rc, st, got = run(eng, stream, F, "crop")
    eng.close()
    assert rc == 1 and st["pictures_ok"] == 4 and st["pictures_failed"] == 2
    for k in range(F):
        if k in (1, 4):
            assert got[k][1] != 1 and "leaves no picture" in got[k][2], got[k][:3]
            continue
        g = geom_of(crops[k], "crop")
        wy, wr = expected(p, packed[k], g)
        assert got[k][3] == g and np.array_equal(got[k][4], wy) and np.array_equal(got[k][5], wr), k


def test_engine_geometry_beside_a_placed_arena(monkeypatch):
    """Engine(placed=True): the four batch buffers are pieces of one placed arena, the output pictures of a geometry batch are
    ordinary allocations beside it -- also after a batch buffer has left the arena for a batch it was not sized for (the
    second job's batches are larger than the arena's)"""
    monkeypatch.setenv("MVHP_PLACED_ARENA_GB", "48")   # (as tests/test_gpu_placement.py: no 200-GB arena in a test)
    p = StreamParams(W, H, 0, 0, 0)
    eng = Engine(contexts=1, chunk_pictures=2, batch_pictures=8, placed=True)
    for F, seed, output in ((4, 41, (40, 40)), (19, 42, "crop"), (19, 43, (40, 40))):
        stream, packed = gen.make_stream_crop(W, H, F, CHANGING, seed=seed, profile="baseline", sps_pps_every_frame=True)
        rc, st, got = run(eng, stream, F, output)
        geoms = [geom_of(CHANGING[k % len(CHANGING)], output) for k in range(F)]
        assert rc == 1 and st["pictures_ok"] == F and st["geometry_launches"] > 0, st
        assert st["d2h_bytes"] == d2h_expected(geoms, 1)
        for k in range(F):
            wy, wr = expected(p, packed[k], geoms[k])
            assert got[k][3] == geoms[k] and np.array_equal(got[k][4], wy) and np.array_equal(got[k][5], wr), (F, k)
    # one run of equal geometry longer than the arena's four pictures: the batch buffer leaves the arena
    stream, packed = gen.make_stream_crop(W, H, 16, ONE, seed=44, profile="baseline")
    rc, st, got = run(eng, stream, 16, "crop")
    eng.close()
    g = geom_of(ONE[0], "crop")
    assert rc == 1 and st["pictures_ok"] == 16 and st["max_batch_pictures"] == 8, st
    for k in range(16):
        wy, wr = expected(p, packed[k], g)
        assert got[k][3] == g and np.array_equal(got[k][4], wy) and np.array_equal(got[k][5], wr), k
