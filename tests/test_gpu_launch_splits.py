"""GPU: the second launches of the output-side kernels, byte for byte against the NumPy restatements (tests/resample_ref.py,
tests/luma_ref.py): launch_resample and launch_crop_copy issue one launch per 65 535 pictures and launch_luma_stats one per
2^23 / bands pictures, each advancing its source and destination pointers.  Picture k of an input is base picture k modulo a
prime, so the reference is computed on the base pictures and tiled (tests/test_thumbnail.py and tests/test_blank.py check the
tiling against the direct reference), and a launch that starts again at picture 0, or at another picture's stride, differs."""
import functools
import time

import numpy as np
import pytest

from minivideo_amd import HotPath
from minivideo_amd.hotpath import StreamParams, geometry
from tests import luma_ref as L, resample_ref as R
from tests.test_gpu_luma_stats import GUARD, _launch, _random, _records
from tests.test_gpu_thumbnail import _planes

pytestmark = pytest.mark.gpu

GRID_Y = 65535                            # pictures per launch of resample_kernel / crop_copy_kernel
RESAMPLE_CYCLE = 263                      # prime
CROP = (2, 4, 12, 10)
MODES = {"crop_copy": (CROP, True), "resample": (CROP + (8, 6), True), "resample_1to1": (CROP, False)}   # (geometry, crop-copy switch)

STATS_RECT = (2, 0, 12, 16)               # 16 bands of one row under set_stats_band(1)
STATS_PER_LAUNCH = (1 << 23) // 16        # 524 288 pictures
STATS_CYCLE = 4099                        # prime


def tiled(base, n, cycle):
    """row k of the result is row k % cycle of `base`"""
    return base[np.arange(n) % cycle]


@functools.lru_cache(maxsize=None)
def resample_case(mode):
    """(263 base pictures of 1 x 1 macroblock, their expected planes, their expected RGB)"""
    g = MODES[mode][0]
    geom = geometry(*g)
    yuv = _planes(1, 1, RESAMPLE_CYCLE, seed=65537)
    want = R.resample(yuv, 1, 1, g[:4] + (geom.out_w, geom.out_h))
    return yuv, want, R.to_rgb(want, geom.out_w, geom.out_h)


@functools.lru_cache(maxsize=None)
def stats_case():
    """(4099 base pictures of 1 x 1 macroblock, their records as (4099, 32) bytes)"""
    yuv = _random(1, 1, STATS_CYCLE, 524289)
    return yuv, L.records(yuv, STATS_CYCLE, 1, 1, STATS_RECT).view(np.uint8).reshape(STATS_CYCLE, 32)


@pytest.fixture(scope="module")
def torch_cuda():
    torch = pytest.importorskip("torch")
    assert torch.cuda.is_available(), "no HIP device"
    return torch


@pytest.fixture(scope="module")
def hot():
    h = HotPath(0)
    yield h
    h.close()


@pytest.fixture(scope="module")
def d_pictures(torch_cuda):
    """65 537 pictures on the device: one buffer for every count and kernel"""
    yuv = tiled(resample_case("crop_copy")[0], GRID_Y + 2, RESAMPLE_CYCLE)
    return torch_cuda.from_numpy(np.ascontiguousarray(yuv).reshape(-1)).to(torch_cuda.device("cuda", 0))


@pytest.mark.parametrize("mode", list(MODES))
@pytest.mark.parametrize("n", [GRID_Y, GRID_Y + 1, GRID_Y + 2])
def test_resample_beyond_one_launch(hot, torch_cuda, d_pictures, n, mode):
    """input and output pictures differ in size (384 bytes in, 180 or 72 out), so a source and a destination advanced by each
    other's stride cannot cancel"""
    g, crop_copy = MODES[mode]
    geom = geometry(*g)
    _, want, want_rgb = resample_case(mode)
    assert want.shape[1] == geom.yuv_bytes != 384 and want_rgb.shape[1] == geom.rgb_bytes != 384
    dev = d_pictures.device
    d_y = torch_cuda.full((GUARD + n * geom.yuv_bytes + GUARD,), 7, dtype=torch_cuda.uint8, device=dev)
    d_r = torch_cuda.full((GUARD + n * geom.rgb_bytes + GUARD,), 7, dtype=torch_cuda.uint8, device=dev)
    torch_cuda.cuda.synchronize(dev)
    hot.set_crop_copy(crop_copy)
    try:
        hot.resample_dev(StreamParams(1, 1, 0, 0, 0), geom, d_pictures.data_ptr(), n, d_y.data_ptr() + GUARD, d_r.data_ptr() + GUARD, None)
        hot.sync_check(None)
    finally:
        hot.set_crop_copy(True)
    for d, ref, what in ((d_y, want, "planes"), (d_r, want_rgb, "RGB")):
        got = d.cpu().numpy()
        assert (got[:GUARD] == 7).all() and (got[-GUARD:] == 7).all(), "bytes outside the %s were written" % what
        got = got[GUARD:-GUARD].reshape(n, -1)
        bad = np.flatnonzero((got != tiled(ref, n, RESAMPLE_CYCLE)).any(axis=1))
        assert bad.size == 0, "%s: %d pictures differ, the first is picture %d" % (what, bad.size, bad[0])


def test_picture_scores_beyond_one_launch(hot, torch_cuda):
    """524 289 pictures of 16 one-row bands: one picture more than a launch of luma_stats_kernel holds -- the smallest input that
    reaches the second launch (201 MB of pictures, 16.8 MB of records, 8.4 M workgroups of one block each).  Measured on one
    MI355X: 12 ms from the call to the end of the second kernel (the printed figure), 0.09 s for the whole test."""
    n = STATS_PER_LAUNCH + 1
    base, base_rec = stats_case()
    d_src = torch_cuda.from_numpy(tiled(base, n, STATS_CYCLE).reshape(-1)).to(torch_cuda.device("cuda", 0))
    hot.set_stats_band(1)
    try:
        t0 = time.perf_counter()
        d = _launch(torch_cuda, hot, d_src, 1, 1, STATS_RECT, n)
        hot.sync_check(None)
        print("luma_stats of %d pictures x 16 bands: %.3f s" % (n, time.perf_counter() - t0))
    finally:
        hot.set_stats_band(0)
    got = _records(d, n).reshape(n, 32)
    bad = np.flatnonzero((got != tiled(base_rec, n, STATS_CYCLE)).any(axis=1))
    assert bad.size == 0, "%d records differ, the first is picture %d" % (bad.size, bad[0])
