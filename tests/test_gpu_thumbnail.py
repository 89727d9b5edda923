"""GPU: the output-geometry pass (resample.hip, mvhp_resample_dev) byte for byte against the NumPy restatement
(tests/resample_ref.py): synthetic planes of every shape class, and generated cropped streams reconstructed on the device."""
import ctypes as C

import numpy as np
import pytest

from minivideo_amd import HotPath, gen
from minivideo_amd.hotpath import MiniVideoError, StreamParams, geometry, output_geometry
from oracle import loader
from tests import resample_ref as R
from tests.util import Stream

pytestmark = pytest.mark.gpu


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


def _planes(W, H, n, seed):
    """random coded pictures with runs of 0 and 255"""
    rng = np.random.default_rng(seed)
    yuv = rng.integers(0, 256, (n, W * H * 384), dtype=np.uint8)
    runs = rng.integers(0, yuv.shape[1], (n, 8))
    for f in range(n):
        for k, r in enumerate(runs[f]):
            yuv[f, r:r + 40] = 255 if k % 2 else 0
    return yuv


def _run(torch, hot, W, H, yuv, geom, planes=True, rgb=True):
    dev = torch.device("cuda", 0)
    n = yuv.shape[0]
    p = StreamParams(W, H, 0, 0, 0)
    d_src = torch.from_numpy(np.ascontiguousarray(yuv).reshape(-1)).to(dev)
    d_y = torch.full((n * geom.yuv_bytes,), 7, dtype=torch.uint8, device=dev) if planes else None
    d_r = torch.full((n * geom.rgb_bytes,), 7, dtype=torch.uint8, device=dev) if rgb else None
    torch.cuda.synchronize(dev)
    hot.resample_dev(p, geom, d_src.data_ptr(), n, d_y.data_ptr() if planes else None, d_r.data_ptr() if rgb else None, None)
    hot.sync_check(None)
    return (d_y.cpu().numpy().reshape(n, -1) if planes else None), (d_r.cpu().numpy().reshape(n, -1) if rgb else None)


def _check(torch, hot, W, H, n, g, seed, planes=True, rgb=True):
    yuv = _planes(W, H, n, seed)
    geom = geometry(*g)
    got_y, got_r = _run(torch, hot, W, H, yuv, geom, planes, rgb)
    want = R.resample(yuv, W, H, (g[0], g[1], g[2], g[3], geom.out_w, geom.out_h))
    if planes:
        assert np.array_equal(got_y, want)
    if rgb:
        assert np.array_equal(got_r, R.to_rgb(want, geom.out_w, geom.out_h))


CASES = [  # (W, H, n, (cx, cy, cw, ch, ow, oh))
    (1, 1, 1, (0, 0, 16, 16, 16, 16)),                # identity
    (1, 1, 3, (0, 0, 16, 16, 2, 2)),                  # 16 -> 2
    (2, 1, 7, (2, 4, 26, 10, 26, 10)),                # crop only, odd chroma offset (x / 2 = 1)
    (3, 2, 7, (6, 2, 40, 28, 20, 14)),                # 2:1, odd chroma halves (10 x 7)
    (4, 3, 5, (0, 0, 64, 48, 42, 32)),                # 3:2 vertically, irregular horizontally
    (13, 9, 2, (10, 6, 190, 130, 98, 66)),            # odd chroma offsets 5, 3
    (120, 68, 2, (0, 0, 1920, 1080, 320, 180)),       # 1080p cropped -> thumbnail
    (120, 68, 1, (0, 0, 1920, 1088, 322, 182)),       # 322 wide: rows of 2 mod 4 samples, chroma 161
    (120, 68, 1, (0, 8, 1920, 1080, 1920, 1080)),     # crop only at 1080p
    (240, 135, 1, (0, 0, 3840, 2160, 320, 180)),      # 2160p
    (7, 5, 300, (2, 2, 106, 74, 54, 38)),             # many pictures
]


@pytest.mark.parametrize("W,H,n,g", CASES)
def test_resample_planes_and_rgb(hot, torch_cuda, W, H, n, g):
    _check(torch_cuda, hot, W, H, n, g, seed=W * 31 + H + n)


@pytest.mark.parametrize("planes,rgb", [(True, False), (False, True)])
def test_resample_one_output(hot, torch_cuda, planes, rgb):
    _check(torch_cuda, hot, 9, 6, 4, (4, 2, 130, 88, 66, 44), seed=3, planes=planes, rgb=rgb)


def test_widest_picture(hot, torch_cuda):
    _check(torch_cuda, hot, 1024, 1, 1, (2, 0, 16380, 16, 16380, 16), seed=5)
    _check(torch_cuda, hot, 1024, 1, 1, (0, 0, 16384, 16, 322, 2), seed=6)


def test_geometry_outside_the_picture_is_refused(hot, torch_cuda):
    p = StreamParams(2, 2, 0, 0, 0)
    dev = torch_cuda.device("cuda", 0)
    # real buffers with room to spare: a regressed check would write wrong bytes here, never outside an allocation
    d_src = torch_cuda.zeros(4 * p.yuv_bytes, dtype=torch_cuda.uint8, device=dev)
    d_out = torch_cuda.full((4 * p.rgb_bytes,), 7, dtype=torch_cuda.uint8, device=dev)
    for g in ((2, 0, 32, 32, 32, 32), (0, 0, 32, 32, 34, 32), (1, 0, 30, 32, 30, 32), (0, 0, 32, 32, 0, 0)):
        with pytest.raises(MiniVideoError):
            hot.resample_dev(p, geometry(*g), d_src.data_ptr(), 1, d_out.data_ptr(), None, None)   # refused before any launch
    torch_cuda.cuda.synchronize(dev)
    assert (d_out.cpu().numpy() == 7).all()


@pytest.mark.parametrize("profile", ["baseline", "high"])
@pytest.mark.parametrize("output", ["crop", (40, 40)])
def test_generated_cropped_streams(hot, torch_cuda, profile, output):
    """generator streams whose SPS crop changes every picture: device reconstruction -> resample against the oracle ->
    resample_ref"""
    W, H, F = 9, 7, 4
    crops = [(0, 0, 0, 4), (1, 3, 2, 1), (0, 0, 0, 0), (5, 2, 7, 3)]
    stream, packed = gen.make_stream_crop(W, H, F, crops, seed=17, profile=profile, sps_pps_every_frame=True)
    dev = torch_cuda.device("cuda", 0)
    with Stream(stream) as s:
        assert s.ok
        p = s.params(0)
        yuv, _ = hot.recon_host(p, packed, F)
        assert np.array_equal(yuv, loader.recon(p, packed, F)[0])
        yuv = yuv.reshape(F, -1)
        for k in range(F):
            g = output_geometry(s.h, k, output)
            want = R.resample(yuv[k], W, H, (g.crop_x, g.crop_y, g.crop_w, g.crop_h, g.out_w, g.out_h))
            got_y, got_r = _run(torch_cuda, hot, W, H, yuv[k:k + 1], g)
            assert np.array_equal(got_y, want) and np.array_equal(got_r, R.to_rgb(want, g.out_w, g.out_h)), k
            if output == "crop":   # crop only: exactly the rectangle of the coded planes
                Y = yuv[k, :W * H * 256].reshape(H * 16, W * 16)
                assert np.array_equal(got_y[0, :g.out_w * g.out_h].reshape(g.out_h, g.out_w),
                                      Y[g.crop_y:g.crop_y + g.crop_h, g.crop_x:g.crop_x + g.crop_w])
    del dev
