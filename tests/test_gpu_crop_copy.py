"""GPU: the crop-only copy kernel (crop_copy.hip, what mvhp_resample_dev runs for out_w == crop_w and out_h == crop_h) byte for
byte against the NumPy restatement (tests/resample_ref.py: D = S is an exact copy, RGB from the cropped planes with 2x2-nearest
chroma), and against the general resample kernel on the same inputs (mvhp_set_crop_copy(ctx, 0)).  Planes only, RGB only and
both; output buffers at 16-, 4- and 8-byte offsets with sentinel bytes around them.

A crop wider than the general kernel's LDS limit cannot be formed: one band needs 5 bytes of LDS per cropped column and the
device has 160 KiB, i.e. 32768 columns, while a coded picture is at most 1024 macroblocks = 16384 samples wide.  The widest
crop there is (16380 of 16384) is a case below."""
import functools

import numpy as np
import pytest

from minivideo_amd import HotPath
from minivideo_amd.hotpath import StreamParams, geometry
from tests import resample_ref as R
from tests.test_gpu_thumbnail import _planes

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


def _run(torch, hot, W, H, yuv, geom, planes, rgb, guard):
    """-> (planes | None, RGB | None); the output buffers start `guard` bytes into allocations filled with 7, and the bytes
    before and behind the outputs must still be 7"""
    dev = torch.device("cuda", 0)
    n = yuv.shape[0]
    p = StreamParams(W, H, 0, 0, 0)
    d_src = torch.from_numpy(np.ascontiguousarray(yuv).reshape(-1)).to(dev)
    d_y = torch.full((n * geom.yuv_bytes + 2 * guard,), 7, dtype=torch.uint8, device=dev) if planes else None
    d_r = torch.full((n * geom.rgb_bytes + 2 * guard,), 7, dtype=torch.uint8, device=dev) if rgb else None
    torch.cuda.synchronize(dev)
    hot.resample_dev(p, geom, d_src.data_ptr(), n, d_y.data_ptr() + guard if planes else None,
                     d_r.data_ptr() + guard if rgb else None, None)
    hot.sync_check(None)
    out = []
    for d in (d_y, d_r):
        if d is None:
            out.append(None)
            continue
        h = d.cpu().numpy()
        assert (h[:guard] == 7).all() and (h[-guard:] == 7).all(), "bytes outside the output buffer were written"
        out.append(h[guard:-guard].reshape(n, -1))
    return out


@functools.lru_cache(maxsize=None)
def _case(W, H, n, g):
    """(coded pictures, expected planes, expected RGB) of a case: the NumPy restatement, once for the three output modes"""
    yuv = _planes(W, H, n, seed=W * 31 + H * 7 + n + g[2])
    want = R.resample(yuv, W, H, (g[0], g[1], g[2], g[3], g[2], g[3]))
    return yuv, want, R.to_rgb(want, g[2], g[3])


CASES = [  # (W, H, n, (cx, cy, cw, ch))
    (1, 1, 1, (0, 0, 16, 16)),                    # one macroblock, nothing cropped
    (1, 1, 1, (2, 4, 12, 10)),                    # ... cropped on all four sides; chroma 6 wide, offset 1
    (2, 2, 3, (6, 2, 2, 28)),                     # crop_w = 2: chroma rows of one byte, odd chroma offset 3
    (2, 1, 7, (2, 4, 26, 10)),                    # crop_w = 2 mod 4 (and 10 mod 16), odd chroma offset
    (2, 1, 5, (4, 0, 18, 16)),                    # crop_w = 2 mod 16
    (13, 9, 2, (10, 6, 190, 130)),                # all four sides, odd chroma offsets 5 and 3, crop_w = 2 mod 4
    (13, 9, 2, (4, 2, 178, 140)),                 # crop_w = 2 mod 16, chroma 89 wide
    (1024, 1, 1, (2, 0, 16380, 16)),              # the widest picture (test_gpu_thumbnail.test_widest_picture)
    (120, 68, 2, (0, 0, 1920, 1080)),             # 1080p: the eight rows of padding go
    (120, 68, 1, (0, 8, 1920, 1080)),
    (120, 68, 1, (6, 2, 1906, 1084)),             # 1080p at a 2-mod-4 source offset, rows of 2 mod 16
    (240, 135, 1, (2, 6, 3830, 2150)),            # 2160p
    (7, 5, 300, (2, 2, 106, 74)),                 # many pictures; picture stride 11766 bytes: every alignment mod 16 occurs
]


@pytest.mark.parametrize("planes,rgb", [(True, True), (True, False), (False, True)])
@pytest.mark.parametrize("W,H,n,g", CASES)
def test_crop_copy_matches_reference_and_general_kernel(hot, torch_cuda, W, H, n, g, planes, rgb):
    yuv, want, want_rgb = _case(W, H, n, g)
    geom = geometry(*g)
    # the restatement of crop only IS the rectangle of the coded planes
    Y = yuv[:, :W * H * 256].reshape(n, H * 16, W * 16)
    assert np.array_equal(want[:, :g[2] * g[3]].reshape(n, g[3], g[2]), Y[:, g[1]:g[1] + g[3], g[0]:g[0] + g[2]])
    for guard in (64, 68, 72):
        got_y, got_r = _run(torch_cuda, hot, W, H, yuv, geom, planes, rgb, guard)
        if planes:
            assert np.array_equal(got_y, want), guard
        if rgb:
            assert np.array_equal(got_r, want_rgb), guard
    hot.set_crop_copy(False)   # the general kernel on the same inputs
    try:
        gen_y, gen_r = _run(torch_cuda, hot, W, H, yuv, geom, planes, rgb, 64)
    finally:
        hot.set_crop_copy(True)
    if planes:
        assert np.array_equal(gen_y, got_y)
    if rgb:
        assert np.array_equal(gen_r, got_r)


def test_setter_changes_the_kernel_not_the_result(hot, torch_cuda):
    """a downscaling geometry runs the general kernel whatever the setter says"""
    yuv = _planes(9, 6, 4, seed=3)
    geom = geometry(4, 2, 130, 88, 66, 44)
    want = R.resample(yuv, 9, 6, (4, 2, 130, 88, 66, 44))
    for on in (True, False):
        hot.set_crop_copy(on)
        try:
            got_y, got_r = _run(torch_cuda, hot, 9, 6, yuv, geom, True, True, 64)
        finally:
            hot.set_crop_copy(True)
        assert np.array_equal(got_y, want) and np.array_equal(got_r, R.to_rgb(want, 66, 44))
