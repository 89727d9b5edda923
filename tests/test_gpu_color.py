"""GPU: the colour kernels (color_convert.hip behind mvhp_color_dev) byte for byte against the integer restatement
(tests/color_ref.py): both matrices, both ranges, the three chroma sitings; sizes from 2 x 2 to the widths and heights at which
the band of staged chroma rows shrinks; 1, 3 and 5 pictures; random planes and the extremes that reach every clamp; input and
output bases at every 4-byte phase of a 16-byte line inside guard bands that must come back untouched; a launch that splits;
every refusal."""
import ctypes as C
import functools

import numpy as np
import pytest

from minivideo_amd import HotPath
from minivideo_amd.hotpath import FAILURE, ColorParams, MiniVideoError, geometry, lib
from tests import color_ref as K
from tests import recon_buffers as B

pytestmark = pytest.mark.gpu

SETTINGS = [(m, f) for m in (K.BT601, K.BT709) for f in (0, 1)]
SITINGS = [K.NEAREST, K.LEFT, K.CENTER]
SIZES = [(2, 2), (4, 2), (2, 4), (6, 6), (14, 6), (18, 10), (34, 18), (62, 34), (130, 66), (258, 18), (4098, 4), (4, 2050)]


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


def _run(torch, hot, planes, w, h, setting, in_phase=0, out_phase=0):
    """planes (n x w*h*3/2) -> RGB (n x w*h*3).  Both buffers lie `phase` bytes behind a 256-byte boundary inside allocations filled
    with a sentinel (tests/recon_buffers.py); every byte of the output allocation outside the payload must still be the sentinel"""
    dev = torch.device("cuda", 0)
    n = planes.shape[0]
    yb, rb = w * h * 3 // 2, w * h * 3
    d_in = torch.full((B.alloc_bytes(yb, n),), B.SENTINEL, dtype=torch.uint8, device=dev)
    d_out = torch.full((B.alloc_bytes(rb, n),), B.SENTINEL, dtype=torch.uint8, device=dev)
    i0 = B.payload_start(d_in.data_ptr(), yb, in_phase)
    o0 = B.payload_start(d_out.data_ptr(), rb, out_phase)
    d_in[i0:i0 + n * yb] = torch.from_numpy(np.ascontiguousarray(planes).reshape(-1)).to(dev)
    torch.cuda.synchronize(dev)
    hot.color_dev(geometry(0, 0, w, h), setting, d_in.data_ptr() + i0, n, d_out.data_ptr() + o0)
    hot.sync_check(None)
    got = d_out.cpu().numpy()
    assert (got[:o0] == B.SENTINEL).all() and (got[o0 + n * rb:] == B.SENTINEL).all(), "bytes outside the output buffer were written"
    return got[o0:o0 + n * rb].reshape(n, rb)


@functools.lru_cache(maxsize=None)
def _planes(w, h, n):
    return np.random.default_rng(w * 131 + h * 17 + n).integers(0, 256, (n, w * h * 3 // 2), dtype=np.uint8)


@functools.lru_cache(maxsize=None)
def _want(w, h, n, matrix, full, siting):
    return K.to_rgb(_planes(w, h, n), w, h, matrix, full, siting)


@pytest.mark.parametrize("siting", SITINGS)
@pytest.mark.parametrize("w,h", SIZES)
def test_color_matches_reference(hot, torch_cuda, w, h, siting):
    for n in (1, 3, 5):
        for matrix, full in SETTINGS:
            got = _run(torch_cuda, hot, _planes(w, h, n), w, h, (matrix, full, siting))
            assert np.array_equal(got, _want(w, h, n, matrix, full, siting)), (n, matrix, full)


def _extremes(w, h):
    """all 0, all 255, luma 0 / 255 checkers over chroma 0 / 255 checkers in both phases, and black / white luma over each
    chroma corner: every clamp of every channel is reached"""
    q = (w // 2) * (h // 2)
    yy, xx = np.mgrid[0:h, 0:w]
    cy, cx = np.mgrid[0:h // 2, 0:w // 2]
    ychk = (((yy + xx) & 1) * 255).astype(np.uint8).reshape(-1)
    cchk = (((cy + cx) & 1) * 255).astype(np.uint8).reshape(-1)
    pics = [np.zeros(w * h + 2 * q, np.uint8), np.full(w * h + 2 * q, 255, np.uint8),
            np.concatenate([ychk, cchk, 255 - cchk]), np.concatenate([255 - ychk, 255 - cchk, cchk]), np.concatenate([ychk, cchk, cchk])]
    for yv in (0, 255):
        for cb in (0, 255):
            for cr in (0, 255):
                pics.append(np.concatenate([np.full(w * h, yv, np.uint8), np.full(q, cb, np.uint8), np.full(q, cr, np.uint8)]))
    return np.stack(pics)


@pytest.mark.parametrize("siting", SITINGS)
@pytest.mark.parametrize("w,h", [(6, 6), (34, 18), (62, 34)])
def test_extremes(hot, torch_cuda, w, h, siting):
    planes = _extremes(w, h)
    seen = set()
    for matrix, full in SETTINGS:
        want = K.to_rgb(planes, w, h, matrix, full, siting)
        got = _run(torch_cuda, hot, planes, w, h, (matrix, full, siting))
        assert np.array_equal(got, want), (matrix, full)
        seen |= {int(want.min()), int(want.max())}
    assert seen == {0, 255}


@pytest.mark.parametrize("siting", SITINGS)
@pytest.mark.parametrize("in_phase,out_phase", [(i, o) for i in (0, 4, 8, 12) for o in (0, 4, 8, 12)])
def test_buffer_phases(hot, torch_cuda, in_phase, out_phase, siting):
    """pictures of 270 and 540 bytes: picture k of a buffer lies at yet another phase"""
    w, h, n = 18, 10, 3
    got = _run(torch_cuda, hot, _planes(w, h, n), w, h, (K.BT709, 0, siting), in_phase, out_phase)
    assert np.array_equal(got, _want(w, h, n, K.BT709, 0, siting))


@pytest.mark.parametrize("siting", SITINGS)
def test_launch_split(hot, torch_cuda, siting):
    """65 537 pictures of 2 x 2: more than one grid dimension holds, two launches"""
    n = 65537
    planes = np.random.default_rng(5).integers(0, 256, (n, 6), dtype=np.uint8)
    got = _run(torch_cuda, hot, planes, 2, 2, (K.BT601, 1, siting))
    assert np.array_equal(got, K.to_rgb(planes, 2, 2, K.BT601, 1, siting))


def test_refused_arguments_launch_nothing(hot, torch_cuda):
    torch = torch_cuda
    dev = torch.device("cuda", 0)
    L = lib()
    d_src = torch.zeros(4096, dtype=torch.uint8, device=dev)
    d_out = torch.full((8192,), 7, dtype=torch.uint8, device=dev)
    torch.cuda.synchronize(dev)

    def call(g, params=(0, 0, 0, 0), n=1, src=None, out=None, ctx=True):
        cp = ColorParams(*params)
        return L.mvhp_color_dev(hot._h if ctx else None, C.byref(g) if g is not None else None, C.byref(cp) if params is not None else None,
                                d_src.data_ptr() if src is None else src, n, d_out.data_ptr() if out is None else out, None)

    ok = geometry(0, 0, 16, 16)
    assert call(ok, n=-1) == FAILURE                                          # n < 0
    for g in (geometry(0, 0, 15, 16), geometry(0, 0, 16, 15), geometry(0, 0, 0, 16), geometry(0, 0, 16, 0), geometry(0, 0, 16386, 2),
              geometry(0, 0, 2, 16386)):
        assert call(g) == FAILURE                                             # odd, zero and oversized sides
    for params in ((2, 0, 0, 0), (-1, 0, 0, 0), (0, 2, 0, 0), (0, -1, 0, 0), (0, 0, 3, 0), (0, 0, -1, 0), (0, 0, 0, 1)):
        assert call(ok, params) == FAILURE                                    # values the header does not name
    assert call(ok, src=d_src.data_ptr() + 2) == FAILURE                      # misaligned and missing pointers
    assert call(ok, out=d_out.data_ptr() + 2) == FAILURE
    assert call(ok, src=0) == FAILURE and call(ok, out=0) == FAILURE
    assert call(None) == FAILURE and call(ok, ctx=False) == FAILURE
    assert L.mvhp_color_dev(hot._h, C.byref(ok), None, d_src.data_ptr(), 1, d_out.data_ptr(), None) == FAILURE
    with pytest.raises(MiniVideoError):
        hot.color_dev(ok, (5, 0, 0), d_src.data_ptr(), 1, d_out.data_ptr())
    assert call(ok, n=0) == 1                                                 # n = 0 does nothing
    hot.sync_check(None)
    assert (d_out.cpu().numpy() == 7).all(), "a refused call wrote"
