"""GPU: the orientation kernels (orient.hip behind mvhp_orient_dev) byte for byte against the NumPy restatement
(tests/orient_ref.py: np.rot90 per plane, RGB of the turned planes), at 0 to 3 quarter turns, planes only, RGB only and both,
from both source forms: the crop rectangle of coded pictures, and dense pictures as the resample pass leaves them."""
import functools

import numpy as np
import pytest

from minivideo_amd import HotPath
from minivideo_amd.hotpath import FAILURE, ORIENT_SRC_CODED, MiniVideoError, StreamParams, geometry, lib
from tests import orient_ref as O
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


def _run(torch, hot, W, H, src, geom, turns, planes, rgb, guard=64, coded=True):
    """-> (planes | None, RGB | None); the output buffers start `guard` bytes into allocations filled with 7, and the bytes
    before and behind the outputs must still be 7"""
    dev = torch.device("cuda", 0)
    n = src.shape[0]
    p = StreamParams(W, H, 0, 0, 0)
    d_src = torch.from_numpy(np.ascontiguousarray(src).reshape(-1)).to(dev)
    d_y = torch.full((n * geom.yuv_bytes + 2 * guard,), 7, dtype=torch.uint8, device=dev) if planes else None
    d_r = torch.full((n * geom.rgb_bytes + 2 * guard,), 7, dtype=torch.uint8, device=dev) if rgb else None
    torch.cuda.synchronize(dev)
    hot.orient_dev(p, geom, turns, d_src.data_ptr(), n, d_y.data_ptr() + guard if planes else None,
                   d_r.data_ptr() + guard if rgb else None, coded=coded)
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
def _source(W, H, n, g):
    """(coded pictures, the dense pictures of the rectangle): once per case"""
    yuv = _planes(W, H, n, seed=W * 31 + H * 7 + n + g[2])
    return yuv, O.crop(yuv, W, H, g)


@functools.lru_cache(maxsize=None)
def _want(W, H, n, g, turns):
    dense = _source(W, H, n, g)[1]
    t = O.turn(dense, g[2], g[3], turns)
    return t, O.to_rgb(t, g[2], g[3], turns)


CASES = [  # (W, H, n, (cx, cy, cw, ch))
    (1, 1, 1, (0, 0, 16, 16)),                    # one macroblock
    (1, 1, 1, (6, 10, 2, 2)),                     # ... and a 2 x 2 crop out of it
    (5, 3, 1, (2, 2, 78, 46)),                    # chroma 39 x 23: output rows start on odd bytes
    (9, 5, 1, (0, 0, 144, 80)),                   # whole tiles plus ragged ones on both axes
    (9, 5, 3, (0, 0, 144, 80)),
    (13, 9, 2, (10, 6, 190, 130)),                # odd chroma offsets on all four sides, sizes 2 mod 4
    (17, 11, 1, (6, 2, 262, 170)),                # three tiles across, two down, all ragged
    (7, 5, 300, (2, 2, 106, 74)),                 # many pictures: every alignment mod 16 occurs
    (1024, 1, 1, (0, 0, 16384, 16)),              # the widest picture ...
    (1, 1024, 1, (0, 0, 16, 16384)),              # ... and the tallest
]


@pytest.mark.parametrize("turns", [0, 1, 2, 3])
@pytest.mark.parametrize("W,H,n,g", CASES)
def test_orient_matches_reference(hot, torch_cuda, W, H, n, g, turns):
    yuv, dense = _source(W, H, n, g)
    want, want_rgb = _want(W, H, n, g, turns)
    geom = geometry(*g)
    for planes, rgb in ((True, True), (True, False), (False, True)):
        got_y, got_r = _run(torch_cuda, hot, W, H, yuv, geom, turns, planes, rgb)
        if planes:
            assert np.array_equal(got_y, want), (planes, rgb)
        if rgb:
            assert np.array_equal(got_r, want_rgb), (planes, rgb)
    # the dense source form on the same picture: what mvhp_resample_dev would have left
    dgeom = geometry(0, 0, g[2], g[3])
    den_y, den_r = _run(torch_cuda, hot, W, H, dense, dgeom, turns, True, True, coded=False)
    assert np.array_equal(den_y, want) and np.array_equal(den_r, want_rgb)


def test_zero_turns_is_the_crop():
    """the identity of the reference: zero turns of the restatement is the rectangle itself"""
    yuv, dense = _source(5, 3, 1, (2, 2, 78, 46))
    assert np.array_equal(O.turn(dense, 78, 46, 0), dense)


@pytest.mark.parametrize("turns", [1, 2, 3])
@pytest.mark.parametrize("guard", [68, 72, 80])
def test_output_phases(hot, torch_cuda, turns, guard):
    """output buffers at 4-, 8- and 16-byte phases, sentinel bytes around them"""
    W, H, n, g = 5, 3, 3, (2, 2, 78, 46)
    yuv, _ = _source(W, H, n, g)
    want, want_rgb = _want(W, H, n, g, turns)
    got_y, got_r = _run(torch_cuda, hot, W, H, yuv, geometry(*g), turns, True, True, guard=guard)
    assert np.array_equal(got_y, want) and np.array_equal(got_r, want_rgb)


def test_launch_split(hot, torch_cuda):
    """65 537 pictures of a 2 x 2 crop: more than one grid dimension holds, two launches"""
    n, g = 65537, (6, 10, 2, 2)
    yuv = np.random.default_rng(5).integers(0, 256, (n, 384), dtype=np.uint8)
    dense = O.crop(yuv, 1, 1, g)
    for turns in (1, 2):
        want = O.turn(dense, 2, 2, turns)
        got_y, got_r = _run(torch_cuda, hot, 1, 1, yuv, geometry(*g), turns, True, True)
        assert np.array_equal(got_y, want)
        assert np.array_equal(got_r, O.to_rgb(want, 2, 2, turns))


def test_four_quarter_turns_give_the_source_back(hot, torch_cuda):
    W, H, n, g = 9, 5, 2, (4, 2, 134, 70)
    yuv, dense = _source(W, H, n, g)
    cur, w, h = dense, g[2], g[3]
    for _ in range(4):
        cur, _ = _run(torch_cuda, hot, W, H, cur, geometry(0, 0, w, h), 1, True, False, coded=False)
        w, h = h, w
    assert np.array_equal(cur, dense)


def test_refused_arguments_launch_nothing(hot, torch_cuda):
    torch = torch_cuda
    dev = torch.device("cuda", 0)
    L = lib()
    p = StreamParams(2, 2, 0, 0, 0)
    d_src = torch.zeros(4 * 384, dtype=torch.uint8, device=dev)
    d_out = torch.full((4 * 384 * 2,), 7, dtype=torch.uint8, device=dev)
    torch.cuda.synchronize(dev)
    import ctypes as C

    def call(g, turns, n, flags=ORIENT_SRC_CODED, src=None, out=None):
        return L.mvhp_orient_dev(hot._h, C.byref(p), C.byref(g), turns, flags, src or d_src.data_ptr(), n,
                                 out or d_out.data_ptr(), None, None)

    ok = geometry(2, 2, 28, 28)
    assert call(ok, -1, 1) == FAILURE and call(ok, 4, 1) == FAILURE          # turns outside 0 .. 3
    assert call(ok, 1, -1) == FAILURE                                        # n < 0
    assert call(geometry(2, 2, 27, 28), 1, 1) == FAILURE                     # odd sizes
    assert call(geometry(1, 2, 28, 28), 1, 1) == FAILURE
    assert call(geometry(2, 2, 0, 28), 1, 1) == FAILURE                      # zero sizes
    assert call(geometry(2, 2, 28, 0), 1, 1) == FAILURE
    assert call(geometry(6, 2, 28, 28), 1, 1) == FAILURE                     # outside the coded picture
    assert call(geometry(2, 6, 28, 28), 1, 1) == FAILURE
    assert call(geometry(2, 2, 28, 28, 14, 14), 1, 1) == FAILURE             # a coded source is not scaled
    assert call(geometry(0, 0, 28, 28, 27, 28), 1, 1, flags=0) == FAILURE    # dense source: odd / zero sizes
    assert call(geometry(0, 0, 28, 28, 0, 28), 1, 1, flags=0) == FAILURE
    assert call(ok, 1, 1, flags=2) == FAILURE                                # unknown source flag
    assert call(ok, 1, 1, src=d_src.data_ptr() + 4) == FAILURE               # misaligned pointers
    assert call(ok, 1, 1, out=d_out.data_ptr() + 2) == FAILURE
    with pytest.raises(MiniVideoError):
        hot.orient_dev(p, ok, 5, d_src.data_ptr(), 1, d_out.data_ptr())
    assert call(ok, 1, 0) == 1                                               # n = 0 does nothing
    hot.sync_check(None)
    assert (d_out.cpu().numpy() == 7).all(), "a refused call wrote"
