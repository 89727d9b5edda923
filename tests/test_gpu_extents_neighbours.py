"""GPU: the kernels beside reconstruction at the widest and tallest pictures (tests/test_gpu_extents.py has the reconstruction
forms): deblocking against tests/deblock_ref.py, the general resample kernel and the crop copy against tests/resample_ref.py,
and stream bytes -> front end -> compact pictures -> expand_compact_kernel -> engine against tests/compact.py and the oracle.

Run time of the references.  deblock_ref filters the macroblocks of one x + 2y together, so a picture one or two macroblocks
wide or high is walked nearly one macroblock per step: 6 .. 14 s per shape on the host, whatever the number of pictures; each
reference is computed once per session and the 600-picture case tiles the pictures of the 3-picture one.  resample_ref builds
dense tap matrices (16 384 x 16 384 for a column of 1024 macroblocks); _resample_in_blocks gives it the same rows in blocks."""
import functools

import numpy as np
import pytest

from minivideo_amd import Engine, HotPath, gen
from minivideo_amd.hotpath import STAGE_DEBLOCK, STREAM_DEBLOCK, geometry
from oracle import loader
from tests import deblock_ref as DR
from tests import resample_ref as RR
from tests.compact import COMPACT_MB_BYTES_MAX, COMPACT_SLACK_BYTES, decode_compact, expand
from tests.test_gpu_crop_copy import _run as _run_guarded
from tests.test_gpu_deblock import _expected, _params_of, _stage4, _stream, _synthetic
from tests.test_gpu_thumbnail import _planes
from tests.test_gpu_thumbnail import _run as _run_resample
from tests.util import Stream

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def torch_cuda():
    torch = pytest.importorskip("torch")
    assert torch.cuda.is_available(), "no HIP device"
    return torch


@pytest.fixture(scope="module")
def one():
    h = HotPath(0)
    yield h
    h.close()


# ---- deblocking ------------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _filtered(W, H):
    p, yuv, rec = _synthetic(W, H, 3, seed=W * 1000 + H + 3)
    want = DR.deblock(yuv, rec, p)
    assert not np.array_equal(want, yuv)
    return p, yuv, rec, want


@pytest.mark.parametrize("W,H", [(1, 1024), (2, 1024), (1024, 1)])
def test_stage4_at_the_extents(one, torch_cuda, W, H):
    p, yuv, rec, want = _filtered(W, H)
    got, _ = _stage4(torch_cuda, one, p, yuv, rec, 3)
    assert np.array_equal(got, want.reshape(-1))


def test_stage4_tall_pictures_four_waves(one, torch_cuda):
    """600 pictures of 2 x 1024 macroblocks: the four-wave variant (deblock_waves), 256 rows per wave; tiled on the device"""
    torch = torch_cuda
    p, yuv, rec, want = _filtered(2, 1024)
    n = 600
    d_packed = torch.from_numpy(rec.reshape(3, -1)).cuda().repeat(n // 3, 1).contiguous()
    d_yuv = torch.from_numpy(yuv.reshape(3, -1)).cuda().repeat(n // 3, 1).contiguous()
    torch.cuda.synchronize()
    one.recon_stages_dev(p, d_packed.data_ptr(), n, d_yuv.data_ptr(), None, None, STAGE_DEBLOCK)
    one.sync_check(None)
    for k in range(3):
        d_want = torch.from_numpy(want.reshape(3, -1)[k]).cuda()
        bad = torch.nonzero((d_yuv[k::3] != d_want).any(dim=1))
        assert bad.numel() == 0, "picture %d differs from deblock_ref" % (k + 3 * int(bad[0]))
    del d_packed, d_yuv
    torch.cuda.empty_cache()


@functools.lru_cache(maxsize=None)
def _deblocked_stream(W, H):
    stream, packed, _ = _stream("high", 3 * W + H, W, H, 2, slices=4, idc=(0, 1, 2))
    p = _params_of(stream, STREAM_DEBLOCK)
    return p, packed, _expected(p, packed, 2)


@pytest.mark.parametrize("W,H", [(1024, 2), (2, 1024)])
def test_generated_stream_reconstructed_and_deblocked(one, W, H):
    """four slices per picture, idc 0 / 1 / 2 and offsets -6 .. 6 per slice: reconstruction (automatic choice), the filter, colour"""
    p, packed, (wy, wr) = _deblocked_stream(W, H)
    yuv, rgb = one.recon_host(p, packed, 2, want_rgb=True)
    assert np.array_equal(yuv, wy) and np.array_equal(rgb, wr)


# ---- resample and crop copy --------------------------------------------------------------------------------------------------------
def _resample_in_blocks(yuv, W, H, g, block=1024):
    """resample_ref.resample of a geometry whose vertical ratio crop_h : out_h is 1 or 2, `block` cropped rows at a time (the
    geometry handed to it is the same with crop_y, crop_h and out_h of the block).  The blocks are exact: the vertical weights
    are W[j, i] = F(C(i + 1)) - F(C(i)) with C(i) = clamp(i D - j S, 0, S), F(c) = (c 2^14 + S / 2) / S; with S = k S', D = k D',
    i = b S' + i', j = b D' + j' one gets C = k C'(i') and, S' being even, F(C) = F'(C'), and C is constant (the weight 0) for i
    outside block b.  (block and block / 2, the chroma rows, are even; a last shorter block occurs only at ratio 1, where the
    weights are 2^14 on the diagonal for every S.)"""
    cx, cy, cw, ch, ow, oh = g
    r = ch // oh
    assert ch == r * oh and r in (1, 2) and block % 4 == 0 and (r == 1 or ch % block == 0)
    n = yuv.shape[0]
    Y, Cb, Cr = [], [], []
    for y0 in range(0, ch, block):
        bs = min(block, ch - y0)
        bd = bs // r
        out = RR.resample(yuv, W, H, (cx, cy + y0, cw, bs, ow, bd))
        q = (ow // 2) * (bd // 2)
        Y.append(out[:, :ow * bd])
        Cb.append(out[:, ow * bd:ow * bd + q])
        Cr.append(out[:, ow * bd + q:])
    return np.concatenate(Y + Cb + Cr, axis=1).reshape(n, -1)


def _geometries(W):
    Wp = 16 * W
    return {"identity": (0, 0, Wp, 16384, Wp, 16384),
            "crop": (2, 6, Wp - 4, 16370, Wp - 4, 16370),          # all four sides; chroma offsets 1 and 3
            "2:1": (0, 0, Wp, 16384, Wp // 2, 8192),
            "16384 -> 322": (0, 0, Wp, 16384, 2 * W, 322)}


@functools.lru_cache(maxsize=None)
def _resampled(W, kind):
    g = _geometries(W)[kind]
    yuv = _planes(W, 1024, 2, seed=W * 31 + len(kind))
    want = RR.resample(yuv, W, 1024, g) if kind == "16384 -> 322" else _resample_in_blocks(yuv, W, 1024, g)
    if g[4] == g[2] and g[5] == g[3]:      # crop only IS the rectangle of the coded planes
        Yp = yuv[:, :W * 1024 * 256].reshape(2, 16384, W * 16)
        assert np.array_equal(want[:, :g[2] * g[3]].reshape(2, g[3], g[2]), Yp[:, g[1]:g[1] + g[3], g[0]:g[0] + g[2]])
    return g, yuv, want, RR.to_rgb(want, g[4], g[5])


@pytest.mark.parametrize("planes,rgb", [(True, True), (True, False), (False, True)])
@pytest.mark.parametrize("kind", ["identity", "crop", "2:1", "16384 -> 322"])
@pytest.mark.parametrize("W", [1, 2])
def test_resample_columns_of_1024_macroblocks(one, torch_cuda, W, kind, planes, rgb):
    """16 384 rows of 16 and 32 samples.  Crop-only geometries run the copy kernel (output buffers at 16-, 4- and 8-byte offsets
    between sentinel bytes) and, with the setter, the general kernel; the others the general kernel."""
    g, yuv, want, want_rgb = _resampled(W, kind)
    geom = geometry(*g)
    if g[4] == g[2] and g[5] == g[3]:
        for guard in (64, 68, 72):
            got_y, got_r = _run_guarded(torch_cuda, one, W, 1024, yuv, geom, planes, rgb, guard)
            assert not planes or np.array_equal(got_y, want), guard
            assert not rgb or np.array_equal(got_r, want_rgb), guard
        one.set_crop_copy(False)
    try:
        got_y, got_r = _run_resample(torch_cuda, one, W, 1024, yuv, geom, planes, rgb)
    finally:
        one.set_crop_copy(True)
    assert not planes or np.array_equal(got_y, want)
    assert not rgb or np.array_equal(got_r, want_rgb)


# ---- stream bytes -> compact pictures -> records -> pictures -----------------------------------------------------------------------
@pytest.mark.parametrize("profile", ["baseline", "high"])        # CAVLC, CABAC with Intra8x8
@pytest.mark.parametrize("W,H", [(1024, 2), (2, 1024), (1, 1024)])
def test_whole_path_at_the_extents(torch_cuda, W, H, profile):
    """expand_compact_kernel with up to 2048 offset-table entries per picture, and the engine's buffers for shapes far from 16 : 9"""
    torch = torch_cuda
    F = 4
    stream, packed, _ = gen.make_stream_ex(W, H, F, seed=W + 7 * H, profile=profile)
    stride = (W * H * COMPACT_MB_BYTES_MAX + COMPACT_SLACK_BYTES + 15) & ~15
    host = np.zeros((F, stride), np.uint8)
    got = {}

    def sink(seq, idr, rc, err, pr, yuv, rgb):
        got[idr] = (rc, None if yuv is None else yuv.copy(), None if rgb is None else rgb.copy())
        return 1 if rc == 1 else 0

    with Stream(stream) as s:
        assert s.ok and s.idr_count == F, s.error()
        p = s.params(0)
        assert (p.width_mbs, p.height_mbs) == (W, H)
        for k in range(F):
            rc, used, buf = decode_compact(s, k)
            assert rc == 1 and used <= stride
            host[k, :used] = buf[:used]
            assert np.array_equal(expand(buf, W * H), packed[k]), k     # the front end's compact picture = the generator's records
        d_compact = torch.from_numpy(host).cuda()
        d_packed = torch.full((F * W * H * 800,), 0xEE, dtype=torch.uint8, device="cuda")
        torch.cuda.synchronize()
        hot = HotPath(0)
        try:
            hot.expand_compact_dev(p, d_compact.data_ptr(), stride, F, d_packed.data_ptr())
            hot.sync_check()
        finally:
            hot.close()
        records = d_packed.cpu().numpy().reshape(F, W * H, 800)
        for k in range(F):
            assert np.array_equal(records[k], expand(host[k], W * H)), k
        eng = Engine(contexts=1)
        try:
            rc, st = eng.decode(s.h, list(range(F)), want_rgb=True, sink=sink)
        finally:
            eng.close()
    assert rc == 1 and st["pictures_ok"] == F and st["pictures_failed"] == 0, st
    for k in range(F):
        ref_yuv, ref_rgb = loader.recon(p, packed[k], 1, want_rgb=True)
        assert got[k][0] == 1 and np.array_equal(got[k][1], ref_yuv) and np.array_equal(got[k][2], ref_rgb), k
