"""GPU: the opt-in deblocking filter (deblock.hip; MVHP_PARAM_DEBLOCK / MVHP_STAGE_DEBLOCK / MINIVIDEO_DEBLOCK=1) against the
NumPy restatement of clause 8.7 (tests/deblock_ref.py) on top of the oracle's reconstruction, byte for byte.  The reference
never deblocks; the tie to the reference-pinned output is that idc = 1 on every slice gives exactly the undeblocked pictures."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

from minivideo_amd import HotPath, gen, lib
from minivideo_amd.hotpath import (PARAM_DEBLOCK, STAGE_COLOR, STAGE_DEBLOCK, STAGE_RECON, STREAM_DEBLOCK, STREAM_SPEC,
                                   MiniVideoError, StreamParams)
from oracle import loader
from tests import deblock_ref as R
from tests.test_deblock import KAT, DStream, kat_planes

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CLI = os.path.join(ROOT, "minivideo_amd", "mini_thumbnailer")
STOCK = os.path.join(ROOT, "oracle", "_ref", "mini_thumbnailer_stock")
PROFILES = ("baseline", "main", "main_cavlc", "high", "high_cavlc", "high_4x4")


@pytest.fixture(scope="module")
def torch_cuda():
    torch = pytest.importorskip("torch")
    assert torch.cuda.is_available(), "no HIP device"
    return torch


def _with_flags(p, flags):
    q = StreamParams()
    C.memmove(C.byref(q), C.byref(p), C.sizeof(StreamParams))
    q.flags = flags
    return q


def _rgb_of(p, yuv):
    L = loader.lib()
    mbs = int(p.width_mbs) * int(p.height_mbs)
    yuv = np.ascontiguousarray(yuv, np.uint8).reshape(-1, mbs * 384)
    rgb = np.zeros((yuv.shape[0], mbs * 768), np.uint8)
    for f in range(yuv.shape[0]):
        L.orc_yuv_to_rgb(C.byref(p), yuv[f].ctypes.data, rgb[f].ctypes.data)
    return rgb.reshape(-1)


def _expected(p, packed, n, want_rgb=True):
    """oracle reconstruction -> deblock_ref -> the oracle's colour conversion"""
    yuv, _ = loader.recon(_with_flags(p, p.flags & ~PARAM_DEBLOCK), packed, n)
    yuv = R.deblock(yuv, packed, p)
    return yuv, (_rgb_of(p, yuv) if want_rgb else None)


def _stage4(torch, hot, p, yuv, rec, n, stages=STAGE_DEBLOCK, want_rgb=False):
    dev = torch.device("cuda", 0)
    d_packed = torch.from_numpy(np.ascontiguousarray(rec).reshape(-1)).to(dev)
    d_yuv = torch.from_numpy(np.ascontiguousarray(yuv).reshape(-1)).to(dev)
    d_rgb = torch.zeros(n * p.rgb_bytes, dtype=torch.uint8, device=dev) if want_rgb else None
    torch.cuda.synchronize(dev)
    hot.recon_stages_dev(p, d_packed.data_ptr(), n, d_yuv.data_ptr(), d_rgb.data_ptr() if want_rgb else None, None, stages)
    hot.sync_check(None)
    return d_yuv.cpu().numpy(), (d_rgb.cpu().numpy() if want_rgb else None)


@pytest.fixture(scope="module")
def one():
    h = HotPath(0)
    yield h
    h.close()


# ---- stage 4 alone on synthetic planes ----
@pytest.mark.parametrize("kw,luma,cb", KAT)
def test_stage4_known_answers(one, torch_cuda, kw, luma, cb):
    p, yuv, rec = kat_planes(**kw)
    got, _ = _stage4(torch_cuda, one, p, yuv, rec, 1)
    Y, Cb = got[:512].reshape(16, 32), got[512:640].reshape(8, 16)
    assert (Y == Y[0]).all() and list(Y[0, 12:20]) == luma and list(Cb[0, 6:10]) == cb
    assert np.array_equal(got, R.deblock(yuv, rec, p))


def _synthetic(W, H, n, seed):
    rng = np.random.default_rng(seed)
    p = StreamParams(W, H, int(rng.integers(-12, 13)), int(rng.integers(-12, 13)), PARAM_DEBLOCK)
    mbs = W * H
    rec = np.zeros((n, mbs, 800), np.uint8)
    rec[:, :, 0] = rng.integers(0, 4, (n, mbs))                    # I4x4 / I8x8 / I16x16 / I_PCM
    rec[:, :, 1] = rng.integers(0, 52, (n, mbs))
    rec[:, :, 5] = rng.choice([0, 0, 0, 1, 2], (n, mbs)) << 1
    rec[:, :, 6] = rng.integers(0, 16, (n, mbs))
    rec[:, :, 7] = (rng.integers(-6, 7, (n, mbs)) & 15) | ((rng.integers(-6, 7, (n, mbs)) & 15) << 4)
    # smooth planes (a level per 4x4 / 2x2 block) with small noise: every branch of the filter runs
    yuv = np.zeros((n, mbs * 384), np.int32)
    for base, pw, ph, blk in ((0, W * 16, H * 16, 4), (mbs * 256, W * 8, H * 8, 2), (mbs * 320, W * 8, H * 8, 2)):
        lv = rng.integers(40, 216, (n, ph // blk, pw // blk)) + rng.integers(-20, 21, (n, 1, 1))
        pl = np.repeat(np.repeat(lv, blk, 1), blk, 2) + rng.integers(-2, 3, (n, ph, pw))
        yuv[:, base:base + pw * ph] = pl.reshape(n, -1)
    return p, np.clip(yuv, 0, 255).astype(np.uint8), rec


@pytest.mark.parametrize("W,H,n", [(1, 1, 3), (2, 1, 3), (1, 2, 3), (7, 35, 3), (120, 68, 2), (240, 135, 1), (13, 9, 600)])
def test_stage4_random_planes(one, torch_cuda, W, H, n):
    p, yuv, rec = _synthetic(W, H, n, seed=W * 1000 + H + n)
    got, _ = _stage4(torch_cuda, one, p, yuv, rec, n)
    want = R.deblock(yuv, rec, p)
    assert not np.array_equal(want, yuv.reshape(-1)) or W * H == 1
    assert np.array_equal(got, want.reshape(-1))


def test_stage4_with_colour(one, torch_cuda):
    p, yuv, rec = _synthetic(9, 6, 4, seed=5)
    got, rgb = _stage4(torch_cuda, one, p, yuv, rec, 4, stages=STAGE_DEBLOCK | STAGE_COLOR, want_rgb=True)
    want = R.deblock(yuv, rec, p)
    assert np.array_equal(got, want.reshape(-1)) and np.array_equal(rgb, _rgb_of(p, want))


def test_too_wide_is_refused(one, torch_cuda):
    p, yuv, rec = _synthetic(2, 1, 1, seed=1)
    q = StreamParams(1025, 1, 0, 0, PARAM_DEBLOCK)
    with pytest.raises(MiniVideoError):
        one.recon_stages_dev(q, 1, 1, 1, None, None, STAGE_DEBLOCK)   # refused before anything is launched


def test_widest_picture(one, torch_cuda):
    """1024 macroblocks (the widest params_ok accepts): the line buffer still fits"""
    p, yuv, rec = _synthetic(1024, 2, 1, seed=2)
    got, _ = _stage4(torch_cuda, one, p, yuv, rec, 1)
    assert np.array_equal(got, R.deblock(yuv, rec, p).reshape(-1))


# ---- generator streams through every form ----
def _stream(profile, seed, W, H, n, slices=1, pcm=0, idc=(0, 1, 2), cqp=(0, 0), qp=(0, 51)):
    return gen.make_stream_ex(W, H, n, seed=seed, profile=profile, slices=slices, pcm_permille=pcm, cqp_offsets=cqp,
                              qp_range=qp, deblock=dict(idc=idc, offsets=(-6, 6)))


def _params_of(stream, flags):
    with DStream(stream, flags) as s:
        assert s.ok, s.error()
        return s.params(0)


@pytest.mark.parametrize("fused", [True, False])
@pytest.mark.parametrize("profile", PROFILES)
def test_generated_streams_every_form(hot, profile, fused):
    W, H, n = 11, 7, 3
    cqp = (5, -7) if profile.startswith("high") else (-12, 12)
    stream, packed, _ = _stream(profile, 40 + len(profile), W, H, n, cqp=cqp)
    p = _params_of(stream, STREAM_DEBLOCK)
    assert p.flags & PARAM_DEBLOCK
    hot.set_fused_color(fused)
    try:
        yuv, rgb = hot.recon_host(p, packed, n, want_rgb=True)
    finally:
        hot.set_fused_color(True)
    wy, wr = _expected(p, packed, n)
    assert np.array_equal(yuv, wy) and np.array_equal(rgb, wr)


@pytest.mark.parametrize("profile", PROFILES)
def test_generated_slices_and_pcm_spec_mode(hot, profile):
    W, H, n = 9, 6, 2
    stream, packed, _ = _stream(profile, 70 + len(profile), W, H, n, slices=4, pcm=80)
    p = _params_of(stream, STREAM_SPEC | STREAM_DEBLOCK)
    assert p.flags & PARAM_DEBLOCK and p.flags & 4
    yuv, rgb = hot.recon_host(p, packed, n, want_rgb=True)
    wy, wr = _expected(p, packed, n)
    assert np.array_equal(yuv, wy) and np.array_equal(rgb, wr)


@pytest.mark.parametrize("n", [1, 17, 300, 1100])
def test_batches_automatic_choice(one, n):
    distinct = 5
    stream, packed, _ = _stream("main", 90 + n, 10, 6, distinct)
    p = _params_of(stream, STREAM_DEBLOCK)
    idx = np.arange(n) % distinct
    yuv, rgb = one.recon_host(p, np.ascontiguousarray(packed[idx]), n, want_rgb=True)
    wy, wr = _expected(p, packed, distinct)
    wy, wr = wy.reshape(distinct, -1), wr.reshape(distinct, -1)
    yuv, rgb = yuv.reshape(n, -1), rgb.reshape(n, -1)
    for f in range(n):
        assert np.array_equal(yuv[f], wy[idx[f]]) and np.array_equal(rgb[f], wr[idx[f]]), f


def test_high_2160p_batch(one):
    stream, packed, _ = _stream("high", 7, 240, 135, 2, qp=(10, 45))
    p = _params_of(stream, STREAM_DEBLOCK)
    yuv, rgb = one.recon_host(p, packed, 2, want_rgb=True)
    wy, wr = _expected(p, packed, 2)
    assert np.array_equal(yuv, wy) and np.array_equal(rgb, wr)


@pytest.mark.parametrize("profile", ["baseline", "high"])
def test_idc1_everywhere_equals_no_deblocking(hot, profile):
    """disable_deblocking_filter_idc = 1 on every slice with deblocking on: the reference-pinned pictures, unchanged"""
    W, H, n = 12, 8, 3
    stream, packed, _ = _stream(profile, 5, W, H, n, idc=(1,), qp=(0, 51))
    p = _params_of(stream, STREAM_DEBLOCK)
    on = hot.recon_host(p, packed, n, want_rgb=True)
    off = hot.recon_host(_with_flags(p, p.flags & ~PARAM_DEBLOCK), packed, n, want_rgb=True)
    ref = loader.recon(_with_flags(p, p.flags & ~PARAM_DEBLOCK), packed, n, want_rgb=True)
    assert np.array_equal(on[0], off[0]) and np.array_equal(on[1], off[1])
    assert np.array_equal(on[0], ref[0]) and np.array_equal(on[1], ref[1])


def test_recon_stage_with_flag_deblocks(one, torch_cuda):
    """stage 1 under MVHP_PARAM_DEBLOCK = reconstruct, then filter; stage 1 without it = the unfiltered pictures"""
    stream, packed, _ = _stream("high", 12, 8, 5, 2)
    p = _params_of(stream, STREAM_DEBLOCK)
    blank = np.zeros(2 * p.yuv_bytes, np.uint8)
    got, _ = _stage4(torch_cuda, one, p, blank, packed, 2, stages=STAGE_RECON)
    assert np.array_equal(got, _expected(p, packed, 2, want_rgb=False)[0])
    q = _with_flags(p, p.flags & ~PARAM_DEBLOCK)
    got, _ = _stage4(torch_cuda, one, q, blank, packed, 2, stages=STAGE_RECON)
    assert np.array_equal(got, loader.recon(q, packed, 2)[0])


# ---- the engine and minivideo_decode ----
def test_engine_deblocks(one):
    from minivideo_amd import Engine
    stream, packed, _ = _stream("high", 21, 10, 6, 4)
    L = lib()
    h = C.c_void_p()
    L.mvhp_stream_open_ex.restype = C.c_int
    L.mvhp_stream_open_ex.argtypes = [C.c_void_p, C.c_size_t, C.c_uint32, C.POINTER(C.c_void_p)]
    assert L.mvhp_stream_open_ex(stream.ctypes.data, stream.size, STREAM_DEBLOCK, C.byref(h)) == 1
    got = {}

    def sink(seq, idr, rc, err, p, yuv, rgb):
        got[idr] = (rc, None if yuv is None else yuv.copy(), None if rgb is None else rgb.copy())
        return 1 if rc == 1 else 0

    eng = Engine(contexts=1)
    try:
        rc, st = eng.decode(h, [0, 1, 2, 3], want_rgb=True, sink=sink)
    finally:
        eng.close()
        L.mvhp_stream_close(h)
    assert rc == 1 and st["pictures_ok"] == 4
    p = _params_of(stream, STREAM_DEBLOCK)
    for k in range(4):
        wy, wr = _expected(p, packed[k], 1)
        assert got[k][0] == 1 and np.array_equal(got[k][1], wy) and np.array_equal(got[k][2], wr), k


def _cli(exe, tmp_path, data, name, fmt, n, deblock):
    path = tmp_path / name
    data.tofile(path)
    env = dict(os.environ)
    env.pop("MINIVIDEO_DEBLOCK", None)
    if deblock:
        env["MINIVIDEO_DEBLOCK"] = "1"
    args = [str(exe), "-i", str(path), "-f", fmt] + (["-n", str(n)] if n > 1 else [])
    r = subprocess.run(args, cwd=tmp_path, capture_output=True, text=True, timeout=120, env=env)
    assert r.returncode == 0 and "decode did not succeed" not in r.stderr, r.stderr


@pytest.mark.parametrize("container", ["es", "mp4"])
@pytest.mark.parametrize("fmt", ["yuv420", "bmp"])
@pytest.mark.parametrize("which", ["product", "stock"])
def test_cli_minivideo_deblock(tmp_path, container, fmt, which):
    from tests.mp4mux import mux
    from tests.test_gpu_api import _bmp
    exe = CLI if which == "product" else STOCK
    if which == "stock" and not os.path.exists(STOCK):
        pytest.skip("oracle/_ref/mini_thumbnailer_stock was not built")
    W, H, F = 12, 9, 3
    stream, packed, _ = _stream("high", 33, W, H, F, qp=(20, 44))
    data = stream if container == "es" else np.frombuffer(mux(stream, W * 16, H * 16), np.uint8)
    ext = "264" if container == "es" else "mp4"
    p = StreamParams(W, H, 0, 0, PARAM_DEBLOCK)
    for deblock in (True, False):
        d = tmp_path / ("on" if deblock else "off")
        d.mkdir()
        _cli(exe, d, data, "c." + ext, fmt, F, deblock)
        for k in range(F):
            if deblock:
                wy, wr = _expected(p, packed[k], 1)
            else:
                wy, wr = loader.recon(_with_flags(p, 0), packed[k], 1, want_rgb=True)
            if fmt == "bmp":
                assert (d / f"c_{k}.bmp").read_bytes() == _bmp(wr, W * 16, H * 16), (deblock, k)
            else:
                assert np.array_equal(np.fromfile(d / f"c_{k}.yuv", np.uint8), wy), (deblock, k)
