"""GPU: the caller buffers of the reconstruction entry points -- mvhp_recon_batch_dev, mvhp_recon_stages_dev and
mvhp_expand_compact_dev -- behind guard bands and at every alignment phase the contract allows (MVHP_RECON_ALIGN,
include/minivideo_hotpath.h; DESIGN.md 5 "Caller buffers of the reconstruction entry points").

Every other GPU test of these paths hands the kernels exactly-sized allocations at allocation bases and compares the output.
Here each of d_packed, d_yuv and d_rgb (and the compact source) is ONE allocation laid out  guard | payload | guard  and filled
with a sentinel byte, the payload at a chosen phase behind a 256-byte line (tests/recon_buffers.py has the arithmetic,
tests/test_recon_buffers_model.py checks it without a device).  After EVERY launch:
* both guards of the outputs are still the sentinel (a store in front of a buffer, a strip flushed past the end of a row or of a
  picture, a short last group of the four- or eight-picture forms whose stores are not switched off),
* the whole input allocation -- guards and payload -- equals its copy from before the launch (the kernels never write their input),
* the payloads equal the reference byte for byte: oracle/recon_ref.c, tests/deblock_ref.py, tests/compact.py,
* an RGB buffer that was not passed is all sentinel, and the launch ran on the form that was forced (no shape here is handed over
  to another form: test_recon_buffers_model.py::test_no_form_hands_these_shapes_over says why).
A pointer below the alignment is refused before anything is launched, and NO test launches on one.

Over-reads of the inputs cannot be seen by a guard and are checked by reading; nothing here tries to provoke one."""
import ctypes as C
import functools
import itertools

import numpy as np
import pytest

from minivideo_amd import HotPath, gen, lib
from minivideo_amd.hotpath import FAILURE, RECON_ALIGN, STAGE_COLOR, STAGE_DEBLOCK, STAGE_RECON, SUCCESS, StreamParams
from minivideo_amd.synth import synth_packed
from oracle import loader
from tests import deblock_ref
from tests.compact import COMPACT_MB_BYTES_MAX, COMPACT_SLACK_BYTES, decode_compact, expand
from tests.recon_buffers import (BAND_SHAPES, COUNTS, OFFSETS, SENTINEL, SHAPES, VARIED, alloc_bytes, guard_bytes,
                                 independent_offsets, payload_start)
from tests.test_gpu_deblock import _expected, _synthetic
from tests.test_gpu_extents import BUILT
from tests.util import Stream

pytestmark = pytest.mark.gpu

PROFILES = ("baseline", "high")
BANDED = ("wide", "quad_wide", "pipe", "pipe1")
MAXN = max(COUNTS)
# deblocking (W, H, pictures).  deblock.hip deblock_waves(): fewer than 512 pictures run 16 waves per picture, 512 and more run
# four; a wave takes every 16th (fourth) row, so 17 (5) rows give wave 0 a second pass
DEBLOCK_CASES = tuple((W, H, n) for (W, H) in ((1, 1), (2, 1), (1, 2), (7, 5)) for n in (3, 9)) + ((2, 17, 3), (2, 5, 513))


@pytest.fixture(scope="module")
def torch_cuda():
    torch = pytest.importorskip("torch")
    assert torch.cuda.is_available(), "no HIP device"
    return torch


@pytest.fixture
def form(request, hot):
    """the layout the `hot` context of this test was made with"""
    return request.node.callspec.params["hot"]


@pytest.fixture(scope="module")
def one():
    h = HotPath(0)
    yield h
    h.close()


# ---- the launch helper ----------------------------------------------------------------------------------------------------------
class Guarded:
    """one allocation  guard | payload | guard  full of SENTINEL; the payload `off` bytes behind a multiple of 256"""

    def __init__(self, torch, picture_bytes, n, off, name):
        self.torch, self.name, self.off = torch, name, off
        self.size = n * picture_bytes
        self.buf = torch.full((alloc_bytes(picture_bytes, n),), SENTINEL, dtype=torch.uint8, device="cuda")
        self.start = payload_start(self.buf.data_ptr(), picture_bytes, off)
        assert self.start >= guard_bytes(picture_bytes) and self.buf.numel() - self.start - self.size >= guard_bytes(picture_bytes)
        self.ptr = self.buf.data_ptr() + self.start
        assert self.ptr % 256 == off

    def fill(self, data):
        self.buf[self.start:self.start + self.size] = data.reshape(-1)
        return self

    def check(self, want, what):
        """the whole allocation: `want` (device, or None = still the sentinel) in the payload, the sentinel around it"""
        torch = self.torch
        exp = torch.full_like(self.buf, SENTINEL)
        if want is not None:
            exp[self.start:self.start + self.size] = want.reshape(-1)
        self.same(exp, what)

    def same(self, exp, what):
        if self.torch.equal(self.buf, exp):
            return
        bad = np.nonzero(self.buf.cpu().numpy() != exp.cpu().numpy())[0]
        lo, hi = self.start, self.start + self.size
        front, inside, back = int((bad < lo).sum()), int(((bad >= lo) & (bad < hi)).sum()), int((bad >= hi).sum())
        raise AssertionError("%s %s (phase %d): %d bytes of the front guard, %d of the payload, %d of the back guard are not what "
                             "they must be; first at payload offset %d, last at %d (payload of %d bytes)"
                             % (what, self.name, self.off, front, inside, back, int(bad[0]) - lo, int(bad[-1]) - lo, self.size))


def _launch(torch, hot, params, n, records, offs, want_yuv, want_rgb, pass_rgb=True, stages=None, yuv_in=None, form=None,
            waves=None, what=""):
    """One call of mvhp_recon_batch_dev (stages None) or mvhp_recon_stages_dev on guarded buffers at the phases offs =
    (packed, planes, RGB), and every check of the module docstring.  records / yuv_in / want_*: device tensors (want None: the
    payload must stay untouched)."""
    what = "%s %dx%d n=%d offs=%s rgb=%s stages=%s:" % (what, params.width_mbs, params.height_mbs, n, offs, pass_rgb, stages)
    P = Guarded(torch, params.packed_bytes, n, offs[0], "d_packed").fill(records)
    Y = Guarded(torch, params.yuv_bytes, n, offs[1], "d_yuv")
    if yuv_in is not None:
        Y.fill(yuv_in)
    R = Guarded(torch, params.rgb_bytes, n, offs[2], "d_rgb")
    before = P.buf.clone()
    torch.cuda.synchronize()
    runs_recon = stages is None or (stages & STAGE_RECON)
    plan = hot.plan_launch(params, n)
    if stages is None:
        hot.recon_dev(params, P.ptr, n, Y.ptr, R.ptr if pass_rgb else None, None)
    else:
        hot.recon_stages_dev(params, P.ptr, n, Y.ptr, R.ptr if pass_rgb else None, None, stages)
    hot.sync_check(None)
    if runs_recon:
        assert hot.last_launch() == plan, (what, hot.last_launch(), plan)
        assert form is None or plan[0] == form, (what, plan, form)
        assert waves is None or plan[1] == waves, (what, plan, waves)
    P.same(before, what)
    Y.check(want_yuv, what)
    R.check(want_rgb if pass_rgb else None, what)


# ---- references, once per (shape, profile) ---------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _case(W, H, profile):
    """MAXN dense synthetic pictures: params, records [MAXN, -1], the oracle's planes and RGB [MAXN, -1]"""
    params, rec = synth_packed(W, H, MAXN, seed=1000 * W + 10 * H + len(profile), profile=profile, density="dense")
    yuv, rgb = loader.recon(params, rec, MAXN, want_rgb=True)
    return params, rec.reshape(MAXN, -1), yuv.reshape(MAXN, -1), rgb.reshape(MAXN, -1)


_ON_DEVICE = {}


def _device_case(torch, W, H, profile):
    key = (W, H, profile)
    if key not in _ON_DEVICE:
        params, rec, yuv, rgb = _case(W, H, profile)
        _ON_DEVICE[key] = (params,) + tuple(torch.from_numpy(a).cuda() for a in (rec, yuv, rgb))
    return _ON_DEVICE[key]


def _recon(torch, hot, form, W, H, profile, n, offs, want_rgb, waves=None):
    params, rec, yuv, rgb = _device_case(torch, W, H, profile)
    _launch(torch, hot, params, n, rec[:n], offs, yuv[:n], rgb[:n] if want_rgb else None, pass_rgb=want_rgb, form=form,
            waves=waves, what="%s %s" % (form, profile))


# ---- mvhp_recon_batch_dev: every form ----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("W,H", SHAPES)
def test_outputs_at_every_phase(hot, form, torch_cuda, W, H):
    """1, 3, 5 and 9 pictures (short last groups of four and of eight), planes alone and with RGB, the outputs at every phase"""
    for profile, n, off, want_rgb in itertools.product(PROFILES, COUNTS, OFFSETS, (True, False)):
        _recon(torch_cuda, hot, form, W, H, profile, n, (0, off, off), want_rgb)


@pytest.mark.parametrize("W,H", VARIED)
def test_three_buffers_at_independent_phases(hot, form, torch_cuda, W, H):
    """records, planes and RGB each at a phase of its own: every pair of buffers at every pair of phases"""
    for profile, n, offs in itertools.product(PROFILES, COUNTS, independent_offsets()):
        _recon(torch_cuda, hot, form, W, H, profile, n, offs, True)
    for profile, n, offs in itertools.product(PROFILES, (3, 9), independent_offsets()):
        _recon(torch_cuda, hot, form, W, H, profile, n, offs, False)


@pytest.mark.parametrize("W,H", BAND_SHAPES)
def test_band_edges_at_every_built_size(hot, form, torch_cuda, W, H):
    """4, 5 and 9 rows -- a band edge, one row past it, two bands plus a row -- at every wave count (banded forms: rows per band)
    the form is built for"""
    try:
        for waves in BUILT[form]:
            hot.set_waves_per_picture(waves)
            for profile, n, off, want_rgb in itertools.product(PROFILES, COUNTS, OFFSETS, (True, False)):
                # a banded form runs exactly the rows per band asked for; the others step down to what the picture has rows for
                _recon(torch_cuda, hot, form, W, H, profile, n, (0, off, off), want_rgb, waves=waves if form in BANDED else None)
    finally:
        hot.set_waves_per_picture(0)


# ---- mvhp_recon_stages_dev ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("W,H", SHAPES)
def test_colour_stage_alone(one, torch_cuda, W, H):
    """MVHP_STAGE_COLOR: ycbcr_to_rgb_kernel on planes the test uploads; the planes are input here and must not change"""
    params, rec, yuv, rgb = _device_case(torch_cuda, W, H, "high")
    for n, (op, oy, orgb) in itertools.product(COUNTS, independent_offsets()[::3]):
        _launch(torch_cuda, one, params, n, rec[:n], (op, oy, orgb), yuv[:n], rgb[:n], stages=STAGE_COLOR, yuv_in=yuv[:n],
                what="colour")
    # without an RGB buffer the stage has nothing to do and touches nothing
    _launch(torch_cuda, one, params, 3, rec[:3], (16, 48, 0), yuv[:3], None, pass_rgb=False, stages=STAGE_COLOR, yuv_in=yuv[:3],
            what="colour, no RGB buffer")


@functools.lru_cache(maxsize=None)
def _deblock_case(W, H, n):
    """records as test_gpu_deblock._synthetic makes them: params (MVHP_PARAM_DEBLOCK), records, the smooth planes and their
    filtered form (deblock_ref), and what reconstruction + filter + colour conversion give from the records alone"""
    p, yuv, rec = _synthetic(W, H, n, seed=7000 + 100 * W + 10 * H + n)
    filtered = deblock_ref.deblock(yuv, rec, p).reshape(n, -1)
    full_yuv, full_rgb = _expected(p, rec, n)
    return p, rec.reshape(n, -1), yuv.reshape(n, -1), filtered, full_yuv.reshape(n, -1), full_rgb.reshape(n, -1)


@pytest.mark.parametrize("W,H,n", DEBLOCK_CASES)
def test_deblock_stage_alone(one, torch_cuda, W, H, n):
    """MVHP_STAGE_DEBLOCK in place on uploaded planes: reads the record headers, writes nothing but the planes' payload"""
    torch = torch_cuda
    p, rec, yuv, filtered, _, _ = _deblock_case(W, H, n)
    d_rec, d_yuv, d_want = (torch.from_numpy(a).cuda() for a in (rec, yuv, filtered))
    assert W * H == 1 or not np.array_equal(yuv, filtered)
    for i, off in enumerate(OFFSETS):
        _launch(torch, one, p, n, d_rec, (OFFSETS[(i + 2) % len(OFFSETS)], off, 0), d_want, None, pass_rgb=False,
                stages=STAGE_DEBLOCK, yuv_in=d_yuv, what="deblock")


@pytest.mark.parametrize("W,H,n", DEBLOCK_CASES)
def test_recon_deblock_colour(hot, form, torch_cuda, W, H, n):
    """all three stages in one call, on every form: reconstruction, the filter in place, then the separate colour kernel"""
    torch = torch_cuda
    p, rec, _, _, full_yuv, full_rgb = _deblock_case(W, H, n)
    d_rec, d_yuv, d_rgb = (torch.from_numpy(a).cuda() for a in (rec, full_yuv, full_rgb))
    for i, off in enumerate(OFFSETS):
        offs = (OFFSETS[(i + 1) % len(OFFSETS)], off, OFFSETS[(i + 3) % len(OFFSETS)])
        _launch(torch, hot, p, n, d_rec, offs, d_yuv, d_rgb, stages=STAGE_RECON | STAGE_DEBLOCK | STAGE_COLOR, form=form,
                what="%s recon + deblock + colour" % form)


# ---- mvhp_expand_compact_dev ---------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _compact_case(W, H, F, profile):
    """F pictures of a generated stream as the front end's compact pictures, `stride` apart with the slack between them full of
    the sentinel; stride: the engine's slot plus 20 bytes, so that only the first picture starts on a 16-byte boundary (the
    kernel reads compact pictures in 4-byte words); the records tests/compact.py expands them to"""
    stream, packed = gen.make_stream(W, H, F, seed=17 * W + H + F, profile=profile)
    stride = ((W * H * COMPACT_MB_BYTES_MAX + COMPACT_SLACK_BYTES + 15) & ~15) + 20
    host = np.full((F, stride), SENTINEL, np.uint8)
    want = np.zeros((F, W * H, 800), np.uint8)
    with Stream(stream) as s:
        assert s.ok and s.idr_count == F, s.error()
        p = s.params(0)
        for k in range(F):
            rc, used, buf = decode_compact(s, k)
            assert rc == 1 and 0 < used <= stride - 20
            host[k, :used] = buf[:used]
            want[k] = expand(buf, W * H)
            assert np.array_equal(want[k], packed[k]), k     # the front end's compact picture = the generator's records
    return p, stride, host, want.reshape(F, -1)


@pytest.mark.parametrize("profile", PROFILES)                    # CAVLC, CABAC with Intra8x8
@pytest.mark.parametrize("W,H,F", [(W, H, F) for (W, H) in ((1, 1), (5, 3), (11, 9)) for F in (1, 9)])
def test_expand_compact(one, torch_cuda, W, H, F, profile):
    torch = torch_cuda
    p, stride, host, want = _compact_case(W, H, F, profile)
    d_host, d_want = torch.from_numpy(host).cuda(), torch.from_numpy(want).cuda()
    for i, off in enumerate(OFFSETS):
        what = "expand %dx%d F=%d %s phase %d:" % (W, H, F, profile, off)
        S = Guarded(torch, stride, F, OFFSETS[(i + 2) % len(OFFSETS)], "d_compact").fill(d_host)
        D = Guarded(torch, p.packed_bytes, F, off, "d_packed")
        before = S.buf.clone()
        torch.cuda.synchronize()
        one.expand_compact_dev(p, S.ptr, stride, F, D.ptr)
        one.sync_check(None)
        S.same(before, what)
        D.check(d_want, what)


# ---- refusals ----------------------------------------------------------------------------------------------------------------------
def test_refused_pointers_launch_nothing(one, torch_cuda):
    """each buffer of each entry point R / 2 and 1 byte off the alignment: MVHP_FAILURE, the argument named, nothing written
    (tests/test_gpu_orient.py::test_refused_arguments_launch_nothing is the model); R off is accepted"""
    torch = torch_cuda
    L = lib()
    R = RECON_ALIGN
    params, rec, yuv, rgb = _device_case(torch, 5, 3, "high")
    n = 3
    stride = ((params.mbs * COMPACT_MB_BYTES_MAX + COMPACT_SLACK_BYTES + 15) & ~15)
    bufs = {"d_packed": Guarded(torch, params.packed_bytes, n, 0, "d_packed"), "d_yuv": Guarded(torch, params.yuv_bytes, n, 0, "d_yuv"),
            "d_rgb": Guarded(torch, params.rgb_bytes, n, 0, "d_rgb"), "d_compact": Guarded(torch, stride, n, 0, "d_compact")}
    torch.cuda.synchronize()

    def ptrs(bad, by):
        return {k: b.ptr + (by if k == bad else 0) for k, b in bufs.items()}

    def refused(rc, fn, arg):
        err = L.mvhp_last_error() or b""
        assert rc == FAILURE, "%s accepted %s off its alignment" % (fn, arg)
        assert fn.encode() in err and arg.encode() in err and b"aligned" in err, err

    pp = C.byref(params)
    # first a call that would launch nothing even if it were let through (colour stage without an RGB buffer): refused all the same
    a = ptrs("d_yuv", R // 2)
    refused(L.mvhp_recon_stages_dev(one._h, pp, a["d_packed"], n, a["d_yuv"], None, None, STAGE_COLOR), "mvhp_recon_stages_dev", "d_yuv")
    for by in (R // 2, 1):
        for bad in ("d_packed", "d_yuv", "d_rgb"):
            a = ptrs(bad, by)
            refused(L.mvhp_recon_batch_dev(one._h, pp, a["d_packed"], n, a["d_yuv"], a["d_rgb"], None), "mvhp_recon_batch_dev", bad)
            for stages in (STAGE_RECON | STAGE_COLOR, STAGE_DEBLOCK, STAGE_COLOR):
                refused(L.mvhp_recon_stages_dev(one._h, pp, a["d_packed"], n, a["d_yuv"], a["d_rgb"], None, stages),
                        "mvhp_recon_stages_dev", bad)
        for bad in ("d_compact", "d_packed"):
            a = ptrs(bad, by)
            refused(L.mvhp_expand_compact_dev(one._h, pp, a["d_compact"], stride, n, a["d_packed"], None), "mvhp_expand_compact_dev", bad)
    one.sync_check(None)
    for b in bufs.values():
        b.check(None, "a refused call wrote:")
    # R off is inside the contract: accepted, and right
    _launch(torch, one, params, n, rec[:n], (R, R, R), yuv[:n], rgb[:n], what="R off")
    assert L.mvhp_recon_stages_dev(one._h, pp, bufs["d_packed"].ptr + R, n, bufs["d_yuv"].ptr + R, None, None, STAGE_COLOR) == SUCCESS
