"""CPU: the opt-in deblocking filter (clause 8.7; MVHP_STREAM_DEBLOCK / MVHP_PARAM_DEBLOCK / MINIVIDEO_DEBLOCK=1).  Outside the
parity contract: the reference never deblocks, and there is no other decoder here -- the authority is the standard's text.

Hand known answers (2 x 1 macroblocks, Intra16x16, one slice, rows constant; left luma 100, right 110, chroma 128):
  1. QP 36 both, offsets 0: qPav = 36 -> indexA = indexB = 36, alpha = 50, beta = 11 (Table 8-16), bS = 4 (macroblock edge).
     ap = |p2 - p0| = 0 < beta, aq = 0 < beta, |p0 - q0| = 10 < (50 >> 2) + 2 = 14: the strong filter (8.7.2.4) on both sides:
       p0' = (p2 + 2p1 + 2p0 + 2q0 + q1 + 4) >> 3 = (100 + 200 + 200 + 220 + 110 + 4) >> 3 = 834 >> 3 = 104
       p1' = (p2 + p1 + p0 + q0 + 2) >> 2 = 412 >> 2 = 103;  p2' = (2p3 + 3p2 + p1 + p0 + q0 + 4) >> 3 = 814 >> 3 = 101
       q0' = (p1 + 2p0 + 2q0 + 2q1 + q2 + 4) >> 3 = 854 >> 3 = 106;  q1' = (p0 + q0 + q1 + q2 + 2) >> 2 = 432 >> 2 = 108
       q2' = (2q3 + 3q2 + q1 + q0 + p0 + 4) >> 3 = 874 >> 3 = 109
     -> columns 12..19 = 100 101 103 104 | 106 108 109 110.  The right macroblock's internal edge at x = 20 (bS 3) then sees
     p = 106 108 109 110, q = 110 110 ..: delta = Clip3(-tc, tc, ((0 << 2) + (109 - 110) + 4) >> 3) = 0, and p1' = 109 +
     Clip3(-tc0, tc0, (108 + 110 - 218) >> 1) = 109: nothing changes; horizontal edges see constant columns.
  2. QP 20 both: alpha(20) = 7 <= |p0 - q0| = 10: nothing.  slice_alpha_c0_offset_div2 = 6: indexA = 20 + 12 = 32, alpha = 32,
     beta(20) = 3; 10 < (32 >> 2) + 2 = 10 is false -> the 3-tap form: p0' = (2p1 + p0 + q1 + 2) >> 2 = (200 + 100 + 110 + 2) >> 2
     = 103, q0' = (2q1 + q0 + p1 + 2) >> 2 = (220 + 110 + 100 + 2) >> 2 = 108; p1, p2 untouched.
  3. Case 1 with Cb 100 | 110 (chroma columns 7 | 8): QPc(36) = 34 (Table 8-15) both sides, alpha(34) = 40, beta(34) = 10, bS 4
     chroma (always the 3-tap form): column 7 -> 103, column 8 -> 108.
  Case 1 with disable_deblocking_filter_idc = 1, or with the right macroblock at QP 0 (qPav = (36 + 0 + 1) >> 1 = 18,
  alpha(18) = 5 <= 10): nothing changes."""
import ctypes as C
import os
import shutil
import subprocess

import numpy as np
import pytest

from minivideo_amd import gen
from minivideo_amd.hotpath import PARAM_DEBLOCK, STREAM_DEBLOCK, STREAM_SPEC, StreamParams, lib
from tests import deblock_ref as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PROFILES = ("baseline", "main", "main_cavlc", "high", "high_cavlc", "high_4x4")


class DStream:
    """a stream handle opened with mvhp_stream_open_ex(flags)"""

    def __init__(self, data, flags):
        self.L = lib()
        self.L.mvhp_stream_last_error.restype = C.c_char_p
        self.L.mvhp_stream_open_ex.restype = C.c_int
        self.L.mvhp_stream_open_ex.argtypes = [C.c_void_p, C.c_size_t, C.c_uint32, C.POINTER(C.c_void_p)]
        self.data = np.ascontiguousarray(data, dtype=np.uint8)
        self.h = C.c_void_p()
        self.ok = self.L.mvhp_stream_open_ex(self.data.ctypes.data, self.data.size, flags, C.byref(self.h)) == 1

    def __enter__(self):
        return self

    def __exit__(self, *a):
        if self.h:
            self.L.mvhp_stream_close(self.h)
            self.h = None

    def params(self, idr=0):
        p = StreamParams()
        return p if self.L.mvhp_stream_params(self.h, idr, C.byref(p)) == 1 else None

    def packed(self, idr):
        p = self.params(idr)
        out = np.zeros(p.packed_bytes, np.uint8)
        rc = self.L.mvhp_stream_decode_packed(self.h, idr, out.ctypes.data, out.size)
        return rc, out

    def error(self):
        e = self.L.mvhp_stream_last_error()
        return e.decode() if e else ""


def kat_planes(qp=(36, 36), offsets=(0, 0), idc=0, cb=(128, 128)):
    """the 2 x 1 known-answer picture: (params, yuv, records)"""
    p = StreamParams(2, 1, 0, 0, PARAM_DEBLOCK)
    yuv = np.zeros(2 * 384, np.uint8)
    Y = yuv[:512].reshape(16, 32)
    Y[:, :16], Y[:, 16:] = 100, 110
    Cb = yuv[512:640].reshape(8, 16)
    Cb[:, :8], Cb[:, 8:] = cb
    yuv[640:] = 128
    rec = np.zeros((2, 800), np.uint8)
    for m in range(2):
        rec[m, 0], rec[m, 1] = 2, qp[m]                            # Intra16x16, QP'Y
        rec[m, 5] = idc << 1
        rec[m, 7] = (offsets[0] & 15) | ((offsets[1] & 15) << 4)
    return p, yuv, rec


KAT = [  # (kwargs, luma row 0 columns 12..19, Cb row 0 columns 6..9)
    (dict(), [100, 101, 103, 104, 106, 108, 109, 110], [128] * 4),
    (dict(qp=(20, 20)), [100] * 4 + [110] * 4, [128] * 4),
    (dict(qp=(20, 20), offsets=(6, 0)), [100, 100, 100, 103, 108, 110, 110, 110], [128] * 4),
    (dict(cb=(100, 110)), [100, 101, 103, 104, 106, 108, 109, 110], [100, 103, 108, 110]),
    (dict(idc=1), [100] * 4 + [110] * 4, [128] * 4),
    (dict(qp=(36, 0)), [100] * 4 + [110] * 4, [128] * 4),
]


@pytest.mark.parametrize("kw,luma,cb", KAT)
def test_known_answers_on_the_reference(kw, luma, cb):
    p, yuv, rec = kat_planes(**kw)
    out = R.deblock(yuv, rec, p)
    Y, Cb = out[:512].reshape(16, 32), out[512:640].reshape(8, 16)
    assert (Y == Y[0]).all() and (Cb == Cb[0]).all()               # rows stay constant
    assert list(Y[0, 12:20]) == luma and list(Y[0, :12]) == [100] * 12 and list(Y[0, 20:]) == [110] * 12
    assert list(Cb[0, 6:10]) == cb
    assert (out[640:] == 128).all()


def test_reference_tables_spot_values():
    assert R.ALPHA[36] == 50 and R.BETA[36] == 11 and R.ALPHA[20] == 7 and R.BETA[20] == 3 and R.ALPHA[32] == 32
    assert R.ALPHA[18] == 5 and R.ALPHA[34] == 40 and R.BETA[34] == 10 and R.QPC[36] == 34 and R.QPC[29] == 29
    assert R.TC0_BS3[17] == 1 and R.TC0_BS3[51] == 25 and R.ALPHA[51] == 255 and R.BETA[51] == 18


# ---- the front end's record fields against the generator's ----
def _gen(profile, seed, slices, idc, offsets, pcm=0, W=5, H=4, n=2, cqp=(0, 0)):
    return gen.make_stream_ex(W, H, n, seed=seed, profile=profile, slices=slices, pcm_permille=pcm, cqp_offsets=cqp,
                              qp_range=(0, 51), deblock=dict(idc=idc, offsets=offsets))


@pytest.mark.parametrize("profile", PROFILES)
@pytest.mark.parametrize("idc", [(0,), (1,), (2,), (0, 1, 2)])
def test_front_end_matches_the_generator_one_slice(profile, idc):
    for seed in range(3):
        stream, packed, _ = _gen(profile, seed, 1, idc, (-6, 6))
        with DStream(stream, STREAM_DEBLOCK) as s:
            assert s.ok, s.error()
            assert s.params(0).flags & PARAM_DEBLOCK
            for k in range(packed.shape[0]):
                rc, got = s.packed(k)
                assert rc == 1, s.error()
                assert np.array_equal(got.reshape(packed[k].shape), packed[k]), (profile, seed, k)
        fl = packed[:, :, 5]
        assert set(np.unique((fl >> 1) & 3)) <= set(idc)


@pytest.mark.parametrize("profile", PROFILES)
def test_front_end_matches_the_generator_several_slices(profile):
    """spec mode and deblock mode together: several slices, I_PCM, per-slice idc / offsets"""
    seen = set()
    for seed in range(4):
        stream, packed, _ = _gen(profile, seed, 4, (0, 1, 2), (-6, 6), pcm=60, W=6, H=5)
        with DStream(stream, STREAM_SPEC | STREAM_DEBLOCK) as s:
            assert s.ok, s.error()
            p = s.params(0)
            assert p.flags & PARAM_DEBLOCK and p.flags & 4            # MVHP_PARAM_SLICES
            for k in range(packed.shape[0]):
                rc, got = s.packed(k)
                assert rc == 1, s.error()
                assert np.array_equal(got.reshape(packed[k].shape), packed[k]), (profile, seed, k)
        seen |= set(np.unique(packed[:, :, 7]).tolist())
    assert len(seen) > 3                                           # offsets really vary from slice to slice


def test_without_the_flag_the_records_carry_nothing():
    stream, packed, _ = _gen("high", 3, 1, (0, 2), (-6, 6))
    with DStream(stream, 0) as s:
        assert s.ok and not (s.params(0).flags & PARAM_DEBLOCK)
        rc, got = s.packed(0)
        assert rc == 1
        got = got.reshape(packed[0].shape)
        assert not got[:, 5].any() and not got[:, 7].any()
        want = packed[0].copy()
        want[:, 5] = 0
        want[:, 7] = 0
        assert np.array_equal(got, want)


def test_generator_without_the_option_is_unchanged():
    """no deblock argument: byte-identical streams (the golden md5 fixture pins them); with it the macroblocks are the same"""
    a, pa, _ = gen.make_stream_ex(4, 3, 2, seed=5, profile="main")
    b, pb, _ = gen.make_stream_ex(4, 3, 2, seed=5, profile="main")
    c, pc, _ = gen.make_stream_ex(4, 3, 2, seed=5, profile="main", deblock=dict(idc=(1,), offsets=(0, 0)))
    assert np.array_equal(a, b) and not np.array_equal(a, c)
    pc = pc.copy()
    pc[:, :, 5] = 0
    assert np.array_equal(pa, pc)


def test_open_ex_accepts_the_deblock_flag():
    stream, _, _ = _gen("baseline", 1, 1, (0,), (0, 0))
    for flags in (STREAM_DEBLOCK, STREAM_SPEC | STREAM_DEBLOCK):
        with DStream(stream, flags) as s:
            assert s.ok and (s.params(0).flags & PARAM_DEBLOCK)
    with DStream(stream, STREAM_SPEC) as s:
        assert s.ok and not (s.params(0).flags & PARAM_DEBLOCK)
    with DStream(stream, 4) as s:                                  # unknown flags are still refused
        assert not s.ok


@pytest.mark.parametrize("idc,offsets,why", [((3,), (0, 0), "disable_deblocking_filter_idc"),
                                             ((0,), (7, 7), "offsets out of range"),
                                             ((2,), (-7, -7), "offsets out of range")])
def test_out_of_range_syntax_refused_only_in_deblock_mode(idc, offsets, why):
    stream, _, _ = _gen("main", 2, 1, idc, offsets)
    with DStream(stream, 0) as s:                                  # reference mode: parsed and dropped, as before
        assert s.ok and s.packed(0)[0] == 1
    with DStream(stream, STREAM_DEBLOCK) as s:
        assert s.ok
        rc, _ = s.packed(0)
        assert rc != 1 and why in s.error()


# ---- the kernel's per-edge arithmetic (deblock_edge.h), host-compiled, against the reference ----
_HARNESS = r"""
#include "deblock_edge.h"
static const uint8_t A[52] = MVDB_ALPHA_TABLE, B[52] = MVDB_BETA_TABLE, T[52] = MVDB_TC0_BS3_TABLE, Q[22] = MVDB_QPC_TABLE;
extern "C" void run(const int *lines, const int *prm, int *out, int n)
{   // prm per line: qPav, alpha_div2, beta_div2, bs4, chroma
    for (int i = 0; i < n; i++) {
        int v[8];
        for (int k = 0; k < 8; k++) v[k] = lines[i * 8 + k];
        const int *p = prm + i * 5;
        mvdb::EdgeParams e = mvdb::edge_params(p[0], p[1], p[2], p[3], A, B, T);
        mvdb::filter_line(v, e, p[4] != 0);
        for (int k = 0; k < 8; k++) out[i * 8 + k] = v[k];
    }
}
extern "C" int qpc(int qpy, int off) { return mvdb::qpc_of(qpy, off, Q); }
"""


@pytest.fixture(scope="module")
def edge_lib(tmp_path_factory):
    cxx = shutil.which("g++") or shutil.which("c++")
    if cxx is None:
        pytest.fail("no host C++ compiler")
    d = tmp_path_factory.mktemp("edge")
    src, so = d / "h.cpp", d / "libedge.so"
    src.write_text(_HARNESS)
    subprocess.run([cxx, "-O2", "-shared", "-fPIC", "-I" + os.path.join(ROOT, "minivideo_amd", "csrc", "hip"), str(src), "-o",
                    str(so)], check=True)
    L = C.CDLL(str(so))
    L.run.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_int]
    L.qpc.argtypes = [C.c_int, C.c_int]
    return L


def test_edge_arithmetic_matches_the_reference(edge_lib):
    rng = np.random.default_rng(8)
    n = 200000
    base = rng.integers(0, 256, n)
    # smooth lines with a step and small noise, plus fully random ones: every branch (alpha / beta pass and fail, strong and
    # normal bS 4, tC clipping, 0 / 255 clipping)
    step = rng.integers(-40, 41, n)
    noise = rng.integers(-3, 4, (n, 8)) * (rng.random(n) < 0.7)[:, None]
    lines = np.clip(base[:, None] + noise + np.where(np.arange(8) >= 4, step[:, None], 0), 0, 255)
    wild = rng.random(n) < 0.15
    lines[wild] = rng.integers(0, 256, (int(wild.sum()), 8))
    lines = lines.astype(np.int32)
    prm = np.stack([rng.integers(0, 52, n), rng.integers(-6, 7, n), rng.integers(-6, 7, n), rng.integers(0, 2, n),
                    rng.integers(0, 2, n)], 1).astype(np.int32)
    out = np.zeros_like(lines)
    edge_lib.run(np.ascontiguousarray(lines).ctypes.data, np.ascontiguousarray(prm).ctypes.data, out.ctypes.data, n)
    want = np.zeros_like(lines)
    for chroma in (0, 1):
        sel = prm[:, 4] == chroma
        al, be, tc = R.edge_params(prm[sel, 0], prm[sel, 1], prm[sel, 2])
        want[sel] = R.filter_lines(lines[sel], al, be, tc, prm[sel, 3] == 1, bool(chroma))
    changed = (want != lines).any(1)
    assert changed.mean() > 0.2 and (~changed).mean() > 0.2
    assert np.array_equal(out, want)
    for q in range(52):
        for off in range(-12, 13):
            assert edge_lib.qpc(q, off) == R.qpc(q, off)


def test_reference_matches_a_plain_raster_loop():
    """deblock_ref filters the macroblocks of one x + 2y together; the standard's raster order written out as plain loops must
    give the same bytes"""
    rng = np.random.default_rng(3)
    W, H, n = 5, 4, 2
    p = StreamParams(W, H, rng.integers(-12, 13), rng.integers(-12, 13), PARAM_DEBLOCK)
    rec = np.zeros((n, W * H, 800), np.uint8)
    rec[:, :, 0] = rng.integers(0, 4, (n, W * H))
    rec[:, :, 1] = rng.integers(10, 52, (n, W * H))
    rec[:, :, 5] = rng.integers(0, 3, (n, W * H)) << 1
    rec[:, :, 6] = rng.integers(0, 16, (n, W * H))
    rec[:, :, 7] = (rng.integers(-6, 7, (n, W * H)) & 15) | ((rng.integers(-6, 7, (n, W * H)) & 15) << 4)
    yuv = np.clip(128 + rng.integers(-6, 7, (n, W * H * 384)) + np.repeat(rng.integers(-30, 31, (n, W * H * 384 // 8)), 8, 1),
                  0, 255).astype(np.uint8)
    got = R.deblock(yuv, rec, p)
    want = _raster(yuv, rec, p)
    assert not np.array_equal(got, yuv) and np.array_equal(got, want)


def _raster(yuv, rec, p):
    W, H = int(p.width_mbs), int(p.height_mbs)
    n = yuv.shape[0]
    out = yuv.astype(np.int32).copy()
    qp, idc, a2, b2, t8, un = (a.reshape(n, H, W) for a in R.header_fields(rec, n, W * H))
    for f in range(n):
        for plane, base, mbsz, off in ((0, 0, 16, None), (1, W * H * 256, 8, int(p.chroma_qp_index_offset)),
                                       (2, W * H * 320, 8, int(p.second_chroma_qp_index_offset))):
            P = out[f, base:base + W * H * mbsz * mbsz].reshape(H * mbsz, W * mbsz)
            q = qp[f] if off is None else R.qpc(qp[f], off)
            for y in range(H):
                for x in range(W):
                    if idc[f, y, x] == 1:
                        continue
                    for d in (0, 1):
                        nb_ok = (x > 0) if d == 0 else (y > 0)
                        if idc[f, y, x] == 2 and (un[f, y, x] & (1 if d == 0 else 2)):
                            nb_ok = False
                        for k in range(mbsz // 4):
                            if k == 0 and not nb_ok:
                                continue
                            if off is None and k in (1, 3) and t8[f, y, x]:
                                continue
                            if k == 0:
                                qpav = (q[y, x] + (q[y, x - 1] if d == 0 else q[y - 1, x]) + 1) >> 1
                            else:
                                qpav = q[y, x]
                            al, be, tc = R.edge_params(qpav, a2[f, y, x], b2[f, y, x])
                            for i in range(mbsz):
                                if d == 0:
                                    r, c0 = y * mbsz + i, x * mbsz + 4 * k - 4
                                    P[r, c0:c0 + 8] = R.filter_lines(P[r, c0:c0 + 8], al, be, tc, k == 0, off is not None)
                                else:
                                    c, r0 = x * mbsz + i, y * mbsz + 4 * k - 4
                                    P[r0:r0 + 8, c] = R.filter_lines(P[r0:r0 + 8, c], al, be, tc, k == 0, off is not None)
    return out.astype(np.uint8)
