"""CPU: the representative-picture policy (DESIGN.md 3 "Representative pictures"): the library's host functions (mvhp_hist_stats,
mvhp_represent_choose) and the policy header the library compiles (csrc/host/represent_policy.h, host-compiled here) against the
Python-integer restatement (tests/hist_ref.py) and against known answers; the two switches, malformed."""
import ctypes as C
import os
import random
import shutil
import subprocess

import numpy as np
import pytest

from minivideo_amd.hotpath import (LUMA_STATS_DTYPE, PLANE_HIST_DTYPE, LumaStats, PlaneHist, hist_stats, luma_score,
                                   represent_choose)
from tests import hist_ref as R, luma_ref as L

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

_HARNESS = r"""
#include <stdio.h>
#include "represent_policy.h"
extern "C" int choose(const mvhp_plane_hist_t *h, int n, const unsigned char *el) { return mvrep::choose(h, n, el); }
extern "C" void stats(const mvhp_plane_hist_t *h, mvhp_luma_stats_t *out) { mvrep::hist_stats(*h, *out); }
extern "C" unsigned score(unsigned long long s, unsigned long long q, unsigned n) { return mvblank::luma_score(s, q, n); }
extern "C" int settings(const char *on, const char *alts, int *is_on, int *a, char *why, int cap)
{
    mvrep::Settings s;
    std::string w;
    const bool ok = mvrep::settings_from(on, alts, s, w);
    *is_on = s.on; *a = s.alternates;
    snprintf(why, (size_t)cap, "%s", w.c_str());
    return ok ? 1 : 0;
}
"""


@pytest.fixture(scope="module")
def policy_lib(tmp_path_factory):
    cxx = shutil.which("g++") or shutil.which("c++")
    if cxx is None:
        pytest.fail("no host C++ compiler")
    d = tmp_path_factory.mktemp("represent")
    src, so = d / "h.cpp", d / "librepresent.so"
    src.write_text(_HARNESS)
    subprocess.run([cxx, "-O2", "-std=c++17", "-shared", "-fPIC", "-I" + os.path.join(ROOT, "minivideo_amd", "csrc", "host"),
                    "-I" + os.path.join(ROOT, "include"), str(src), "-o", str(so)], check=True)
    lib = C.CDLL(str(so))
    lib.choose.argtypes = [C.c_void_p, C.c_int, C.c_void_p]
    lib.stats.argtypes = [C.c_void_p, C.c_void_p]
    lib.stats.restype = None
    lib.score.restype = C.c_uint32
    lib.score.argtypes = [C.c_uint64, C.c_uint64, C.c_uint32]
    lib.settings.argtypes = [C.c_char_p, C.c_char_p, C.POINTER(C.c_int), C.POINTER(C.c_int), C.c_char_p, C.c_int]
    return lib


def _all(policy_lib, recs, eligible=None):
    """the choice by the restatement, the library and the host-compiled header: equal, and returned"""
    recs = np.ascontiguousarray(recs, dtype=PLANE_HIST_DTYPE).reshape(-1)
    el = None if eligible is None else np.asarray([1 if e else 0 for e in eligible], np.uint8)
    want = R.choose(recs, eligible)
    got_lib = represent_choose(recs, eligible)
    got_hdr = policy_lib.choose(recs.ctypes.data, len(recs), None if el is None else el.ctypes.data)
    assert want == got_lib == got_hdr, (want, got_lib, got_hdr)
    return want


def _rec(y=None, cb=None, cr=None, samples=None, chroma=None):
    """a record from sparse {value: count} dictionaries"""
    r = np.zeros(1, PLANE_HIST_DTYPE)
    for name, d in (("y", y), ("cb", cb), ("cr", cr)):
        for v, c in (d or {}).items():
            r[name][0][v] = c
    r["samples"] = sum((y or {}).values()) if samples is None else samples
    r["chroma_samples"] = sum((cb or {}).values()) if chroma is None else chroma
    return r


def _cat(*recs):
    return np.concatenate(recs)


def test_record_layout():
    assert C.sizeof(PlaneHist) == 3104 and PLANE_HIST_DTYPE.itemsize == 3104 and R.HIST_DTYPE == PLANE_HIST_DTYPE
    assert PlaneHist.y.offset == 0 and PlaneHist.cb.offset == 1024 and PlaneHist.cr.offset == 2048
    assert PlaneHist.samples.offset == 3072 and PlaneHist.chroma_samples.offset == 3076 and PlaneHist.reserved.offset == 3080


# ---- the choice ----
def test_one_and_two_candidates_return_the_first(policy_lib):
    a, b = _rec({0: 64}, {128: 16}, {128: 16}), _rec({255: 64}, {0: 16}, {255: 16})
    assert _all(policy_lib, a) == 0
    assert _all(policy_lib, _cat(a, b)) == 0 and _all(policy_lib, _cat(b, a)) == 0
    assert _all(policy_lib, _cat(a, b, b), [1, 1, 0]) == 0              # two candidates of three entries
    assert _all(policy_lib, _cat(a, b, b), [0, 0, 1]) == 2              # one


def test_the_outlier_is_never_chosen(policy_lib):
    near = [_rec({100: 60, 101: 4}, {128: 16}, {128: 16}), _rec({100: 58, 101: 6}, {128: 16}, {128: 16})]
    out = _rec({0: 64}, {30: 16}, {200: 16})
    for order in ((0, 1, 2), (0, 2, 1), (2, 0, 1), (2, 1, 0), (1, 2, 0), (1, 0, 2)):
        recs = [near[0], near[1], out]
        got = _all(policy_lib, _cat(*[recs[i] for i in order]))
        assert order[got] != 2, order
    # an outlier in chroma alone: the three planes count alike
    same = _rec({50: 64}, {128: 16}, {128: 16})
    assert _all(policy_lib, _cat(_rec({50: 64}, {128: 16}, {10: 16}), same, same)) == 1


def test_all_equal_returns_the_first(policy_lib):
    a = _rec({7: 10, 9: 54}, {1: 16}, {2: 16})
    assert _all(policy_lib, _cat(*[a] * 5)) == 0
    assert _all(policy_lib, _cat(*[a] * 17)) == 0


def test_primary_ineligible(policy_lib):
    a = _rec({7: 64}, {1: 16}, {2: 16})
    assert _all(policy_lib, _cat(*[a] * 4), [0, 0, 1, 1]) == 2          # the first eligible among equal ones
    assert _all(policy_lib, _cat(*[a] * 4), [0, 1, 1, 1]) == 1
    # the first eligible entry sets the sizes: entries of another size are no candidates
    other = _rec({7: 32}, {1: 8}, {2: 8})
    assert _all(policy_lib, _cat(a, other, other, other), [0, 1, 1, 1]) == 1
    assert _all(policy_lib, _cat(a, other, a, a), [0, 1, 1, 1]) == 1    # one candidate: the two of the primary's size are not


def test_none_eligible(policy_lib):
    a = _rec({7: 64}, {1: 16}, {2: 16})
    assert _all(policy_lib, _cat(a, a, a), [0, 0, 0]) == -1
    assert _all(policy_lib, a, [0]) == -1
    assert represent_choose(np.zeros(0, PLANE_HIST_DTYPE)) == -1
    assert policy_lib.choose(None, 0, None) == -1 and policy_lib.choose(None, 3, None) == -1
    assert policy_lib.choose(a.ctypes.data, -2, None) == -1 and policy_lib.choose(a.ctypes.data, 0, None) == -1


def test_other_sizes_are_no_candidates(policy_lib):
    a, b = _rec({10: 64}, {1: 16}, {2: 16}), _rec({12: 64}, {1: 16}, {2: 16})
    odd = _rec({10: 32, 12: 32}, {1: 16}, {2: 16}, samples=63)          # the exact mean, but another size
    assert _all(policy_lib, _cat(a, odd, b)) == 0                       # two candidates: the first
    odd2 = _rec({10: 32, 12: 32}, {1: 16}, {2: 16}, chroma=15)
    assert _all(policy_lib, _cat(a, odd2, b)) == 0
    mid = _rec({10: 32, 12: 32}, {1: 16}, {2: 16})
    assert _all(policy_lib, _cat(a, mid, b)) == 1                       # ... and of the same size it wins


def test_largest_counts_do_not_overflow(policy_lib):
    """17 candidates, 2^28 samples in one bin: sixteen at bin 0, one at bin 255 -- |k h - M| = 16 * 2^28 in two bins of the odd
    one, a distance of 2^65 that a 64-bit sum would lose"""
    n, c = 1 << 28, 1 << 26
    a, odd = _rec({0: n}, {0: c}, {0: c}), _rec({255: n}, {0: c}, {0: c})
    for at in (0, 5, 16):
        recs = [a] * 17
        recs[at] = odd
        d = R.distances([R.bins(r[0]) for r in recs])
        assert max(d) == 2 * (16 * n) ** 2 and max(d) > 1 << 64 and d.index(max(d)) == at
        assert _all(policy_lib, _cat(*recs)) == (1 if at == 0 else 0)
    # every bin of every plane at its largest difference: the sum stays below 2^76
    full = np.zeros(1, PLANE_HIST_DTYPE)
    for p in ("y", "cb", "cr"):
        full[p][0][:] = n
    full["samples"] = full["chroma_samples"] = n
    zero = np.zeros(1, PLANE_HIST_DTYPE)
    zero["samples"] = zero["chroma_samples"] = n
    recs = [zero] * 17
    recs[3] = full
    assert max(R.distances([R.bins(r[0]) for r in recs])) == 768 * (16 * n) ** 2 < 1 << 76
    assert _all(policy_lib, _cat(*recs)) == 0
    recs = [full] * 17
    recs[0] = zero
    assert _all(policy_lib, _cat(*recs)) == 1


def test_random_cases_against_python_integers(policy_lib):
    rnd = random.Random(11)
    rng = np.random.default_rng(11)
    for case in range(2000):
        n = rnd.randrange(1, 18)
        samples = rnd.choice([4, 64, 1920 * 1080, 1 << 28])
        recs = np.zeros(n, PLANE_HIST_DTYPE)
        kind = rnd.randrange(4)
        centre = rng.integers(0, 256, 3)
        for i in range(n):
            for k, (p, total) in enumerate((("y", samples), ("cb", samples // 4), ("cr", samples // 4))):
                if kind == 0:                                          # a few populated bins near a common centre: close races
                    at = (centre[k] + rng.integers(-2, 3, 4)) % 256
                    part = rng.multinomial(total, [0.25] * 4) if total < 1 << 27 else np.array([total // 4] * 3 + [total - 3 * (total // 4)])
                    np.add.at(recs[p][i], at, part.astype(np.uint32))
                elif kind == 1:                                        # one bin: many exact ties
                    recs[p][i][rnd.choice([0, 255, int(centre[k])])] = total
                else:                                                  # spread over all bins
                    w = rng.integers(0, 1 << 12, 256).astype(np.uint64)
                    c = (w * total // max(int(w.sum()), 1)).astype(np.uint32)
                    c[0] += total - int(c.sum())
                    recs[p][i] = c
            recs["samples"][i], recs["chroma_samples"][i] = samples, samples // 4
            if rnd.random() < 0.15:                                    # an entry of another size
                if rnd.random() < 0.5:
                    recs["samples"][i] = samples - 2
                else:
                    recs["chroma_samples"][i] = samples // 4 + 1
        eligible = None if rnd.random() < 0.3 else [rnd.random() < 0.7 for _ in range(n)]
        got = _all(policy_lib, recs, eligible)
        assert (got == -1) == (eligible is not None and not any(eligible)), case


# ---- the score of a histogram ----
def _stats_all(policy_lib, rec):
    rec = np.ascontiguousarray(rec, dtype=PLANE_HIST_DTYPE).reshape(1)
    out = np.full(1, 0xA5, np.uint8).repeat(32).view(LUMA_STATS_DTYPE)
    policy_lib.stats(rec.ctypes.data, out.ctypes.data)
    st = hist_stats(rec)
    assert isinstance(st, LumaStats) and bytes(st) == out.tobytes()
    assert (int(out["sum"][0]), int(out["sumsq"][0]), int(out["samples"][0])) == R.stats(rec[0]) and not out["reserved"].any()
    return st


def test_hist_stats_is_the_picture_score_record(policy_lib):
    rng = np.random.default_rng(5)
    for wmb, hmb, rect in ((1, 1, (0, 0, 16, 16)), (3, 2, (6, 2, 30, 22)), (20, 17, (2, 4, 310, 262)), (2, 2, (30, 30, 2, 2))):
        for content in ("random", "flat", "dark"):
            yuv = {"random": rng.integers(0, 256, wmb * hmb * 384), "flat": np.full(wmb * hmb * 384, 200),
                   "dark": rng.integers(0, 3, wmb * hmb * 384)}[content].astype(np.uint8)
            rec = R.record(yuv, wmb, hmb, rect)
            st = _stats_all(policy_lib, rec)
            direct = L.record(L.luma_plane(yuv, wmb, hmb), *rect)       # what mvhp_luma_stats_dev writes: from the samples
            assert bytes(st) == direct.tobytes()
            want = L.score(*L.stats(L.luma_plane(yuv, wmb, hmb), *rect))
            assert luma_score(st) == want == policy_lib.score(st.sum, st.sumsq, st.samples)
    big = _rec({255: 1 << 28})                                          # the largest record: sumsq = 255^2 2^28
    st = _stats_all(policy_lib, big)
    assert (st.sum, st.sumsq, st.samples) == (255 << 28, 255 * 255 << 28, 1 << 28) and luma_score(st) == 0
    half = _rec({0: 1 << 27, 255: 1 << 27})
    assert luma_score(_stats_all(policy_lib, half)) == L.SCORE_MAX


# ---- the streams of the GPU tests ----
def test_the_cli_streams_pick_their_winners_by_the_reference_rule():
    """tests/test_gpu_cli_represent.py relies on it: on the oracle's planes the reference rule alone picks the stated IDR for every
    slot, with and without the blank threshold, every other picture at least twice as far from the mean (scenario() asserts it)"""
    from tests import represent_streams as S
    for name, (letters, n, final, final_b) in S.SCENARIOS.items():
        stream, planes, scores, recs = S.scenario(name)
        assert planes.shape[0] == len(letters) == len(scores) == len(recs) and len(final) == len(final_b) == n
        assert all((sc >= S.B.MIN_SCORE) == c.isupper() for sc, c in zip(scores, letters))
    assert S.SCENARIOS["outlier"][2] != [0] and S.SCENARIOS["blank_majority"][2] != S.SCENARIOS["blank_majority"][3]


# ---- the switches ----
def _settings(policy_lib, on, alts):
    is_on, a, why = C.c_int(), C.c_int(), C.create_string_buffer(256)
    enc = [None if v is None else v.encode() for v in (on, alts)]
    ok = policy_lib.settings(*enc, C.byref(is_on), C.byref(a), why, 256)
    return ok, is_on.value, a.value, why.value.decode()


def test_settings(policy_lib):
    assert _settings(policy_lib, None, None) == (1, 0, 8, "")
    assert _settings(policy_lib, "", "") == (1, 0, 8, "")
    assert _settings(policy_lib, "1", None) == (1, 1, 8, "")
    assert _settings(policy_lib, "0", "16") == (1, 0, 16, "")
    assert _settings(policy_lib, "1", "1") == (1, 1, 1, "")
    for var, bad in [("MINIVIDEO_REPRESENTATIVE_ALTERNATES", v) for v in ("abc", "-1", "0", "17", "4x", " 4", "4 ", "1.5", "99999999999")] + \
                    [("MINIVIDEO_REPRESENTATIVE", v) for v in ("abc", "2", "-1", "yes", "1 ")]:
        for on in ("0", "1"):                                           # malformed fails whether or not the feature is on
            args = {"MINIVIDEO_REPRESENTATIVE": on, "MINIVIDEO_REPRESENTATIVE_ALTERNATES": None}
            args[var] = bad
            ok, _, _, why = _settings(policy_lib, args["MINIVIDEO_REPRESENTATIVE"], args["MINIVIDEO_REPRESENTATIVE_ALTERNATES"])
            assert ok == 0 and why.startswith(var + "=") and "'%s'" % bad in why, (var, bad, why)
