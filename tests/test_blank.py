"""CPU: picture scores and the blank-picture policy (DESIGN.md 3 "Picture scores"): the library's host functions
(mvhp_luma_score, mvhp_blank_choose) and the policy header the library compiles (csrc/host/blank_policy.h, host-compiled here)
against the Python-integer restatement (tests/luma_ref.py) and against known answers; the three environment values, malformed,
through the product CLI: the call fails with a message that names the variable, before any device work (this box has no device:
a call that got further would fail with another message)."""
import ctypes as C
import os
import random
import shutil
import subprocess

import numpy as np
import pytest

from minivideo_amd import gen
from minivideo_amd.hotpath import LUMA_STATS_DTYPE, LumaStats, blank_choose, luma_score
from tests import luma_ref as L

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CLI = os.path.join(ROOT, "minivideo_amd", "mini_thumbnailer")

_HARNESS = r"""
#include "blank_policy.h"
extern "C" unsigned score(unsigned long long s, unsigned long long q, unsigned n) { return mvblank::luma_score(s, q, n); }
extern "C" int choose(const unsigned *v, int n, unsigned m) { return mvblank::choose(v, n, m); }
extern "C" int alternates(const int *slots, int n_slots, int n_idr, int a, int k, int *out)
{
    const std::vector<int> r = mvblank::alternates(std::vector<int>(slots, slots + n_slots), n_idr, a, k);
    for (size_t i = 0; i < r.size(); i++) out[i] = r[i];
    return (int)r.size();
}
extern "C" int settings(const char *skip, const char *var, const char *alts, int *on, unsigned *min_score, int *a, char *why, int cap)
{
    mvblank::Settings s;
    std::string w;
    const bool ok = mvblank::settings_from(skip, var, alts, s, w);
    *on = s.on; *min_score = s.min_score; *a = s.alternates;
    snprintf(why, (size_t)cap, "%s", w.c_str());
    return ok ? 1 : 0;
}
"""


@pytest.fixture(scope="module")
def policy_lib(tmp_path_factory):
    cxx = shutil.which("g++") or shutil.which("c++")
    if cxx is None:
        pytest.fail("no host C++ compiler")
    d = tmp_path_factory.mktemp("blank")
    src, so = d / "h.cpp", d / "libblank.so"
    src.write_text("#include <stdio.h>\n" + _HARNESS)
    subprocess.run([cxx, "-O2", "-std=c++17", "-shared", "-fPIC", "-I" + os.path.join(ROOT, "minivideo_amd", "csrc", "host"), str(src),
                    "-o", str(so)], check=True)
    lib = C.CDLL(str(so))
    lib.score.restype = C.c_uint32
    lib.score.argtypes = [C.c_uint64, C.c_uint64, C.c_uint32]
    lib.choose.argtypes = [C.POINTER(C.c_uint32), C.c_int, C.c_uint32]
    lib.alternates.argtypes = [C.POINTER(C.c_int), C.c_int, C.c_int, C.c_int, C.c_int, C.POINTER(C.c_int)]
    lib.settings.argtypes = [C.c_char_p, C.c_char_p, C.c_char_p, C.POINTER(C.c_int), C.POINTER(C.c_uint32), C.POINTER(C.c_int),
                             C.c_char_p, C.c_int]
    return lib


def _both(policy_lib, s, q, n):
    a, b = luma_score((s, q, n)), int(policy_lib.score(s, q, n))
    assert a == b
    return a


# ---- the score ----
def test_record_layout():
    assert C.sizeof(LumaStats) == 32 and LUMA_STATS_DTYPE.itemsize == 32 and L.STATS_DTYPE == LUMA_STATS_DTYPE
    assert LumaStats.sum.offset == 0 and LumaStats.sumsq.offset == 8 and LumaStats.samples.offset == 16


def test_known_scores(policy_lib):
    for v in (0, 1, 128, 255):                                    # a flat picture
        assert _both(policy_lib, *L.stats(np.full((18, 22), v, np.uint8), 0, 0, 22, 18)) == 0
    half = np.zeros((16, 32), np.uint8)
    half[:, 16:] = 255
    assert _both(policy_lib, *L.stats(half, 0, 0, 32, 16)) == 260100 == L.SCORE_MAX
    assert _both(policy_lib, 200, 200 * 200, 1) == 0             # a single sample
    n = 1 << 28
    assert _both(policy_lib, 255 * n, 255 * 255 * n, n) == 0     # all 255 at the largest rectangle: 16 N Q = 2^76 (the 128-bit path)
    assert _both(policy_lib, 255 * (n // 2), 255 * 255 * (n // 2), n) == 260100
    assert _both(policy_lib, 0, 0, 0) == 0 and _both(policy_lib, 5, 25, 0) == 0   # N = 0
    assert _both(policy_lib, 1 + 2, 1 + 4, 2) == 4               # samples 1, 2: variance 1/4 -> 4 sixteenths
    assert _both(policy_lib, 0 + 1 + 1, 2, 3) == 3               # variance 2/9 -> floor(32/9)
    assert luma_score(LumaStats(3, 5, 2)) == 4


def test_random_records_against_python_integers(policy_lib):
    rnd = random.Random(5)
    for _ in range(3000):
        n = rnd.choice([1, 2, 3, 255, 256, 65536, 1920 * 1080, (1 << 28) - 1, 1 << 28, rnd.randrange(1, 1 << 28)])
        if n <= 4096:
            v = [rnd.randrange(256) for _ in range(n)]
            s, q = sum(v), sum(x * x for x in v)
        else:                                                     # k samples of a, the rest of b: any two-level picture
            k, a, b = rnd.randrange(n + 1), rnd.randrange(256), rnd.randrange(256)
            s, q = k * a + (n - k) * b, k * a * a + (n - k) * b * b
        want = L.score(s, q, n)
        assert 0 <= want <= L.SCORE_MAX
        assert _both(policy_lib, s, q, n) == want, (s, q, n)


def test_restatement_on_planes():
    rng = np.random.default_rng(3)
    p = rng.integers(0, 256, (34, 50), dtype=np.uint8)
    s, q, n = L.stats(p, 6, 4, 18, 10)
    r = p[4:14, 6:24].astype(np.int64)
    assert (s, q, n) == (int(r.sum()), int((r * r).sum()), 180)
    assert L.score(s, q, n) == int(np.floor(16 * (n * q - s * s) / (n * n)))    # (small numbers: exact in float64)
    rec = L.record(p, 6, 4, 18, 10)
    assert rec.tobytes() == np.array([s, q], "<u8").tobytes() + np.array([n, 0, 0, 0], "<u4").tobytes()


# ---- the choice ----
CHOOSE = [([5, 20, 30], 10, 1), ([50, 20, 30], 10, 0), ([5, 7, 6], 10, 1), ([5, 7, 7], 10, 1), ([3, 3, 3], 10, 0), ([9], 10, 0),
          ([9, 10], 10, 1), ([0, 0], 0, 0), ([1, 2, 3, 2_000_000_000, 4_000_000_000], 4_000_000_000, 4)]


def test_choose(policy_lib):
    for scores, m, want in CHOOSE:
        arr = (C.c_uint32 * len(scores))(*scores)
        assert L.choose(scores, m) == blank_choose(scores, m) == policy_lib.choose(arr, len(scores), m) == want, (scores, m)
    assert L.choose([], 10) == blank_choose([], 10) == policy_lib.choose(None, 0, 10) == -1
    assert policy_lib.choose((C.c_uint32 * 1)(7), -3, 10) == -1
    rnd = random.Random(9)
    for _ in range(500):
        scores = [rnd.choice([0, 1, 99, 100, 101, 260100]) for _ in range(rnd.randrange(1, 18))]
        m = rnd.choice([0, 100, 101, 300000])
        assert L.choose(scores, m) == blank_choose(scores, m) == policy_lib.choose((C.c_uint32 * len(scores))(*scores), len(scores), m)


# ---- the alternates ----
ALTERNATES = [
    ([0, 1, 2], 10, 4, [[], [], [3, 4, 5, 6]]),                   # unfiltered, consecutive: only the last slot has any
    ([0, 1, 2], 3, 4, [[], [], []]),                              # ... and none at the end of the stream
    ([0, 5, 10], 18, 4, [[1, 2, 3, 4], [6, 7, 8, 9], [11, 12, 13, 14]]),   # distributed
    ([0, 5, 10], 18, 16, [[1, 2, 3, 4], [6, 7, 8, 9], [11, 12, 13, 14, 15, 16, 17]]),   # a larger than the gaps
    ([0, 2, 3], 5, 1, [[1], [], [4]]),
    ([0], 9, 4, [[1, 2, 3, 4]]),                                  # -n 1: the following a pictures
    ([3], 5, 4, [[4]]),                                           # the last slot close to the end
    ([4], 5, 4, [[]]),
    ([], 5, 4, []),
]


def test_alternates(policy_lib):
    for slots, n_idr, a, want in ALTERNATES:
        assert L.alternates(slots, n_idr, a) == want
        out = (C.c_int * 32)()
        arr = (C.c_int * max(1, len(slots)))(*slots)
        got = [list(out[:policy_lib.alternates(arr, len(slots), n_idr, a, k, out)]) for k in range(len(slots))]
        assert got == want, (slots, n_idr, a)
    assert policy_lib.alternates((C.c_int * 1)(0), 1, 9, 4, 5, (C.c_int * 32)()) == 0     # no such slot


def test_policy_restatement():
    scores = [5, 7, 900, 3, 2, 800, 1, 1, 1, 6]
    assert L.policy([0], scores, 100, 4) == ([2], [1, 2, 3, 4])                   # blank, blank, busy
    assert L.policy([0], scores, 100, 1) == ([1], [1])                            # one alternate only: the better blank
    assert L.policy([0], [5, 7, 7, 3], 100, 4) == ([1], [1, 2, 3])                # none busy: the highest, the earliest
    assert L.policy([2, 5], scores, 100, 4) == ([2, 5], [])                       # nothing blank: no second pass
    assert L.policy([0, 1, 6], scores, 100, 4) == ([0, 2, 9], [2, 3, 4, 5, 7, 8, 9])   # slot 0 has no alternate: it keeps its blank
    assert L.policy([6, 7, 8], scores, 100, 4) == ([6, 7, 9], [9])                # consecutive slots: only the last one has any
    assert L.policy([0, 3, 6], scores, 100, 4) == ([2, 5, 9], [1, 2, 4, 5, 7, 8, 9])


# ---- the switches ----
def _settings(policy_lib, skip, var, alts):
    on, ms, a, why = C.c_int(), C.c_uint32(), C.c_int(), C.create_string_buffer(256)
    enc = [None if v is None else v.encode() for v in (skip, var, alts)]
    ok = policy_lib.settings(*enc, C.byref(on), C.byref(ms), C.byref(a), why, 256)
    return ok, on.value, ms.value, a.value, why.value.decode()


def test_settings(policy_lib):
    assert _settings(policy_lib, None, None, None) == (1, 0, 16 * 256, 4, "")
    assert _settings(policy_lib, "1", None, None) == (1, 1, 16 * 256, 4, "")
    assert _settings(policy_lib, "0", "1000", "16") == (1, 0, 16000, 16, "")
    assert _settings(policy_lib, "1", "0", "1") == (1, 1, 0, 1, "")
    assert _settings(policy_lib, "1", "16256", "7") == (1, 1, 16 * 16256, 7, "")
    for var, bad in [("MINIVIDEO_BLANK_VARIANCE", v) for v in ("abc", "-1", "16257", "1 ", " 1", "1.5", "0x10", "99999999999")] + \
                    [("MINIVIDEO_BLANK_ALTERNATES", v) for v in ("abc", "-1", "0", "17", "4x")] + \
                    [("MINIVIDEO_SKIP_BLANK", v) for v in ("abc", "2", "-1", "yes")]:
        args = {"MINIVIDEO_SKIP_BLANK": "1", "MINIVIDEO_BLANK_VARIANCE": None, "MINIVIDEO_BLANK_ALTERNATES": None}
        args[var] = bad
        ok, _, _, _, why = _settings(policy_lib, args["MINIVIDEO_SKIP_BLANK"], args["MINIVIDEO_BLANK_VARIANCE"],
                                     args["MINIVIDEO_BLANK_ALTERNATES"])
        assert ok == 0 and var in why and "'%s'" % bad in why, (var, bad, why)


@pytest.mark.parametrize("var,bad", [("MINIVIDEO_BLANK_VARIANCE", "abc"), ("MINIVIDEO_BLANK_VARIANCE", "-1"),
                                     ("MINIVIDEO_BLANK_VARIANCE", "16257"), ("MINIVIDEO_BLANK_ALTERNATES", "0"),
                                     ("MINIVIDEO_BLANK_ALTERNATES", "17"), ("MINIVIDEO_BLANK_ALTERNATES", "abc")])
def test_malformed_values_fail_the_call_before_any_device_work(tmp_path, var, bad):
    stream, _ = gen.make_stream(2, 2, 2, seed=5, profile="baseline", dense=True, want_packed=False)
    stream.tofile(tmp_path / "c.264")
    env = {k: v for k, v in os.environ.items() if not k.startswith("MINIVIDEO_")}
    env.update({"MINIVIDEO_SKIP_BLANK": "1", var: bad})
    r = subprocess.run([CLI, "-i", str(tmp_path / "c.264"), "-f", "yuv420", "-n", "2"], cwd=tmp_path, capture_output=True, text=True,
                       timeout=60, env=env)
    assert var in r.stderr and "'%s'" % bad in r.stderr and "decode did not succeed" in r.stderr, r.stdout + r.stderr
    assert "hip" not in r.stderr.lower() and "device" not in r.stderr.lower(), r.stderr
    assert sorted(os.listdir(tmp_path)) == ["c.264"]


def test_tiled_reference_of_the_split_launch_test():
    """tests/test_gpu_launch_splits.py computes the records of 4099 base pictures and tiles them: the same bytes as the direct
    reference on the first 300 pictures and across the wrap; 16 one-row bands put one picture more than a launch holds at
    524 289"""
    from tests import test_gpu_launch_splits as X
    base, rec = X.stats_case()
    n = X.STATS_CYCLE + 11
    yuv, want = X.tiled(base, n, X.STATS_CYCLE), X.tiled(rec, n, X.STATS_CYCLE)
    assert L.records(yuv[:300], 300, 1, 1, X.STATS_RECT).tobytes() == want[:300].tobytes()
    assert L.records(yuv[-30:], 30, 1, 1, X.STATS_RECT).tobytes() == want[-30:].tobytes()
    assert len({r.tobytes() for r in rec}) == X.STATS_CYCLE
    assert X.STATS_RECT[3] * X.STATS_PER_LAUNCH == 1 << 23
