#!/usr/bin/env python3
"""What the inputs of the older test files reach, by the content census (tests/recon_census.py).  CPU only, a report, nothing is
asserted:   python tools/census_report.py [--large]

Corpora: the records of tests/refcorpus.py (the front end's output for the reference corpus), the grid of tests/test_spec_model.py,
the synth_packed calls of tests/test_gpu_parity.py and those of tests/test_gpu_recon_buffers.py -- and, for comparison, the directed
corpus of tests/recon_directed.py.  Pictures of more than 2000 macroblocks are left out unless --large is given (they add minutes and,
being drawn like the small ones, few cells).

Per corpus: the macroblock cells with a position against the universe of a shape that has every column and row class (9 x 9 and 1 x 9
at four rows per band), the cells without a position, and the wave cells for groups of eight, of four and for macroblock pairs;
the wave cells of full groups that are missed are listed by name."""
import os
import sys
from collections import Counter

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from minivideo_amd.synth import synth_packed          # noqa: E402
from tests import recon_census as RC                  # noqa: E402

LARGE = "--large" in sys.argv


def refcorpus_batches():
    from tests import refcorpus
    from tests.util import Stream
    for case in refcorpus.CORPUS:
        if case["width_mbs"] * case["height_mbs"] > 2000 and not LARGE:
            continue
        stream, packed = refcorpus.make(case)
        with Stream(stream) as s:
            yield s.params(0), np.asarray(packed).reshape(case["n_frames"], -1, 800)


def spec_grid_batches():
    from tests import spec_synth as S
    from tests import test_spec_model as T
    for mi in range(len(S.SLICE_MAPS)):
        for si in range(len(T.SIZES)):
            for p, rec, ids, cls in T.grid_case(mi, si):
                yield p, rec


def gpu_parity_batches():
    for W, H in [(1, 1), (2, 1), (1, 2), (3, 2), (5, 3), (11, 9), (20, 17), (64, 5), (7, 35)]:
        for profile in ("baseline", "high"):
            yield synth_packed(W, H, 3, seed=W * 100 + H, profile=profile, density="dense")
    for waves in (1, 2, 4, 8, 16):
        yield synth_packed(23, 37, 5, seed=waves, profile="high", density="dense")
    yield synth_packed(30, 20, 4, seed=5, density="light")
    for qr in [(0, 12), (13, 23), (24, 35), (36, 51)]:
        yield synth_packed(12, 7, 2, seed=qr[0], profile="high", qp_range=qr, cqp_offsets=(3, -5))
    for off in [(-12, 12), (12, -12)]:
        yield synth_packed(9, 6, 2, seed=77, profile="high", qp_range=(0, 51), cqp_offsets=off)
    yield synth_packed(10, 6, 3, seed=9, profile="high", illegal_modes=True)
    yield synth_packed(10, 6, 2, seed=10, qp_range=(36, 36), allow_qp36_i16=True)
    yield synth_packed(8, 8, 2, seed=11, profile="high", qp_range=(0, 51))     # (test_large_levels, before it enlarges the levels)
    yield synth_packed(40, 30, 6, seed=21, profile="high")
    if LARGE:
        yield synth_packed(120, 68, 2, seed=1080, profile="baseline", density="dense")
        yield synth_packed(120, 68, 17, seed=1081, profile="baseline", density="dense")
        yield synth_packed(240, 135, 1, seed=2160, profile="high", density="dense")
    rng = np.random.default_rng(2024)                                             # test_random_configurations
    for _ in range(40):
        W, H, n = int(rng.integers(1, 30)), int(rng.integers(1, 30)), int(rng.integers(1, 11))
        lo = int(rng.integers(0, 40))
        hi = int(rng.integers(lo, 52))
        rng.integers(0, 6)
        yield synth_packed(W, H, n, seed=int(rng.integers(0, 1 << 30)), profile=["baseline", "high"][int(rng.integers(0, 2))],
                           density=["dense", "light"][int(rng.integers(0, 2))], qp_range=(lo, hi),
                           cqp_offsets=(int(rng.integers(-12, 13)), int(rng.integers(-12, 13))),
                           illegal_modes=bool(rng.random() < 0.2), allow_qp36_i16=bool(rng.random() < 0.5))
        rng.integers(0, 2)


def recon_buffers_batches():
    from tests import recon_buffers as B
    for (W, H) in dict.fromkeys(B.SHAPES + B.BAND_SHAPES):
        for profile in ("baseline", "high"):
            params, rec = synth_packed(W, H, max(B.COUNTS), seed=1000 * W + 10 * H + len(profile), profile=profile, density="dense")
            for n in B.COUNTS:            # the test launches the first 1, 3, 5 and 9 pictures: four different sets of groups
                yield params, rec[:n]


def directed_batches():
    from tests import recon_directed as D
    for b in D.corpus("parity"):
        yield b.params, b.rec


CORPORA = (("tests/refcorpus.py", refcorpus_batches), ("tests/test_spec_model.py grid", spec_grid_batches),
           ("tests/test_gpu_parity.py", gpu_parity_batches), ("tests/test_gpu_recon_buffers.py", recon_buffers_batches),
           ("tests/recon_directed.py (parity)", directed_batches))


def survey(batches):
    """cells reached: positional (rows per band 4), without a position, wave cells per group size; spec-mode batches are
    surveyed as what they are (a spec-mode picture has no "zero" cells)"""
    pos, free, waves, n = set(), set(), {1: set(), 4: set(), 8: set()}, 0
    for params, rec in batches:
        rec = np.asarray(rec)
        p, f = RC.raw_cells(params, rec)
        pos |= RC.classed(p, int(params.width_mbs), 4)
        free |= f
        for g in waves:
            waves[g] |= RC.wave_cells(params, rec, g)
        n += rec.shape[0]
    return pos, free, waves, n


def main():
    upos = RC.positional_universe("parity", 9, 9, 4) | RC.positional_universe("parity", 1, 9, 4)
    for name, make in CORPORA:
        pos, free, waves, n = survey(make())
        print("## %s: %d pictures" % (name, n))
        print("  positional cells      %5d of %5d, missed %5d" % (len(pos & upos), len(upos), len(upos - pos)))
        by = Counter(t[0] for t in upos - pos)
        print("      missed by kind: " + ", ".join("%s %d" % kv for kv in sorted(by.items())))
        by = Counter((t[1], t[2]) for t in upos - pos if t[0] != "zero")
        print("      missed by class: " + ", ".join("%s/%s %d" % (k[0], k[1], v) for k, v in sorted(by.items())))
        for g in (8, 4, 1):
            u = RC.free_universe("parity", g)
            got = free | waves[g]
            miss = u - got
            qp = [t for t in miss if t[0] in ("qp", "qpc", "qpi_clip")]
            print("  group %d: cells without a position %4d of %4d, missed %4d (of them QP / QPc / clip: %d)" % (
                g, len(u & got), len(u), len(miss), len(qp)))
            full = sorted((t for t in miss if t[0] in ("wave", "wave2", "pair") and t[3] == "full"), key=repr)
            short = [t for t in miss if t[0] in ("wave", "wave2", "pair") and t[3] != "full"]
            print("      missed wave cells of full groups (%d): %s" % (len(full), "; ".join(
                "%s %s%s" % (t[1], t[2], "" if t[0] == "wave2" or t[4] is None else " at %d" % t[4]) for t in full) or "none"))
            print("      missed wave cells of short last groups: %d" % len(short))
        print()


if __name__ == "__main__":
    main()
