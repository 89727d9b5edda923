"""Writes launch_plan.json: what mvhp_plan_launch answers for a sample of {device, forced settings, picture shape, batch size}.

The committed table was dumped from a build in which pick_layout / pick_waves had only been MOVED out of hotpath_abi.hip (the
context's fields replaced by the PlanDevice's, nothing else), before the form table and plan_launch were written: it pins the
policy as it was.  Run it again only to EXTEND the sample, from a library whose answers for the existing rows are unchanged
(tests/test_launch_plan.py says so), or after a deliberate change of a threshold.

usage: python tests/golden/make_launch_plan.py [libminivideo.so]"""
import functools
import itertools
import json
import os
import random
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))
if len(sys.argv) > 1:
    os.environ["MINIVIDEO_LIB"] = os.path.abspath(sys.argv[1])
from minivideo_amd import hotpath  # noqa: E402

CUS = (64, 256, 304)
LDS = (65536, 160 * 1024)
WIDTHS = (1, 5, 20, 120, 160, 161, 240, 1024)
HEIGHTS = (1, 3, 4, 17, 68, 135)
FLAGS = (0, hotpath.PARAM_MAY_HAVE_8X8, hotpath.PARAM_SLICES, hotpath.PARAM_SCALING)
LAYOUTS = range(8)
WAVES = (0, 1, 2, 4, 6, 8, 12, 16)


@functools.lru_cache(maxsize=None)
def batch_sizes(cus, w, h, may8):
    """both sides of every threshold of the planner, in pictures"""
    wide_rows = max(0.0, (w - 120.0) / 120.0)
    qw_share = min(0.84, max(0.60, 0.84 - (0.19 if may8 else 0.06) * wide_rows))
    edges = [k * cus / h for k in (18, 34, 40, 46, 76)]                       # row-waves
    edges += [k * cus for k in (0.44, 1.15, 1.2, 1.5, 2, 3.4, 4, 8, 12, 16)]   # pictures (4 / 8 x CUs: rounds of the batch kernels)
    edges += [qw_share * 4 * cus, 383.5, 8 * cus - 3.5]                       # ... 384 pictures, 2 x CUs groups of four
    ns = {1, 2, 3, 5, 300, 1100, 2048, 2080, 2560}
    for e in edges:
        ns |= {int(e), int(e) + 1}
    t = 4 * cus + 1                                                          # the round model: where its choice changes
    prev = None
    while t <= 16 * cus:
        got = hotpath.plan_launch(hotpath.PlanDevice(cus, 160 * 1024, 0, 0), hotpath.StreamParams(w, h, 0, 0, int(may8)), t)
        if prev is not None and got != prev:
            ns |= {t - 1, t}
        prev = got
        t += 1
    return sorted(n for n in ns if n >= 1)


def main():
    rng = random.Random(20250)
    cases = set()
    # the automatic choice: every batch size on the usual shapes, a sample of the whole product
    for cus, w, h, fl in itertools.product(CUS, (20, 120, 240), (17, 68, 135), (0, 1)):
        cases |= {(cus, LDS[1], w, h, fl, 0, 0, n) for n in batch_sizes(cus, w, h, fl & 1)}
    prod = list(itertools.product(CUS, LDS, WIDTHS, HEIGHTS, FLAGS))
    for cus, lds, w, h, fl in prod:
        for n in rng.sample(batch_sizes(cus, w, h, fl & 1), 1):
            cases.add((cus, lds, w, h, fl, 0, 0, n))
    # forced layouts and waves: a sample of the whole product
    for _ in range(2000):
        cus, lds, w, h, fl = rng.choice(prod)
        cases.add((cus, lds, w, h, fl, rng.choice(LAYOUTS), rng.choice(WAVES), rng.choice(batch_sizes(cus, w, h, fl & 1))))
    # line buffers that do not fit in 64 KiB: every fallback of every forced form
    for w, h, fl, lay, nw, n in itertools.product((161, 240, 1024), (3, 68), (0, 1, 4), LAYOUTS, (0, 8), (1, 5, 300, 2100)):
        cases.add((256, LDS[0], w, h, fl, lay, nw, n))
    # ... and devices with less LDS than any real one: the fallbacks of pipe and pipe1, whose buffers fit 64 KiB at every width
    for lds, w, fl, lay, n in itertools.product((16384, 32768, 49152), (240, 1024), (0, 1, 4), LAYOUTS, (1, 5, 300, 2100)):
        cases.add((256, lds, w, 68, fl, lay, 0, n))
    # the macroblock caps of oct (2^19) and pipe / quad_wide (2^20; out of reach below 1025 x 1025): pictures whose line
    # buffers would fit a (hypothetical) 1 MiB of LDS
    for h, lay, n in itertools.product((512, 513, 1024), (0, 3, 5, 6), (1, 5, 2100)):
        cases.add((256, 1 << 20, 1024, h, 0, lay, 0, n))
    rows = []
    for (cus, lds, w, h, fl, lay, nw, n) in sorted(cases):
        got = hotpath.plan_launch(hotpath.PlanDevice(cus, lds, lay, nw), hotpath.StreamParams(w, h, 0, 0, fl), n)
        rows.append([cus, lds, w, h, fl, lay, nw, n, hotpath.LAYOUTS.index(got[0]), got[1]])
    doc = {"columns": ["n_cus", "max_lds", "width_mbs", "height_mbs", "flags", "forced_layout", "forced_waves", "n_frames",
                       "layout", "waves"], "rows": rows}
    with open(os.path.join(HERE, "launch_plan.json"), "w") as f:
        f.write(json.dumps(doc, separators=(",", ":")).replace("],[", "],\n[") + "\n")
    print(len(rows), "rows")


if __name__ == "__main__":
    main()
