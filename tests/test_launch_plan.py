"""CPU: the launch planner (csrc/hip/launch_plan.hip behind mvhp_plan_launch) -- which of the seven kernel forms a batch runs on
and with how many waves, as pure arithmetic on a DESCRIBED device: no GPU, nothing launched.

* golden/launch_plan.json pins the policy: dumped from a build in which pick_layout / pick_waves had only been moved out of
  hotpath_abi.hip, before the form table existed (golden/make_launch_plan.py says what is sampled: 64 / 256 / 304 CUs, 64 and
  160 KiB of LDS and less, widths 1 .. 1024, every forced layout and wave count, batch sizes on both sides of every threshold).
  A row that no longer reproduces is a changed choice: either a bug, or a deliberate retuning that regenerates the table.
* known answers that do not come from the planner: the forms the GPU tests assert on a 256-CU MI355X (test_gpu_wide.py,
  test_gpu_configs.py), here for a described device of 256 CUs and 160 KiB of LDS.
* malformed arguments are refused."""
import ctypes as C
import json
import os

import pytest

from minivideo_amd import hotpath
from minivideo_amd.hotpath import LAYOUTS, PlanDevice, StreamParams, plan_launch

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "launch_plan.json")
MI355X = (256, 160 * 1024)   # CUs, LDS bytes per CU


def test_golden_table_reproduces():
    doc = json.load(open(GOLDEN))
    assert doc["columns"] == ["n_cus", "max_lds", "width_mbs", "height_mbs", "flags", "forced_layout", "forced_waves", "n_frames",
                              "layout", "waves"]
    rows = doc["rows"]
    assert len(rows) >= 3000
    bad = []
    for (cus, lds, w, h, flags, lay, nw, n, want_layout, want_waves) in rows:
        got = plan_launch(PlanDevice(cus, lds, lay, nw), StreamParams(w, h, 0, 0, flags), n)
        if got != (LAYOUTS[want_layout], want_waves):
            bad.append(((cus, lds, w, h, flags, lay, nw, n), (LAYOUTS[want_layout], want_waves), got))
    assert not bad, (len(bad), bad[:10])
    # the sample itself: every form chosen automatically, every form forced, every wave count each form is built for
    assert {r[8] for r in rows if r[5] == 0} == set(range(1, 8)) and {r[5] for r in rows} == set(range(8))
    built = {"rows": {4, 8, 16}, "quad": {4, 6, 8, 12, 16}, "oct": {4, 6, 8}, "wide": {4}, "quad_wide": {4, 8}, "pipe": {1, 2, 4},
             "pipe1": {1, 2, 4}}
    for name, waves in built.items():
        assert {r[9] for r in rows if LAYOUTS[r[8]] == name} == waves, name


# (width, height, pictures, flags, form): tests/test_gpu_wide.py::test_automatic_choice_by_batch_size
ON_256_CUS = [(20, 17, 1, 0, "pipe"), (20, 17, 2, 0, "pipe1"), (20, 17, 3, 1, "pipe1"), (20, 17, 4, 1, "pipe1"), (20, 17, 4, 0, "pipe1"),
              (20, 17, 271, 0, "pipe1"), (20, 17, 272, 0, "pipe"), (20, 17, 512, 0, "pipe"), (20, 17, 513, 0, "quad_wide"),
              (20, 68, 67, 0, "pipe1"), (20, 68, 68, 0, "pipe"), (20, 68, 286, 0, "pipe"), (20, 68, 287, 0, "quad_wide"),
              (20, 68, 173, 1, "pipe1"), (20, 68, 174, 1, "wide"), (20, 68, 286, 1, "wide"), (20, 68, 287, 1, "quad_wide"),
              (6, 68, 860, 0, "quad_wide"), (6, 68, 861, 0, "quad")]
# ... and tests/test_gpu_configs.py::test_full_hd_batches_on_the_automatic_layout (120 x 68 Baseline)
ON_256_CUS += [(120, 68, n, 0, form) for (n, form) in [(1, "pipe"), (2, "pipe1"), (40, "pipe1"), (64, "pipe1"), (128, "pipe"),
                                                        (512, "quad_wide"), (1024, "quad"), (1100, "quad_wide"), (2048, "oct"),
                                                        (2080, "quad_wide")]]


@pytest.mark.parametrize("w,h,n,flags,form", ON_256_CUS)
def test_what_the_gpu_tests_assert_on_256_cus(w, h, n, flags, form):
    got = plan_launch(PlanDevice(MI355X[0], MI355X[1], 0, 0), StreamParams(w, h, 0, 0, flags), n)
    assert got is not None and got[0] == form, got


def test_malformed_arguments_are_refused():
    L = hotpath.lib()
    dev, ok = PlanDevice(MI355X[0], MI355X[1], 0, 0), StreamParams(20, 17, 0, 0, 0)
    lay, nw = C.c_int(-1), C.c_int(-1)

    def call(ctx, d, p, n=4):
        return L.mvhp_plan_launch(ctx, C.byref(d) if d is not None else None, C.byref(p), n, C.byref(lay), C.byref(nw))

    assert call(None, dev, ok) == hotpath.SUCCESS and (LAYOUTS[lay.value], nw.value) == ("pipe1", 4)
    assert call(None, None, ok) == hotpath.FAILURE                                     # neither a context nor a device
    assert call(C.c_void_p(1), dev, ok) == hotpath.FAILURE                             # both (refused before either is read)
    assert call(None, dev, StreamParams(0, 17, 0, 0, 0)) == hotpath.FAILURE
    assert call(None, dev, StreamParams(1025, 17, 0, 0, 0)) == hotpath.FAILURE
    assert call(None, dev, StreamParams(20, 17, 13, 0, 0)) == hotpath.FAILURE
    assert call(None, dev, ok, n=0) == hotpath.FAILURE
    assert call(None, PlanDevice(MI355X[0], MI355X[1], 8, 0), ok) == hotpath.FAILURE   # no such layout
    assert plan_launch(dev, StreamParams(20, 0, 0, 0, 0), 4) is None
