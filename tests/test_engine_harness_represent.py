"""CPU: the decode engine with MVHP_OUTPUT_HIST on the stub device of tools/engine_harness.cpp, under ThreadSanitizer and
AddressSanitizer.  The harness's hist mode (a fifth argument "hist" behind the geometry mode's stream; the stub's plane-histogram
operation counts the stub's coded planes on the CPU) checks, with one to three contexts, small and large batches, for planes, RGB,
RGB only and the JPEG operation, at the coded size, cropped and boxed, with the flag alone and beside MVHP_OUTPUT_SCORE:
  * mvhp_engine_picture_hist inside the sink call is the picture's own record -- the counts of the stub's planes over the
    geometry's rectangle, 16-byte aligned -- and its mvhp_hist_stats score is the score MVHP_OUTPUT_SCORE delivers; it is NULL for
    every other picture, for failed pictures, without the flag and once the call is over; a picture the sink keeps stays readable
    until it is released, and is NULL from then on;
  * the pictures, g->reserved[] and the sink's arguments are what they are without the flag, and a failed batch that is re-queued
    is counted again with the same result;
  * d2h_bytes is exactly 3104 per picture of a downloaded batch more than without the flag (3136 beside the score), one
    operation runs behind every launch, none without the flag, and a request with the flag alone runs no geometry launch;
  * a device table without the operation fails every picture of such a call with a message, before anything is launched;
  * MVHP_OUTPUT_HIST with MVHP_OUTPUT_BARS is refused with a message, before anything is launched.
Through the public API (minivideo_decode under MINIVIDEO_REPRESENTATIVE=1) on the stub, whose histograms are functions of the
records' checksum and the rectangle, so that the harness computes every slot's winner itself with the policy header:
  * the three passes run: the order lists of passes 2 and 3 (MINIVIDEO_STATS) are the predicted ones, every file starts with its
    winner's checksum, no .part file stays, and a call in which every picture is a slot lists no candidate and replaces nothing;
  * MINIVIDEO_BATCH=1, three contexts and the writer pool give the same lists and files;
  * under MINIVIDEO_CROP, with an SPS crop that changes from picture to picture, candidates of another size are left out, and an
    alternate whose geometry cannot be formed is skipped;
  * with MINIVIDEO_SKIP_BLANK=1 as well only candidates at or above the threshold are compared, a slot whose candidates are all
    blank goes to the blank rule, blank skipping's own pass is not run and no picture-score operation is launched;
  * each malformed MINIVIDEO_REPRESENTATIVE / _REPRESENTATIVE_ALTERNATES value makes minivideo_decode return FAILURE with a
    message before a device context exists, whether or not the feature is on.
The existing modes run first in the same process and must still pass."""
import os
import subprocess

import pytest

from tests.test_engine_harness import _build
from tests.test_engine_harness_geometry import _streams

_SWITCHES = ("MINIVIDEO_CROP", "MINIVIDEO_THUMBNAIL", "MINIVIDEO_WRITERS", "MINIVIDEO_JPEG", "MINIVIDEO_SKIP_BLANK",
             "MINIVIDEO_BLANK_VARIANCE", "MINIVIDEO_BLANK_ALTERNATES", "MINIVIDEO_REPRESENTATIVE",
             "MINIVIDEO_REPRESENTATIVE_ALTERNATES", "MINIVIDEO_BATCH", "MINIVIDEO_FAKE_GPUS", "MINIVIDEO_STATS")


@pytest.mark.parametrize("sanitize", ["thread", "address,undefined"])
def test_engine_harness_hist(tmp_path, sanitize):
    _streams(tmp_path)
    exe = _build(tmp_path, sanitize)
    env = dict(os.environ, TSAN_OPTIONS="halt_on_error=1", ASAN_OPTIONS="detect_leaks=1")
    for k in _SWITCHES:
        env.pop(k, None)
    r = subprocess.run([str(exe), str(tmp_path / "a.264"), str(tmp_path / "b.264"), "4", str(tmp_path / "c.264"), "hist"],
                       capture_output=True, text=True, timeout=600, env=env)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "HIST MODE DONE" in r.stdout and "HARNESS OK" in r.stdout, r.stdout + r.stderr
    out = r.stdout
    assert out.count("hist: flag off") == 36 and out.count("hist: table without it") == 2 and out.count("hist with bars") == 1
    assert out.count("hist coded size") == out.count("hist crop") == out.count("hist box") == 24
    assert out.count("public API, representative") == 10 and out.count("malformed representative switch") == 5
    assert "ThreadSanitizer" not in r.stderr and "AddressSanitizer" not in r.stderr and "runtime error" not in r.stderr, r.stderr
