"""CPU: the decode engine with MVHP_OUTPUT_SCORE on the stub device of tools/engine_harness.cpp, under ThreadSanitizer and
AddressSanitizer.  The harness's score mode (a fifth argument "score" behind the geometry mode's stream; the stub's picture-score
operation sums the stub's coded planes on the CPU) checks, with one to three contexts, small and large batches, for planes, RGB,
RGB only and the JPEG operation, at the coded size, cropped and boxed:
  * g->reserved[1] of every delivered picture is the score of the stub's planes over the geometry's rectangle, the pictures and
    reserved[0] are what they are without the flag, and a failed batch that is re-queued is scored again with the same result;
  * without the flag reserved[1] is 0 and the operation is never called;
  * d2h_bytes is exactly 32 per picture of a downloaded batch more than without the flag, and a request with the flag alone runs
    no geometry launch;
  * a device table without the operation fails every picture of such a call with a message, before anything is launched;
  * each malformed MINIVIDEO_SKIP_BLANK / _BLANK_VARIANCE / _BLANK_ALTERNATES value makes minivideo_decode return FAILURE with a
    message before a device context exists.
The existing modes run first in the same process and must still pass."""
import os
import subprocess

import pytest

from tests.test_engine_harness import _build
from tests.test_engine_harness_geometry import _streams


@pytest.mark.parametrize("sanitize", ["thread", "address,undefined"])
def test_engine_harness_score(tmp_path, sanitize):
    _streams(tmp_path)
    exe = _build(tmp_path, sanitize)
    env = dict(os.environ, TSAN_OPTIONS="halt_on_error=1", ASAN_OPTIONS="detect_leaks=1")
    for k in ("MINIVIDEO_CROP", "MINIVIDEO_THUMBNAIL", "MINIVIDEO_WRITERS", "MINIVIDEO_JPEG", "MINIVIDEO_SKIP_BLANK",
              "MINIVIDEO_BLANK_VARIANCE", "MINIVIDEO_BLANK_ALTERNATES"):
        env.pop(k, None)
    r = subprocess.run([str(exe), str(tmp_path / "a.264"), str(tmp_path / "b.264"), "4", str(tmp_path / "c.264"), "score"],
                       capture_output=True, text=True, timeout=600, env=env)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "SCORE MODE DONE" in r.stdout and "HARNESS OK" in r.stdout, r.stdout + r.stderr
    assert r.stdout.count("score: table without it") == 2 and r.stdout.count("malformed blank switch") == 6
    assert "ThreadSanitizer" not in r.stderr and "AddressSanitizer" not in r.stderr and "runtime error" not in r.stderr, r.stderr
