"""CPU: the decode engine with MVHP_OUTPUT_BARS and MVHP_OUTPUT_TRIM on the stub device of tools/engine_harness.cpp, under
ThreadSanitizer and AddressSanitizer.  The harness's bars mode (a fifth argument "bars" behind the geometry mode's stream; the
stub's black-bar operation gives every picture a box of its own, a function of its records) checks, with one to three contexts,
small and large batches and a failed batch re-queued, for planes, RGB and RGB only, at the coded size, cropped and boxed:
  * every launch of such a call carries `bars` and the level of the request (0 means 24);
  * g->reserved[0] / [1] of every delivered picture are x | y << 16 and w | h << 16 of that picture's own box, the pictures are
    what they are without the flag, and without the flag both words are 0 and the operation is never called;
  * d2h_bytes is exactly 32 per picture of a downloaded batch more than without the flag, and a request with the flag alone runs
    no geometry launch;
  * a device table without CAP_BARS fails every picture of such a call with a message, before anything is launched;
  * the flag is refused, with a message and before any work, together with MVHP_OUT_JPEG, MVHP_OUT_PNG, MVHP_OUTPUT_SCORE and
    with the plain sink;
  * a call with MVHP_OUTPUT_TRIM and a box set on the stream launches the geometry with the trimmed rectangle; without a box the
    flag is MVHP_OUTPUT_CROP, and a box without the flag changes nothing;
  * minivideo_decode under MINIVIDEO_TRIM=1 runs its probe call and its decode call on one engine and writes the right pictures;
    each malformed MINIVIDEO_TRIM / _TRIM_LEVEL / _TRIM_PROBES value makes it return FAILURE with a message before a device
    context exists.
The existing modes run first in the same process and must still pass."""
import os
import subprocess

import pytest

from tests.test_engine_harness import _build
from tests.test_engine_harness_geometry import _streams


@pytest.mark.parametrize("sanitize", ["thread", "address,undefined"])
def test_engine_harness_bars(tmp_path, sanitize):
    _streams(tmp_path)
    exe = _build(tmp_path, sanitize)
    env = dict(os.environ, TSAN_OPTIONS="halt_on_error=1", ASAN_OPTIONS="detect_leaks=1")
    for k in ("MINIVIDEO_CROP", "MINIVIDEO_THUMBNAIL", "MINIVIDEO_WRITERS", "MINIVIDEO_JPEG", "MINIVIDEO_PNG", "MINIVIDEO_SKIP_BLANK",
              "MINIVIDEO_TRIM", "MINIVIDEO_TRIM_LEVEL", "MINIVIDEO_TRIM_PROBES"):
        env.pop(k, None)
    r = subprocess.run([str(exe), str(tmp_path / "a.264"), str(tmp_path / "b.264"), "4", str(tmp_path / "c.264"), "bars"],
                       capture_output=True, text=True, timeout=600, env=env)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "BARS MODE DONE" in r.stdout and "HARNESS OK" in r.stdout, r.stdout + r.stderr
    assert r.stdout.count("bars: table without it") == 2 and r.stdout.count("malformed trim switch") == 6
    assert r.stdout.count("message: MVHP_OUTPUT_BARS") == 4
    assert "ThreadSanitizer" not in r.stderr and "AddressSanitizer" not in r.stderr and "runtime error" not in r.stderr, r.stderr
