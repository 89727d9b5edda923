"""CPU: the decode engine under MVHP_OUTPUT_ORIENT / MVHP_OUTPUT_ROTATE on the stub device of tools/engine_harness.cpp, under
ThreadSanitizer and AddressSanitizer.  The harness's orient mode (a fifth argument "orient" behind the geometry mode's stream)
checks, at 1 to 3 quarter turns, alone, cropped and boxed, for planes, RGB and RGB only:
  * every delivered geometry is what mvhp_output_geometry announces for the request, the output buffers hold n pictures of it
    (the stub fills them to their last byte) and d2h_bytes is the sum of the delivered sizes;
  * every batch of a call that turns runs the turn and counts in geometry_launches; the buffer of the unturned planes exists
    exactly in the batches that scale before the turn;
  * turns that come to 0 run no turn, no extra buffer and -- at the coded size -- no geometry launch, and give the launches and
    bytes of the request without the flags;
  * a failed batch is re-queued with its turn; JPEG files are made of the turned pictures;
  * a device table without the operation fails every picture of a call that turns, with a message;
  * MINIVIDEO_ROTATE=90 / 180 / 270 writes files of the turned size, auto / 0 / the empty string are today's files, and 45, 90x
    and other malformed values make minivideo_decode return FAILURE with a message before a device context exists.
The existing modes run first in the same process and must still pass."""
import os
import subprocess

import pytest

from tests.test_engine_harness import _build
from tests.test_engine_harness_geometry import _streams


@pytest.mark.parametrize("sanitize", ["thread", "address,undefined"])
def test_engine_harness_orient(tmp_path, sanitize):
    _streams(tmp_path)
    exe = _build(tmp_path, sanitize)
    env = dict(os.environ, TSAN_OPTIONS="halt_on_error=1", ASAN_OPTIONS="detect_leaks=1")
    for k in ("MINIVIDEO_CROP", "MINIVIDEO_THUMBNAIL", "MINIVIDEO_WRITERS", "MINIVIDEO_JPEG", "MINIVIDEO_SKIP_BLANK",
              "MINIVIDEO_BLANK_VARIANCE", "MINIVIDEO_BLANK_ALTERNATES", "MINIVIDEO_ROTATE"):
        env.pop(k, None)
    r = subprocess.run([str(exe), str(tmp_path / "a.264"), str(tmp_path / "b.264"), "4", str(tmp_path / "c.264"), "orient"],
                       capture_output=True, text=True, timeout=600, env=env)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "ORIENT MODE DONE" in r.stdout and "HARNESS OK" in r.stdout, r.stdout + r.stderr
    assert r.stdout.count("malformed rotation") == 6 and r.stdout.count("public API, orientation") == 12
    assert "orient: table without it" in r.stdout and "orient requeue/3ctx" in r.stdout
    assert "ThreadSanitizer" not in r.stderr and "AddressSanitizer" not in r.stderr and "runtime error" not in r.stderr, r.stderr
