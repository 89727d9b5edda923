"""CPU: the decode engine with MVHP_OUT_PNG on the stub device of tools/engine_harness.cpp, under ThreadSanitizer and
AddressSanitizer.  The harness's PNG mode (a fifth argument "png" behind the geometry mode's stream) checks, with one to three
contexts, small and large batches and a failed batch re-queued:
  * every launch of such a call is the device table's PNG operation, with RGB present -- the fused RGB where the pictures are of
    the coded size, the target of the geometry or orientation pass exactly where they are not -- and no output planes;
  * the blob holds n x the longest file (mvhp_png_max_bytes, rounded to 16);
  * the sink gets no planes, the right picture's file in `rgb` and its length in the geometry's reserved[0] (the stub's files
    have lengths that depend on the picture and end marks; AddressSanitizer watches the buffers);
  * `wanted` is respected, scores travel beside the files, d2h_bytes is exactly the table entries plus the files' bytes;
  * a device table without the operation fails every picture with a message; the plain sink, and PNG together with JPEG, are
    refused.
The existing modes run first in the same process and must still pass."""
import os
import subprocess

import pytest

from tests.test_engine_harness import _build
from tests.test_engine_harness_geometry import _streams


@pytest.mark.parametrize("sanitize", ["thread", "address,undefined"])
def test_engine_harness_png(tmp_path, sanitize):
    _streams(tmp_path)
    exe = _build(tmp_path, sanitize)
    env = dict(os.environ, TSAN_OPTIONS="halt_on_error=1", ASAN_OPTIONS="detect_leaks=1")
    for k in ("MINIVIDEO_CROP", "MINIVIDEO_THUMBNAIL", "MINIVIDEO_WRITERS", "MINIVIDEO_JPEG", "MINIVIDEO_PNG"):
        env.pop(k, None)
    r = subprocess.run([str(exe), str(tmp_path / "a.264"), str(tmp_path / "b.264"), "4", str(tmp_path / "c.264"), "png"],
                       capture_output=True, text=True, timeout=600, env=env)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "PNG MODE DONE" in r.stdout and "HARNESS OK" in r.stdout, r.stdout + r.stderr
    assert r.stdout.count("\npng ") >= 15
    assert "ThreadSanitizer" not in r.stderr and "AddressSanitizer" not in r.stderr and "runtime error" not in r.stderr, r.stderr
