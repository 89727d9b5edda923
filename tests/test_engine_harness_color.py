"""CPU: the decode engine under MVHP_OUTPUT_ASPECT / MVHP_OUTPUT_COLOR on the stub device of tools/engine_harness.cpp, under
ThreadSanitizer and AddressSanitizer (a stand-alone program, nothing preloaded).  The harness's color mode (a fifth argument
"color" and a sixth, a stream whose SPSs alternate between two VUIs that differ in matrix and range only) checks, for RGB, RGB
only and PNG, at the coded size, cropped, boxed, with the aspect, the aspect and a box, and the aspect turned by 90 degrees, under
"auto" and a forced mode:
  * the job descriptors: a colour pass exactly in the batches of a call that delivers RGB and asks for it, never beside JPEG, with
    planes to read and RGB to write -- the pass's targets behind a pass, the buffers of the coded size otherwise -- and no RGB from
    any other pass (the stub refuses a malformed descriptor);
  * every picture's RGB carries ITS OWN resolved setting (centred where the pass scaled), and batches split where the setting
    changes: under "auto" at every picture of this stream, under a forced mode nowhere;
  * the buffers hold n pictures of the delivered geometry, d2h_bytes is the sum of the delivered sizes and equals the call without
    the flag; the aspect geometry is the rule's;
  * the flag with planes only or JPEG runs no colour pass and gives the launches and bytes of the request without it;
  * a re-queued batch keeps its setting; a device table without the operation fails every picture with a message;
  * MINIVIDEO_ASPECT=1 and MINIVIDEO_COLOR=auto|bt709-full write files of the rule's size and RGB with the picture's setting, 0 and
    the empty string are today's files, and malformed values make minivideo_decode return FAILURE with a message before a device
    context exists.
The existing modes run first in the same process and must still pass."""
import os
import subprocess

import pytest

from minivideo_amd import gen
from tests.test_engine_harness import _build
from tests.test_engine_harness_geometry import _streams


@pytest.mark.parametrize("sanitize", ["thread", "address,undefined"])
def test_engine_harness_color(tmp_path, sanitize):
    _streams(tmp_path)
    vuis = [gen.vui_record(sar=14, full_range=1, matrix=1, overscan=1), gen.vui_record(sar=(8, 6), full_range=0, matrix=6, timing=True)]
    s4, _ = gen.make_stream_vui(6, 5, 8, vuis, crops=[(1, 2, 0, 3)], seed=12, profile="baseline", sps_pps_every_frame=True)
    s4.tofile(tmp_path / "d.264")
    exe = _build(tmp_path, sanitize)
    env = dict(os.environ, TSAN_OPTIONS="halt_on_error=1", ASAN_OPTIONS="detect_leaks=1")
    for k in ("MINIVIDEO_CROP", "MINIVIDEO_THUMBNAIL", "MINIVIDEO_WRITERS", "MINIVIDEO_JPEG", "MINIVIDEO_PNG", "MINIVIDEO_SKIP_BLANK",
              "MINIVIDEO_BLANK_VARIANCE", "MINIVIDEO_BLANK_ALTERNATES", "MINIVIDEO_ROTATE", "MINIVIDEO_ASPECT", "MINIVIDEO_COLOR"):
        env.pop(k, None)
    r = subprocess.run([str(exe), str(tmp_path / "a.264"), str(tmp_path / "b.264"), "4", str(tmp_path / "c.264"), "color",
                        str(tmp_path / "d.264")], capture_output=True, text=True, timeout=600, env=env)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "COLOR MODE DONE" in r.stdout and "HARNESS OK" in r.stdout, r.stdout + r.stderr
    assert r.stdout.count("malformed display switch") == 7 and r.stdout.count("public API, display") == 10
    assert "color: table without it" in r.stdout and "color requeue/3ctx" in r.stdout
    assert "ThreadSanitizer" not in r.stderr and "AddressSanitizer" not in r.stderr and "runtime error" not in r.stderr, r.stderr
