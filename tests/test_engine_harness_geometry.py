"""CPU: the decode engine with an output request (mvhp_engine_decode_ex) and minivideo_decode under MINIVIDEO_CROP /
MINIVIDEO_THUMBNAIL, on the stub device of tools/engine_harness.cpp, under ThreadSanitizer and AddressSanitizer.  The harness's
geometry mode (its fourth argument: a stream whose SPS crop changes) checks, against mvhp_output_geometry itself:
  * a stream that mixes two crops, uncropped pictures and one crop that leaves nothing splits into one batch per run of equal
    geometry; the picture without a geometry arrives as a failure with the library's message, and decoding goes on;
  * the sink sees the right geometry per picture, in order, and buffers that reach to the last byte of that geometry (the stub
    fills and marks every output picture; AddressSanitizer watches the device and host buffers); planes only, planes + RGB and
    RGB only; d2h_bytes is exactly the sum of the geometry sizes delivered;
  * a failed batch is re-queued with its geometry;
  * a request that equals the coded size never calls the device table's geometry operation (geometry_launches = 0);
  * minivideo_decode writes yuv420 / bmp / tga files with the sizes and headers of the output geometry and the stub's stamps
    in place, with and without writer threads; with neither switch the files are of the coded size;
  * each malformed MINIVIDEO_THUMBNAIL value makes minivideo_decode return FAILURE with a message before a device context exists.
The existing invocation (three arguments) runs first in the same process and must still end in HARNESS OK."""
import os
import subprocess

import pytest

from minivideo_amd import gen
from tests.test_engine_harness import SRC, _break_picture, _build

A, B, Z, NOTHING = (1, 3, 2, 1), (0, 0, 0, 4), (0, 0, 0, 0), (30, 30, 0, 0)   # (left, right, top, bottom) crop offsets
CROPS = [A, A, A, B, B, A, Z, Z, B, B, B, NOTHING, B, A, A, Z, A]


def _streams(tmp_path):
    stream, _ = gen.make_stream(6, 4, 23, seed=5, profile="baseline", dense=True, want_packed=False)
    stream.tofile(tmp_path / "a.264")
    s2, _ = gen.make_stream(5, 3, 11, seed=6, profile="main", dense=True, want_packed=False)
    _break_picture(s2, 4).tofile(tmp_path / "b.264")
    s3, _ = gen.make_stream_crop(6, 5, len(CROPS), CROPS, seed=9, profile="baseline", sps_pps_every_frame=True)
    s3.tofile(tmp_path / "c.264")


@pytest.mark.parametrize("sanitize", ["thread", "address,undefined"])
def test_engine_harness_geometry(tmp_path, sanitize):
    assert len(SRC) == 8
    _streams(tmp_path)
    exe = _build(tmp_path, sanitize)
    env = dict(os.environ, TSAN_OPTIONS="halt_on_error=1", ASAN_OPTIONS="detect_leaks=1")
    for k in ("MINIVIDEO_CROP", "MINIVIDEO_THUMBNAIL", "MINIVIDEO_WRITERS"):
        env.pop(k, None)
    r = subprocess.run([str(exe), str(tmp_path / "a.264"), str(tmp_path / "b.264"), "4", str(tmp_path / "c.264")],
                       capture_output=True, text=True, timeout=600, env=env)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "GEOMETRY MODE DONE" in r.stdout and "HARNESS OK" in r.stdout, r.stdout + r.stderr
    assert r.stdout.count("malformed thumbnail") >= 4
    assert "ThreadSanitizer" not in r.stderr and "AddressSanitizer" not in r.stderr and "runtime error" not in r.stderr, r.stderr
