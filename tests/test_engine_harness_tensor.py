"""CPU: the decode engine with MVHP_OUT_TENSOR on the stub device of tools/engine_harness.cpp, under ThreadSanitizer and
AddressSanitizer: a stand-alone program, nothing preloaded.  The harness's tensor mode (a fifth argument "tensor" behind the
geometry mode's stream; the stub's tensor operation stamps every tensor with the checksum its picture's RGB carries) checks, with
one to three contexts, small and large batches, at the coded size, cropped and boxed onto a fixed canvas, alone and beside
MVHP_OUTPUT_SCORE:
  * host delivery: the sink gets no planes, the stub's tensor of its own picture, of exactly the length g->reserved[0] names, and
    the geometry of the request; d2h_bytes is the tensors' bytes (and 32 per score), one operation runs behind every launch, a
    re-queued batch is packed again, and a picture larger than the canvas fails in its place with a message;
  * device delivery into a stand-in target in host memory, on one context: nothing is downloaded, the sink gets neither planes
    nor RGB and finds the tensor in slot `seq` of the target when it runs, pictures whose geometry cannot be formed, that fail to
    parse or that lie past the target's last slot fail and leave their slots untouched;
  * refused with a message before any launch: a tensor call without a request (also after the request was taken back), tensors
    with JPEG, PNG or the black-bar probe, through the sink without a geometry, device delivery on two contexts, and every
    malformed request;
  * a device table without the operation fails the call before any launch, and calls without MVHP_OUT_TENSOR are not affected,
    with or without a request set.
The existing modes run first in the same process and must still pass."""
import os
import subprocess

import pytest

from tests.test_engine_harness import _build
from tests.test_engine_harness_geometry import _streams

_SWITCHES = ("MINIVIDEO_CROP", "MINIVIDEO_THUMBNAIL", "MINIVIDEO_WRITERS", "MINIVIDEO_JPEG", "MINIVIDEO_SKIP_BLANK",
             "MINIVIDEO_REPRESENTATIVE", "MINIVIDEO_BATCH", "MINIVIDEO_FAKE_GPUS", "MINIVIDEO_STATS")


@pytest.mark.parametrize("sanitize", ["thread", "address,undefined"])
def test_engine_harness_tensor(tmp_path, sanitize):
    _streams(tmp_path)
    exe = _build(tmp_path, sanitize)
    env = dict(os.environ, TSAN_OPTIONS="halt_on_error=1", ASAN_OPTIONS="detect_leaks=1")
    for k in _SWITCHES:
        env.pop(k, None)
    r = subprocess.run([str(exe), str(tmp_path / "a.264"), str(tmp_path / "b.264"), "4", str(tmp_path / "c.264"), "tensor"],
                       capture_output=True, text=True, timeout=600, env=env)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "GEOMETRY MODE DONE" in r.stdout and "TENSOR MODE DONE" in r.stdout and "HARNESS OK" in r.stdout, r.stdout + r.stderr
    out = r.stdout
    assert out.count("tensor coded size, host") == out.count("tensor crop, host") == out.count("tensor box, host") == 12
    assert out.count("tensor box, device") == 2 and out.count("tensor, device, broken") == 1
    assert out.count("tensor: canvas too small") == 1 and out.count("malformed tensor request") == 9
    for name in ("tensor: no request", "tensor with JPEG", "tensor with PNG", "tensor with bars", "tensor, plain sink",
                 "tensor, device, 2 contexts", "tensor: table without it ", "tensor: table without it, off", "tensor: request set, flag off"):
        assert out.count(name) == 1, name
    assert "ThreadSanitizer" not in r.stderr and "AddressSanitizer" not in r.stderr and "runtime error" not in r.stderr, r.stderr
