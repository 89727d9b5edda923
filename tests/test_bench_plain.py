"""bench.py's plain run (no --full) and --dump-outputs: the plain line carries the headline figures and none of the side legs;
the dump is what the last timed step wrote, a fixed, seeded sample of the batch equal to the oracle's pictures at the same
places."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BENCH = os.path.join(ROOT, "bench.py")


def test_steps_must_be_positive_and_the_options_exist():
    r = subprocess.run([sys.executable, BENCH, "--steps", "0"], capture_output=True, text=True, timeout=120)
    assert r.returncode == 2 and "--steps must be at least 1" in r.stderr
    r = subprocess.run([sys.executable, BENCH, "--help"], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0 and "--full" in r.stdout and "--dump-outputs" in r.stdout


@pytest.mark.gpu
def test_plain_run_dumps_what_the_last_step_computed(tmp_path):
    import bench
    from minivideo_amd import gen
    from minivideo_amd.hotpath import StreamParams
    from oracle import loader

    frames, dump = 40, tmp_path / "dump"
    r = subprocess.run([sys.executable, BENCH, "--gpus", "1", "--steps", "3", "--warmup", "1", "--frames", str(frames),
                        "--dump-outputs", str(dump)], cwd=ROOT, capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stderr[-2000:]
    lines = [l for l in r.stdout.splitlines() if l.startswith("{")]
    assert len(lines) == 1, r.stdout[-2000:]
    d = json.loads(lines[0])
    assert d["unit"] == "macroblocks/s" and d["higher_is_better"] is True and d["dtype"] == "int32"
    assert d["steps"] == 3 and d["warmup"] == 1 and d["ms_per_step"] > 0 and d["value"] > 0
    assert abs(d["value"] - frames * 8160 / (d["ms_per_step"] * 1e-3)) / d["value"] < 1e-6
    # the side legs are --full's
    assert d["end_to_end"] is None and d["engine_multi_context"] is None and d["cli"] is None and d["placement"] is None
    assert "cpu_baseline" not in d and d["config"]["bit_exact_vs_oracle"] is None

    # the same inputs as the bench (16 distinct pictures of the rank-0 stream, tiled) through the oracle
    _, packed = gen.make_stream(120, 68, 16, seed=1000, profile="baseline", dense=True)
    params = StreamParams(120, 68, 0, 0, 0)
    rng = np.random.default_rng(bench.DUMP_SEED)
    pics = np.sort(rng.choice(frames, size=bench.DUMP_PICTURES, replace=False))
    ref = [loader.recon(params, packed[f % 16], 1, want_rgb=True) for f in pics]
    total = 0
    for name, k in (("ycbcr", 0), ("rgb", 1)):
        got = np.load(dump / (name + ".npy"))
        total += got.nbytes
        n = ref[0][k].size
        offs = np.sort(rng.choice(n, size=bench.DUMP_OFFSETS, replace=False))
        assert got.dtype == np.float32 and got.shape == (len(pics), len(offs)), (name, got.shape)
        for i in range(len(pics)):
            assert np.array_equal(got[i], ref[i][k][offs].astype(np.float32)), (name, int(pics[i]))
    assert total <= 64 << 20
