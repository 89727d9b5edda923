"""GPU: MINIVIDEO_ASPECT=1 and MINIVIDEO_COLOR=auto|bt601|bt709|bt601-full|bt709-full through minivideo_decode -- the product CLI
with its -a and -m options -- on Annex B and MP4: png, bmp and tga files of the aspect's size whose pixels are the colour pass
over the final planes; yuv420 and jpg files are those without -m; malformed values fail with a message and write nothing.
Expected pictures: the chain of tests/test_gpu_engine_color.py (oracle planes, tests/resample_ref.py, tests/color_ref.py)."""
import os
import subprocess

import numpy as np
import pytest

from minivideo_amd import gen
from minivideo_amd.hotpath import StreamParams
from oracle import loader
from tests import refdec
from tests import resample_ref as R
from tests.mp4mux import mux
from tests.test_gpu_engine_color import CROP, SAR, H, W, chain, expected_rgb

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CLI = os.path.join(ROOT, "minivideo_amd", "mini_thumbnailer")
F = 3
SWITCHES = ("MINIVIDEO_CROP", "MINIVIDEO_THUMBNAIL", "MINIVIDEO_DEBLOCK", "MINIVIDEO_SPEC", "MINIVIDEO_JPEG", "MINIVIDEO_ROTATE",
            "MINIVIDEO_PNG", "MINIVIDEO_SKIP_BLANK", "MINIVIDEO_ASPECT", "MINIVIDEO_COLOR")
DISPLAY = dict(signal_present=1, full_range=0, matrix_coefficients=1, chroma_loc=1)      # BT.709 limited, centred chroma


@pytest.fixture(scope="module")
def clip():
    """(Annex-B bytes, the same as an MP4, oracle planes per picture); one SPS: the MP4 carries it in avcC"""
    rec = gen.vui_record(sar=SAR, full_range=0, matrix=1, chroma_loc=1, timing=True)
    stream, packed = gen.make_stream_vui(W, H, F, [rec], crops=[CROP], seed=43, profile="high")
    planes = loader.recon(StreamParams(W, H, 0, 0, 1), packed, F)[0].reshape(F, -1)
    return stream, np.frombuffer(mux(stream, 16 * W, 16 * H), np.uint8), planes


def _run(d, data, name, fmt, args=(), env_extra=None, check=True):
    d.mkdir()
    path = d / name
    data.tofile(path)
    env = dict(os.environ)
    for k in SWITCHES:
        env.pop(k, None)
    env.update(env_extra or {})
    r = subprocess.run([CLI, "-i", str(path), "-f", fmt, "-n", str(F), *args], cwd=d, capture_output=True, text=True, timeout=120, env=env)
    if check:
        assert r.returncode == 0 and "decode did not succeed" not in r.stderr, r.stderr
    return r, {f: (d / f).read_bytes() for f in sorted(os.listdir(d)) if f != name}


def _check_rgb(files, fmt, planes, shape, color):
    assert sorted(files) == ["c_%d.%s" % (k, fmt) for k in range(F)]
    for k in range(F):
        geom, wy, scaled = chain(planes[k], shape)
        px, w, h = refdec.read_rgb(fmt, files["c_%d.%s" % (k, fmt)])
        assert (w, h) == geom[4:], (k, w, h)
        assert np.array_equal(px, expected_rgb(wy, geom, scaled, color, DISPLAY)), (fmt, k)


@pytest.mark.parametrize("container", ["annexb", "mp4"])
@pytest.mark.parametrize("fmt", ["png", "bmp", "tga"])
def test_aspect_and_colour_files(tmp_path, clip, fmt, container):
    stream, mp4, planes = clip
    data, name = (stream, "c.264") if container == "annexb" else (mp4, "c.mp4")
    _, files = _run(tmp_path / "a", data, name, fmt, ["-a", "-m", "auto"])
    _check_rgb(files, fmt, planes, dict(aspect=True), "auto")
    _, files = _run(tmp_path / "b", data, name, fmt, ["-m", "bt709-full"])
    _check_rgb(files, fmt, planes, dict(), "bt709-full")
    _, files = _run(tmp_path / "c", data, name, fmt, ["-m", "auto", "-s", "40x24"])
    _check_rgb(files, fmt, planes, dict(output=(40, 24)), "auto")


def test_aspect_alone_and_by_variable(tmp_path, clip):
    """-a alone: the size of the rule, today's colour formula; the variable does what the option does"""
    stream, _, planes = clip
    _, alone = _run(tmp_path / "d", stream, "c.264", "bmp", ["-a"])
    _, by_env = _run(tmp_path / "e", stream, "c.264", "bmp", env_extra={"MINIVIDEO_ASPECT": "1"})
    assert alone == by_env
    px, w, h = refdec.read_rgb("bmp", alone["c_0.bmp"])
    geom, wy, _ = chain(planes[0], dict(aspect=True))
    assert (w, h) == geom[4:] == (74, 32) and np.array_equal(px, R.to_rgb(wy, w, h).reshape(-1))


@pytest.mark.parametrize("value", ["0", ""])
def test_zero_and_empty_are_the_files_without_the_switches(tmp_path, clip, value):
    stream = clip[0]
    _, plain = _run(tmp_path / "f", stream, "c.264", "bmp")
    _, off = _run(tmp_path / "g", stream, "c.264", "bmp", env_extra={"MINIVIDEO_ASPECT": value, "MINIVIDEO_COLOR": value})
    assert off == plain and len(plain) == F


def test_compressed_png_of_the_colour_pass(tmp_path, clip):
    stream, _, planes = clip
    _, files = _run(tmp_path / "z", stream, "c.264", "png", ["-z", "-a", "-m", "auto"])
    _check_rgb(files, "png", planes, dict(aspect=True), "auto")


@pytest.mark.parametrize("fmt,extra", [("yuv420", []), ("jpg", ["-j"])])
def test_colour_leaves_planes_and_jpeg_alone(tmp_path, clip, fmt, extra):
    stream, _, _ = clip
    _, with_m = _run(tmp_path / "m", stream, "c.264", fmt, ["-m", "bt709-full", "-c"] + extra)
    _, without = _run(tmp_path / "p", stream, "c.264", fmt, ["-c"] + extra)
    assert with_m == without and len(without) == F


@pytest.mark.parametrize("var,opt,bad", [("MINIVIDEO_COLOR", "-m", "709"), ("MINIVIDEO_COLOR", "-m", "bt709x"), ("MINIVIDEO_COLOR", "-m", "AUTO"),
                                         ("MINIVIDEO_ASPECT", None, "yes"), ("MINIVIDEO_ASPECT", None, "4:3")])
def test_malformed_values_fail_and_write_nothing(tmp_path, clip, var, opt, bad):
    stream = clip[0]
    args, env = ((opt, bad), {}) if opt else ((), {var: bad})
    r, files = _run(tmp_path / "x", stream, "c.264", "bmp", args, env, check=False)
    assert var in r.stderr and "decode did not succeed" in r.stderr, r.stderr
    assert files == {}
