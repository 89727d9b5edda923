"""GPU: MINIVIDEO_JPEG=1 through minivideo_decode -- the product CLI (also with its -j option) and the stock upstream main.cpp
built against this library: `-f jpg` writes <name>_k.jpg whose bytes are the model's (tests/jpeg_ref.py) of the expected picture
at the asked quality, Annex B like MP4, together with MINIVIDEO_CROP / MINIVIDEO_THUMBNAIL / MINIVIDEO_DEBLOCK; without the
variable `-f jpg` still writes the PNG fallback, byte for byte what `-f png` writes."""
import os
import subprocess

import numpy as np
import pytest

from minivideo_amd import gen
from minivideo_amd.hotpath import PARAM_DEBLOCK, STREAM_DEBLOCK, StreamParams
from oracle import loader
from tests import deblock_ref, jpeg_ref as J, resample_ref as R
from tests.test_deblock import DStream

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CLI = os.path.join(ROOT, "minivideo_amd", "mini_thumbnailer")
STOCK = os.path.join(ROOT, "oracle", "_ref", "mini_thumbnailer_stock")
W, H, F = 9, 7, 3
CROP = (1, 3, 2, 1)
SWITCHES = ("MINIVIDEO_CROP", "MINIVIDEO_THUMBNAIL", "MINIVIDEO_DEBLOCK", "MINIVIDEO_SPEC", "MINIVIDEO_JPEG")


def _run(exe, d, data, name, env_extra, args=(), fmt="jpg"):
    d.mkdir()
    path = d / name
    data.tofile(path)
    env = dict(os.environ)
    for k in SWITCHES:
        env.pop(k, None)
    env.update(env_extra)
    r = subprocess.run([str(exe), "-i", str(path), "-f", fmt, "-n", str(F), *args], cwd=d, capture_output=True, text=True,
                       timeout=120, env=env)
    assert r.returncode == 0 and "decode did not succeed" not in r.stderr, r.stderr
    return {f: (d / f).read_bytes() for f in sorted(os.listdir(d)) if f != name}


@pytest.fixture(scope="module")
def cropped():
    stream, packed = gen.make_stream_crop(W, H, F, [CROP], seed=23, profile="high")
    yuv = loader.recon(StreamParams(W, H, 0, 0, 0), packed, F)[0].reshape(F, -1)
    return stream, yuv


def _geom(switch):
    l, r, t, b = CROP
    cx, cy, cw, ch = 2 * l, 2 * t, 16 * W - 2 * (l + r), 16 * H - 2 * (t + b)
    if switch == "none":
        return 0, 0, 16 * W, 16 * H, 16 * W, 16 * H
    ow, oh = (cw, ch) if switch == "crop" else R.fit(cw, ch, 40, 40)
    return cx, cy, cw, ch, ow, oh


def _files(planes, g, quality):
    return {"c_%d.jpg" % k: J.encode(R.resample(planes[k], W, H, g).reshape(-1), g[4], g[5], quality) for k in range(len(planes))}


@pytest.mark.parametrize("switch", ["none", "crop", "box"])
@pytest.mark.parametrize("which", ["product", "stock"])
def test_cli_writes_the_models_files(tmp_path, cropped, which, switch):
    from tests.mp4mux import mux
    exe = CLI if which == "product" else STOCK
    if which == "stock" and not os.path.exists(STOCK):
        pytest.skip("oracle/_ref/mini_thumbnailer_stock was not built")
    stream, planes = cropped
    env = {"MINIVIDEO_JPEG": "1"}
    env.update({"crop": {"MINIVIDEO_CROP": "1"}, "box": {"MINIVIDEO_THUMBNAIL": "40x40"}}.get(switch, {}))
    es = _run(exe, tmp_path / "es", stream, "c.264", env)
    mp4 = _run(exe, tmp_path / "mp4", np.frombuffer(mux(stream, W * 16, H * 16), np.uint8), "c.mp4", env)
    assert es == mp4 == _files(planes, _geom(switch), 75)     # (both front ends default to quality 75)


def test_product_cli_quality_and_option(tmp_path, cropped):
    stream, planes = cropped
    a = _run(CLI, tmp_path / "env", stream, "c.264", {"MINIVIDEO_JPEG": "1"}, ["-q", "90"])
    b = _run(CLI, tmp_path / "opt", stream, "c.264", {}, ["-q", "90", "-j"])
    assert a == b == _files(planes, _geom("none"), 90)
    one = _run(CLI, tmp_path / "one", stream, "c.264", {}, ["-j", "-n", "1"])     # a single picture has no _k
    assert one == {"c.jpg": _files(planes, _geom("none"), 75)["c_0.jpg"]}


@pytest.mark.parametrize("which", ["product", "stock"])
def test_without_the_variable_the_png_fallback_stays(tmp_path, cropped, which):
    exe = CLI if which == "product" else STOCK
    if which == "stock" and not os.path.exists(STOCK):
        pytest.skip("oracle/_ref/mini_thumbnailer_stock was not built")
    stream, _ = cropped
    jpg = _run(exe, tmp_path / "jpg", stream, "c.264", {})
    png = _run(exe, tmp_path / "png", stream, "c.264", {}, fmt="png")
    off = _run(exe, tmp_path / "off", stream, "c.264", {"MINIVIDEO_JPEG": "0"})
    assert sorted(jpg) == ["c_%d.png" % k for k in range(F)] and jpg == png == off
    other = _run(exe, tmp_path / "bmp", stream, "c.264", {"MINIVIDEO_JPEG": "1"}, fmt="bmp")   # other formats: untouched
    assert other == _run(exe, tmp_path / "bmp0", stream, "c.264", {}, fmt="bmp")


def test_cli_with_spec_mode(tmp_path):
    """MINIVIDEO_SPEC=1 changes the planes (several slices, I_PCM: what only spec mode decodes), and the encoder takes them as
    they are: the .jpg files are the model's of the planes the same CLI writes as yuv420 under the same switch"""
    stream, _, _ = gen.make_stream_ex(W, H, F, seed=41, profile="high", slices=3, pcm_permille=50)
    spec = {"MINIVIDEO_SPEC": "1"}
    yuv = _run(CLI, tmp_path / "yuv", stream, "c.264", spec, fmt="yuv420")
    assert sorted(yuv) == ["c_%d.yuv" % k for k in range(F)]
    got = _run(CLI, tmp_path / "jpg", stream, "c.264", dict(spec, MINIVIDEO_JPEG="1"))
    want = {"c_%d.jpg" % k: J.encode(np.frombuffer(yuv["c_%d.yuv" % k], np.uint8), 16 * W, 16 * H, 75) for k in range(F)}
    assert got == want


def test_cli_with_deblocking(tmp_path):
    stream, packed, _ = gen.make_stream_ex(W, H, F, seed=23, profile="high", deblock=dict(idc=(0, 1, 2), offsets=(-6, 6)))
    with DStream(stream, STREAM_DEBLOCK) as s:
        p = s.params(0)
    off = StreamParams.from_buffer_copy(p)
    off.flags = p.flags & ~PARAM_DEBLOCK
    planes = np.asarray(deblock_ref.deblock(loader.recon(off, packed, F)[0], packed, p)).reshape(F, -1)
    got = _run(CLI, tmp_path / "d", stream, "c.264", {"MINIVIDEO_JPEG": "1", "MINIVIDEO_DEBLOCK": "1", "MINIVIDEO_THUMBNAIL": "40x40"})
    g = (0, 0, 16 * W, 16 * H) + tuple(R.fit(16 * W, 16 * H, 40, 40))
    assert got == _files(planes, g, 75)
