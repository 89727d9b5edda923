"""GPU: MINIVIDEO_CROP=1 / MINIVIDEO_THUMBNAIL=<w>x<h> through minivideo_decode -- the product CLI (also with its -c / -s
options) and the stock upstream main.cpp built against this library: unchanged file names, yuv420 / yuv444 / bmp / tga bytes and
png pixels of the expected pictures at the output size, MP4 like Annex B.  Expected pictures: oracle reconstruction of the
generator's records, then tests/resample_ref.py with the geometry worked out here from the crop offsets."""
import os
import subprocess

import numpy as np
import pytest

from minivideo_amd import gen
from minivideo_amd.hotpath import StreamParams
from oracle import loader
from tests import resample_ref as R
from tests.test_gpu_api import _bmp, _png_pixels, _tga

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CLI = os.path.join(ROOT, "minivideo_amd", "mini_thumbnailer")
STOCK = os.path.join(ROOT, "oracle", "_ref", "mini_thumbnailer_stock")
W, H, F = 9, 7, 3
CROP = (1, 3, 2, 1)
SWITCHES = {"crop": {"MINIVIDEO_CROP": "1"}, "box": {"MINIVIDEO_THUMBNAIL": "40x40"},
            "both": {"MINIVIDEO_CROP": "1", "MINIVIDEO_THUMBNAIL": "40x40"}}


def _geom(switch):
    l, r, t, b = CROP
    cx, cy, cw, ch = 2 * l, 2 * t, 16 * W - 2 * (l + r), 16 * H - 2 * (t + b)
    ow, oh = (cw, ch) if switch == "crop" else R.fit(cw, ch, 40, 40)
    return cx, cy, cw, ch, ow, oh


def _expected(packed_k, g):
    yuv, _ = loader.recon(StreamParams(W, H, 0, 0, 0), packed_k, 1)
    planes = R.resample(yuv, W, H, g)
    return planes.reshape(-1), R.to_rgb(planes, g[4], g[5]).reshape(-1)


def _yuv444(planes, w, h):
    """export.cpp write_yuv444: chroma doubled, the (odd, odd) sample left 0"""
    n = w * h
    out = [planes[:n]]
    for c in range(2):
        src = planes[n + c * (n // 4):n + (c + 1) * (n // 4)].reshape(h // 2, w // 2)
        up = np.zeros((h, w), np.uint8)
        up[0::2, 0::2] = src
        up[0::2, 1::2] = src
        up[1::2, 0::2] = src
        out.append(up.reshape(-1))
    return np.concatenate(out)


def _run(exe, d, data, name, fmt, env_extra, args=()):
    d.mkdir()
    path = d / name
    data.tofile(path)
    env = dict(os.environ)
    for k in ("MINIVIDEO_CROP", "MINIVIDEO_THUMBNAIL"):
        env.pop(k, None)
    env.update(env_extra)
    r = subprocess.run([str(exe), "-i", str(path), "-f", fmt, "-n", str(F), *args], cwd=d, capture_output=True, text=True,
                       timeout=120, env=env)
    assert r.returncode == 0 and "decode did not succeed" not in r.stderr, r.stderr
    return sorted(f for f in os.listdir(d) if f != name)


def _stream():
    return gen.make_stream_crop(W, H, F, [CROP], seed=23, profile="high")


@pytest.mark.parametrize("switch", ["crop", "box", "both"])
@pytest.mark.parametrize("fmt", ["yuv420", "yuv444", "bmp", "tga", "png"])
@pytest.mark.parametrize("which", ["product", "stock"])
def test_cli_output_geometry(tmp_path, which, fmt, switch):
    from tests.mp4mux import mux
    exe = CLI if which == "product" else STOCK
    if which == "stock" and not os.path.exists(STOCK):
        pytest.skip("oracle/_ref/mini_thumbnailer_stock was not built")
    stream, packed = _stream()
    g = _geom(switch)
    ow, oh = g[4], g[5]
    ext = {"yuv420": "yuv", "yuv444": "yuv"}.get(fmt, fmt)
    names = [f"c_{k}.{ext}" for k in range(F)]
    plain = _run(exe, tmp_path / "plain", stream, "c.264", fmt, {})
    es = _run(exe, tmp_path / "es", stream, "c.264", fmt, SWITCHES[switch])
    mp4 = _run(exe, tmp_path / "mp4", np.frombuffer(mux(stream, W * 16, H * 16), np.uint8), "c.mp4", fmt, SWITCHES[switch])
    assert plain == es == mp4 == names   # file names do not change
    for k in range(F):
        wy, wr = _expected(packed[k], g)
        data = (tmp_path / "es" / names[k]).read_bytes()
        if fmt == "yuv420":
            assert data == wy.tobytes(), k
        elif fmt == "yuv444":
            assert data == _yuv444(wy, ow, oh).tobytes(), k
        elif fmt == "bmp":
            assert data == _bmp(wr, ow, oh), k
        elif fmt == "tga":
            assert data == _tga(wr, ow, oh), k
        else:
            pix, w, h = _png_pixels(data)
            assert (w, h) == (ow, oh) and np.array_equal(pix, wr), k
        assert (tmp_path / "mp4" / names[k]).read_bytes() == data, k
        # with neither switch: the coded size, as before
        if fmt == "yuv420":
            assert (tmp_path / "plain" / names[k]).read_bytes() == loader.recon(StreamParams(W, H, 0, 0, 0), packed[k], 1)[0].tobytes()


@pytest.mark.parametrize("fmt", ["yuv420", "bmp"])
def test_product_cli_options_equal_the_environment(tmp_path, fmt):
    stream, _ = _stream()
    for switch, args in (("crop", ["-c"]), ("box", ["-s", "40x40"]), ("both", ["-c", "-s", "40x40"])):
        a = _run(CLI, tmp_path / (switch + "_env"), stream, "c.264", fmt, SWITCHES[switch])
        b = _run(CLI, tmp_path / (switch + "_opt"), stream, "c.264", fmt, {}, args)
        assert a == b and len(a) == F
        for name in a:
            assert (tmp_path / (switch + "_env") / name).read_bytes() == (tmp_path / (switch + "_opt") / name).read_bytes(), name


@pytest.mark.parametrize("bad", ["abc", "0x10", "320", "1x40"])
def test_cli_malformed_thumbnail_fails(tmp_path, bad):
    stream, _ = _stream()
    path = tmp_path / "c.264"
    stream.tofile(path)
    r = subprocess.run([CLI, "-i", str(path), "-f", "yuv420", "-s", bad], cwd=tmp_path, capture_output=True, text=True, timeout=120)
    assert "MINIVIDEO_THUMBNAIL" in r.stderr and "decode did not succeed" in r.stderr, r.stderr
    assert [f for f in os.listdir(tmp_path) if f != "c.264"] == []
