"""GPU: MINIVIDEO_PNG=1 through minivideo_decode -- the product CLI (also with its -z option) and the stock upstream main.cpp
built against this library: whenever the format resolves to PNG the files are the model's (tests/png_ref.py) of the expected
picture's RGB, under today's names, Annex B like MP4, together with MINIVIDEO_CROP / _THUMBNAIL / _ROTATE / _DEBLOCK / _SPEC /
_SKIP_BLANK; every file decodes in PIL to the pixels of the `-f bmp` file of the same job; MINIVIDEO_JPEG=1 with `-f jpg` still
gives JPEG; and without the variable nothing changes."""
import io
import os
import subprocess

import numpy as np
import pytest
from PIL import Image

from minivideo_amd import gen
from minivideo_amd.hotpath import StreamParams
from oracle import loader
from tests import orient_ref as O, png_ref as P, resample_ref as R

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CLI = os.path.join(ROOT, "minivideo_amd", "mini_thumbnailer")
STOCK = os.path.join(ROOT, "oracle", "_ref", "mini_thumbnailer_stock")
W, H, F = 9, 7, 3
CROP = (1, 3, 2, 1)
SWITCHES = ("MINIVIDEO_CROP", "MINIVIDEO_THUMBNAIL", "MINIVIDEO_DEBLOCK", "MINIVIDEO_SPEC", "MINIVIDEO_JPEG", "MINIVIDEO_PNG",
            "MINIVIDEO_ROTATE", "MINIVIDEO_SKIP_BLANK")


def _run(exe, d, data, name, env_extra, args=(), fmt="png"):
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


def _files(planes, g, turns=0):
    out = {}
    for k in range(len(planes)):
        t = O.turn(R.resample(planes[k], W, H, g), g[4], g[5], turns)
        tw, th = O.turned_size(g[4], g[5], turns)
        out["c_%d.png" % k] = P.encode(R.to_rgb(t, tw, th).reshape(-1), tw, th)
    return out


def _pixels_of_bmp(b):
    return np.asarray(Image.open(io.BytesIO(b)).convert("RGB"))


@pytest.mark.parametrize("switch", ["none", "crop", "box"])
@pytest.mark.parametrize("which", ["product", "stock"])
def test_cli_writes_the_models_files(tmp_path, cropped, which, switch):
    from tests.mp4mux import mux
    exe = CLI if which == "product" else STOCK
    if which == "stock" and not os.path.exists(STOCK):
        pytest.skip("oracle/_ref/mini_thumbnailer_stock was not built")
    stream, planes = cropped
    env = {"MINIVIDEO_PNG": "1"}
    env.update({"crop": {"MINIVIDEO_CROP": "1"}, "box": {"MINIVIDEO_THUMBNAIL": "40x40"}}.get(switch, {}))
    es = _run(exe, tmp_path / "es", stream, "c.264", env)
    mp4 = _run(exe, tmp_path / "mp4", np.frombuffer(mux(stream, W * 16, H * 16), np.uint8), "c.mp4", env)
    assert es == mp4 == _files(planes, _geom(switch))
    jpg = _run(exe, tmp_path / "jpg", stream, "c.264", env, fmt="jpg")          # -f jpg without MINIVIDEO_JPEG resolves to PNG
    assert jpg == es
    bmp = _run(exe, tmp_path / "bmp", stream, "c.264", env, fmt="bmp")          # the same job as bitmaps: untouched by the switch
    assert bmp == _run(exe, tmp_path / "bmp0", stream, "c.264", {k: v for k, v in env.items() if k != "MINIVIDEO_PNG"}, fmt="bmp")
    for k in range(F):
        im = Image.open(io.BytesIO(es["c_%d.png" % k]))
        im.load()
        assert np.array_equal(np.asarray(im), _pixels_of_bmp(bmp["c_%d.bmp" % k])), k


def test_product_cli_option_names_and_jpeg(tmp_path, cropped):
    stream, planes = cropped
    a = _run(CLI, tmp_path / "env", stream, "c.264", {"MINIVIDEO_PNG": "1"})
    b = _run(CLI, tmp_path / "opt", stream, "c.264", {}, ["-z"])
    assert a == b == _files(planes, _geom("none"))
    one = _run(CLI, tmp_path / "one", stream, "c.264", {}, ["-z", "-n", "1"])     # a single picture has no _k
    assert one == {"c.png": a["c_0.png"]}
    both = _run(CLI, tmp_path / "both", stream, "c.264", {"MINIVIDEO_PNG": "1", "MINIVIDEO_JPEG": "1"}, fmt="jpg")
    assert both == _run(CLI, tmp_path / "jpeg", stream, "c.264", {"MINIVIDEO_JPEG": "1"}, fmt="jpg")   # still JPEG
    assert sorted(both) == ["c_%d.jpg" % k for k in range(F)]
    turned = _run(CLI, tmp_path / "rot", stream, "c.264", {"MINIVIDEO_PNG": "1", "MINIVIDEO_ROTATE": "90", "MINIVIDEO_CROP": "1"})
    assert turned == _files(planes, _geom("crop"), 1)


@pytest.mark.parametrize("which", ["product", "stock"])
def test_without_the_variable_nothing_changes(tmp_path, cropped, which):
    """the host writer's stored files, the same bytes with the variable unset, 0 or empty -- and larger than the compressed ones"""
    exe = CLI if which == "product" else STOCK
    if which == "stock" and not os.path.exists(STOCK):
        pytest.skip("oracle/_ref/mini_thumbnailer_stock was not built")
    stream, _ = cropped
    png = _run(exe, tmp_path / "png", stream, "c.264", {})
    off = _run(exe, tmp_path / "off", stream, "c.264", {"MINIVIDEO_PNG": "0"})
    on = _run(exe, tmp_path / "on", stream, "c.264", {"MINIVIDEO_PNG": "1"})
    assert sorted(png) == sorted(on) == ["c_%d.png" % k for k in range(F)] and png == off
    data = 16 * H * (3 * 16 * W + 1)
    for k in range(F):                                   # (export.cpp write_png: filter 0, one IDAT of stored blocks)
        assert len(png["c_%d.png" % k]) == 8 + 25 + 12 + 2 + 5 * -(-data // 65535) + data + 4 + 12
        assert len(on["c_%d.png" % k]) < len(png["c_%d.png" % k])
        a, b = Image.open(io.BytesIO(png["c_%d.png" % k])), Image.open(io.BytesIO(on["c_%d.png" % k]))
        assert np.array_equal(np.asarray(a), np.asarray(b))


def test_cli_with_spec_mode_deblocking_and_blank_skipping(tmp_path):
    """the planes change under these switches and the encoder takes the RGB as it is: the .png files hold the pixels of the .bmp
    files the same CLI writes under the same switches, and are the model's files of them"""
    spec_stream, _, _ = gen.make_stream_ex(W, H, F, seed=41, profile="high", slices=3, pcm_permille=50)   # (what only spec mode decodes)
    stream, _, _ = gen.make_stream_ex(W, H, F, seed=23, profile="high", deblock=dict(idc=(0, 1, 2), offsets=(-6, 6)))
    for name, data, env in (("spec", spec_stream, {"MINIVIDEO_SPEC": "1"}), ("blank", stream, {"MINIVIDEO_SKIP_BLANK": "1"}),
                            ("deblock", stream, {"MINIVIDEO_DEBLOCK": "1", "MINIVIDEO_THUMBNAIL": "40x40"})):
        bmp = _run(CLI, tmp_path / (name + "_bmp"), data, "c.264", env, fmt="bmp")
        got = _run(CLI, tmp_path / (name + "_png"), data, "c.264", dict(env, MINIVIDEO_PNG="1"))
        assert sorted(got) == ["c_%d.png" % k for k in range(F)]
        for k in range(F):
            px = _pixels_of_bmp(bmp["c_%d.bmp" % k])
            assert got["c_%d.png" % k] == P.encode(px, px.shape[1], px.shape[0]), (name, k)
