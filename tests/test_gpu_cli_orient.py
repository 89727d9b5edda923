"""GPU: MINIVIDEO_ROTATE=auto|0|90|180|270 through minivideo_decode -- the product CLI (with its -r option) and the stock
upstream main.cpp built against this library (which takes the variable itself): bmp, yuv420 and jpg files of the turned size and
bytes; without the switch the files of today.  Expected pictures: oracle reconstruction of the generator's records,
tests/resample_ref.py with the geometry before the turn, tests/orient_ref.py, and tests/jpeg_ref.py of the turned planes."""
import os
import subprocess

import numpy as np
import pytest

from minivideo_amd import gen
from minivideo_amd.hotpath import StreamParams
from oracle import loader
from tests import jpeg_ref as J
from tests import orient_ref as O
from tests import resample_ref as R
from tests.orient_streams import rotated_mp4
from tests.test_gpu_api import _bmp

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CLI = os.path.join(ROOT, "minivideo_amd", "mini_thumbnailer")
STOCK = os.path.join(ROOT, "oracle", "_ref", "mini_thumbnailer_stock")
W, H, F = 9, 7, 3
CROP = (1, 3, 2, 1)
SWITCHES = ("MINIVIDEO_CROP", "MINIVIDEO_THUMBNAIL", "MINIVIDEO_DEBLOCK", "MINIVIDEO_SPEC", "MINIVIDEO_JPEG", "MINIVIDEO_ROTATE")


@pytest.fixture(scope="module")
def clip():
    """(Annex-B bytes, the same as a 90-degree MP4, oracle planes per picture)"""
    stream, packed = gen.make_stream_crop(W, H, F, [CROP], seed=37, profile="high")
    planes = loader.recon(StreamParams(W, H, 0, 0, 1), packed, F)[0].reshape(F, -1)
    mp4 = np.frombuffer(rotated_mp4(stream, 16 * W, 16 * H, 1), np.uint8)
    return stream, mp4, planes


def _run(exe, d, data, name, fmt, env_extra, args=()):
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


def _turned(planes_k, box, turns):
    """-> (turned planes, RGB, width, height): the geometry before the turn from the crop offsets and the box turned back"""
    l, r, t, b = CROP
    if box is None:
        g = (0, 0, 16 * W, 16 * H, 16 * W, 16 * H)
    else:
        cw, ch = 16 * W - 2 * (l + r), 16 * H - 2 * (t + b)
        bw, bh = (box[1], box[0]) if turns & 1 else box
        g = (2 * l, 2 * t, cw, ch) + R.fit(cw, ch, bw, bh)
    tp = O.turn(R.resample(planes_k, W, H, g), g[4], g[5], turns)
    tw, th = O.turned_size(g[4], g[5], turns)
    return tp.reshape(-1), O.to_rgb(tp, g[4], g[5], turns).reshape(-1), tw, th


def _files(planes, fmt, box, turns):
    out = {}
    for k in range(F):
        ty, tr, tw, th = _turned(planes[k], box, turns)
        if fmt == "yuv420":
            out["c_%d.yuv" % k] = ty.tobytes()
        elif fmt == "bmp":
            out["c_%d.bmp" % k] = _bmp(tr, tw, th)
        else:
            out["c_%d.jpg" % k] = J.encode(ty, tw, th, 75)
    return out


@pytest.mark.parametrize("fmt", ["bmp", "yuv420", "jpg"])
@pytest.mark.parametrize("which", ["product", "stock"])
def test_auto_on_a_90_degree_mp4(tmp_path, clip, which, fmt):
    if which == "stock" and not os.path.exists(STOCK):
        pytest.skip("oracle/_ref/mini_thumbnailer_stock was not built")
    stream, mp4, planes = clip
    jpeg = {"MINIVIDEO_JPEG": "1"} if fmt == "jpg" else {}
    if which == "product":
        got = _run(CLI, tmp_path / "r", mp4, "c.mp4", fmt, jpeg, ["-r", "auto"])
    else:
        got = _run(STOCK, tmp_path / "r", mp4, "c.mp4", fmt, dict(jpeg, MINIVIDEO_ROTATE="auto"))
    assert got == _files(planes, fmt, None, 1)
    # without the switch: the files of today, lying on their side
    plain = _run(CLI if which == "product" else STOCK, tmp_path / "plain", mp4, "c.mp4", fmt, jpeg)
    assert plain == _files(planes, fmt, None, 0)
    # and "auto" on the elementary stream, which has no rotation, changes nothing
    es = _run(CLI if which == "product" else STOCK, tmp_path / "es", stream, "c.264", fmt, dict(jpeg, MINIVIDEO_ROTATE="auto"))
    assert es == plain


@pytest.mark.parametrize("fmt", ["bmp", "yuv420", "jpg"])
def test_explicit_angle_and_box(tmp_path, clip, fmt):
    stream, mp4, planes = clip
    jpeg = ["-j"] if fmt == "jpg" else []
    got = _run(CLI, tmp_path / "a", stream, "c.264", fmt, {}, ["-r", "270", "-s", "64x64"] + jpeg)
    assert got == _files(planes, fmt, (64, 64), 3)
    # an explicit angle is taken whatever the file says
    same = _run(CLI, tmp_path / "b", mp4, "c.mp4", fmt, {}, ["-r", "270", "-s", "64x64"] + jpeg)
    assert same == got
    half = _run(CLI, tmp_path / "c", stream, "c.264", fmt, {"MINIVIDEO_ROTATE": "180"}, jpeg)
    assert half == _files(planes, fmt, None, 2)


@pytest.mark.parametrize("bad", ["45", "90x", "left"])
def test_cli_malformed_rotation_fails(tmp_path, clip, bad):
    path = tmp_path / "c.264"
    clip[0].tofile(path)
    r = subprocess.run([CLI, "-i", str(path), "-f", "yuv420", "-r", bad], cwd=tmp_path, capture_output=True, text=True, timeout=120)
    assert "MINIVIDEO_ROTATE" in r.stderr and "decode did not succeed" in r.stderr, r.stderr
    assert [f for f in os.listdir(tmp_path) if f != "c.264"] == []
