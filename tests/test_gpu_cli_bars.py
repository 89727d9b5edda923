"""GPU: MINIVIDEO_TRIM=1 through minivideo_decode -- the product CLI with its -t option and with the environment: Annex B and the
same stream in MP4, yuv420 bytes and png pixels, alone, with -s, with -r 90 and with -b.  The expected files are what the Python
model makes from the oracle's planes: the boxes of tests/bars_ref.py on the model's probe pictures, their union, the trim rule,
then tests/resample_ref.py / tests/orient_ref.py on the trimmed rectangle.  The generator has no black macroblocks, so the bars
come from the level (a switch of its own): the streams are put together from one-picture generator streams whose boxes at LEVEL lie
well inside the picture, and each scenario first asserts what the model says about it."""
import os
import subprocess

import numpy as np
import pytest

from minivideo_amd import gen
from minivideo_amd.hotpath import StreamParams
from oracle import loader
from tests import bars_ref as B
from tests import luma_ref as L
from tests import orient_ref as O
from tests import resample_ref as R
from tests.test_gpu_api import _png_pixels

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CLI = os.path.join(ROOT, "minivideo_amd", "mini_thumbnailer")
W, H, F, N = 9, 7, 5, 3
CROP = (1, 3, 2, 1)
RECT = (2, 4, 16 * W - 8, 16 * H - 6)
LEVEL = 245
_CACHE = {}


def _pictures(kind):
    """F one-picture streams put together -> (stream, oracle planes[F]).  "bars": pictures whose box at LEVEL the trim rule accepts
    and that leaves a bar on the left; "dark": sparse pictures without a sample above 254"""
    if kind not in _CACHE:
        parts, planes, seed = [], [], 100
        p = StreamParams(W, H, 0, 0, 0)
        while len(parts) < F:
            seed += 1
            assert seed < 400, "the generator no longer makes such pictures"
            s, pk = gen.make_stream_crop(W, H, 1, [CROP], seed=seed, profile="high", dense=kind == "bars", qp_range=(20, 44))
            yuv = loader.recon(p, pk[0], 1)[0].reshape(-1)
            Y = B.luma_plane(yuv, W, H)
            if kind == "bars":
                ok, rect = B.trim_rect(RECT, B.record(Y, RECT, LEVEL)[:4])
                good = ok == 1 and rect[0] >= 12 and B.record(Y, RECT)[:4] == RECT    # (a bar on the left in every one: so has the union)
            else:
                good = B.record(Y, RECT, 254)[:4] == (0, 0, 0, 0)
            if good:
                parts.append(s)
                planes.append(yuv)
        _CACHE[kind] = (np.concatenate(parts), np.stack(planes))
    return _CACHE[kind]


def _model_rect(planes, level, probes=B.PROBES):
    """what minivideo_decode trims to: the union over the model's probes of the unfiltered list (every IDR, in order)"""
    boxes = [B.record(B.luma_plane(planes[k], W, H), RECT, level)[:4] for k in B.probes(list(range(len(planes))), probes)]
    return B.trim_rect(RECT, B.union(boxes)[1])


def _expected(planes_k, rect, box, turns):
    size = rect[2:] if box is None else R.fit(rect[2], rect[3], *((box[1], box[0]) if turns & 1 else box))
    g = tuple(rect) + tuple(size)
    t = O.turn(R.resample(planes_k, W, H, g), g[4], g[5], turns)
    return O.turned_size(g[4], g[5], turns), t.reshape(-1), O.to_rgb(t, g[4], g[5], turns).reshape(-1)


def _run(d, data, name, fmt, env_extra, args=(), n=N, fail=False):
    d.mkdir()
    path = d / name
    np.asarray(data, np.uint8).tofile(path)
    env = {k: v for k, v in os.environ.items() if not k.startswith("MINIVIDEO_")}
    env.update(env_extra)
    r = subprocess.run([CLI, "-i", str(path), "-f", fmt, "-n", str(n), *args], cwd=d, capture_output=True, text=True, timeout=120, env=env)
    if fail:
        assert "decode did not succeed" in r.stderr, r.stderr
    else:
        assert r.returncode == 0 and "decode did not succeed" not in r.stderr, r.stderr
    return {f: (d / f).read_bytes() for f in sorted(os.listdir(d)) if f != name}, r.stderr


ON = {"MINIVIDEO_TRIM_LEVEL": str(LEVEL)}
CASES = {"alone": ([], None, 0), "box": (["-s", "40x40"], (40, 40), 0), "turned": (["-r", "90"], None, 1), "blank": (["-b"], None, 0)}


@pytest.mark.parametrize("case", list(CASES))
@pytest.mark.parametrize("fmt", ["yuv420", "png"])
def test_cli_trims(tmp_path, fmt, case):
    from tests.mp4mux import mux
    stream, planes = _pictures("bars")
    args, box, turns = CASES[case]
    ok, rect = _model_rect(planes, LEVEL)
    assert ok == 1 and rect != RECT                               # the scenario: the union of the probes is trusted and trims
    if case == "blank":                                           # every picture is busy over the trimmed rectangle: -b replaces none
        assert all(L.picture_score(planes[k], W, H, rect) > 16 * 256 for k in range(F))
    ext = "yuv" if fmt == "yuv420" else "png"
    names = [f"c_{k}.{ext}" for k in range(N)]
    es, _ = _run(tmp_path / "es", stream, "c.264", fmt, ON, ["-t"] + args)
    env, _ = _run(tmp_path / "env", stream, "c.264", fmt, dict(ON, MINIVIDEO_TRIM="1"), args)
    mp4, _ = _run(tmp_path / "mp4", np.frombuffer(mux(stream, W * 16, H * 16), np.uint8), "c.mp4", fmt, ON, ["-t"] + args)
    assert list(es) == list(env) == list(mp4) == names            # file names and counts do not change
    for k in range(N):
        (ow, oh), wy, wr = _expected(planes[k], rect, box, turns)
        if fmt == "yuv420":
            assert es[names[k]] == wy.tobytes(), k
        else:
            pix, w, h = _png_pixels(es[names[k]])
            assert (w, h) == (ow, oh) and np.array_equal(pix, wr), k
        assert env[names[k]] == es[names[k]] and mp4[names[k]] == es[names[k]], k


def test_cli_compressed_png_and_one_picture(tmp_path):
    """-z: the device's PNG files of the trimmed pictures; -n 1: the one picture is among the probes"""
    from tests import png_ref as P
    stream, planes = _pictures("bars")
    ok, rect = _model_rect(planes, LEVEL)
    assert ok == 1
    files, _ = _run(tmp_path / "z", stream, "c.264", "png", ON, ["-t", "-z"])
    for k in range(N):
        (ow, oh), _, wr = _expected(planes[k], rect, None, 0)
        assert files[f"c_{k}.png"] == bytes(P.encode(wr, ow, oh)), k
    one, err = _run(tmp_path / "one", stream, "c.264", "yuv420", dict(ON, MINIVIDEO_STATS="1"), ["-t"], n=1)
    assert list(one) == ["c.yuv"] and one["c.yuv"] == _expected(planes[0], rect, None, 0)[1].tobytes()
    assert "black bars:" in err and "applied" in err and "not applied" not in err
    few, _ = _run(tmp_path / "few", stream, "c.264", "yuv420", dict(ON, MINIVIDEO_TRIM_PROBES="2"), ["-t"])
    ok2, rect2 = _model_rect(planes, LEVEL, 2)                    # fewer probes: the model's union over THOSE pictures
    for k in range(N):
        assert few[f"c_{k}.yuv"] == _expected(planes[k], rect2 if ok2 else RECT, None, 0)[1].tobytes(), k


@pytest.mark.parametrize("kind,level", [("dark", 254), ("bars", B.LEVEL)])
def test_cli_nothing_to_trim_is_the_crop(tmp_path, kind, level):
    """a stream without a bright sample, and a stream without bars: the -c files byte for byte"""
    stream, planes = _pictures(kind)
    ok, rect = _model_rect(planes, level)
    assert (ok, rect) == ((0, RECT) if kind == "dark" else (1, RECT))
    for fmt in ("yuv420", "png"):
        crop, _ = _run(tmp_path / ("c_" + fmt), stream, "c.264", fmt, {}, ["-c"])
        trim, _ = _run(tmp_path / ("t_" + fmt), stream, "c.264", fmt, {"MINIVIDEO_TRIM_LEVEL": str(level)}, ["-t"])
        assert trim == crop and len(crop) == N
    boxed, _ = _run(tmp_path / "cs", stream, "c.264", "yuv420", {}, ["-c", "-s", "40x40"])
    boxed_t, _ = _run(tmp_path / "ts", stream, "c.264", "yuv420", {"MINIVIDEO_TRIM_LEVEL": str(level)}, ["-t", "-s", "40x40"])
    assert boxed_t == boxed


@pytest.mark.parametrize("var,value", [("MINIVIDEO_TRIM_LEVEL", "300"), ("MINIVIDEO_TRIM_PROBES", "0"), ("MINIVIDEO_TRIM", "x")])
def test_cli_malformed_switch_fails(tmp_path, var, value):
    stream, _ = _pictures("bars")
    for k, extra in enumerate(({"MINIVIDEO_TRIM": "1"}, {})):     # whether or not the feature is switched on
        files, err = _run(tmp_path / str(k), stream, "c.264", "yuv420", dict(extra, **{var: value}), fail=True)
        assert var in err and files == {}


def test_cli_without_the_switch(tmp_path):
    """0, the empty string and no switch at all: the coded pictures, as before; the other two variables alone change nothing"""
    stream, planes = _pictures("bars")
    want = {f"c_{k}.yuv": planes[k].tobytes() for k in range(N)}
    for k, env in enumerate(({}, {"MINIVIDEO_TRIM": "0"}, {"MINIVIDEO_TRIM": ""}, {"MINIVIDEO_TRIM_LEVEL": "200", "MINIVIDEO_TRIM_PROBES": "3"})):
        files, err = _run(tmp_path / str(k), stream, "c.264", "yuv420", dict(env, MINIVIDEO_STATS="1"))
        assert files == want and "black bars" not in err, env
