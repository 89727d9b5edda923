"""GPU: MINIVIDEO_SKIP_BLANK=1 through minivideo_decode -- the product CLI (also with its -b option) and the stock upstream
main.cpp built against this library.  The expected files are worked out from the oracle's planes, the scores of
tests/luma_ref.py and its restatement of the policy (which IDR every slot ends on, which alternates the second pass decodes);
bytes are compared for yuv420 / bmp, and for jpg against tests/jpeg_ref.py.  Streams mix busy and blank pictures
(tests/blank_streams.py) and every scenario first asserts that the threshold it passes separates the two."""
import os
import subprocess

import numpy as np
import pytest

from oracle import loader  # noqa: F401  (the planes come from it, through blank_streams)
from tests import blank_streams as B, jpeg_ref as J, luma_ref as L, resample_ref as R
from tests.test_gpu_api import _bmp

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CLI = os.path.join(ROOT, "minivideo_amd", "mini_thumbnailer")
STOCK = os.path.join(ROOT, "oracle", "_ref", "mini_thumbnailer_stock")
W, H = 20, 17
ON = {"MINIVIDEO_SKIP_BLANK": "1", "MINIVIDEO_BLANK_VARIANCE": str(B.VARIANCE)}

# name: (busy per picture, -n, -e, profile)
SCENARIOS = {
    "third": ([0, 0, 1, 0, 0], 1, "unfiltered", "high"),            # -n 1 on blank, blank, busy
    "none": ([0, 0, 0, 0], 1, "unfiltered", "high"),                # -n 1 on four blanks: the highest-scoring one
    "last_slot": ([1, 1, 0, 0, 1, 1], 3, "unfiltered", "high"),     # a blank last slot and busy pictures behind it
    "distributed": ([0, 0, 1] + [0] * 8 + [1] + [0] * 6, 3, "distributed", "baseline"),   # 16 sparse + 2 dense survive mean / 1.66
    "busy_only": ([1, 1, 1], 3, "unfiltered", "high"),
}
_CACHE = {}


def _content(name):
    if name not in _CACHE:
        busy, n, mode, profile = SCENARIOS[name]
        stream, _, planes, scores = B.mixed(W, H, busy, seed=5, profile=profile)
        assert all((v > B.MIN_SCORE) == bool(b) for v, b in zip(scores, busy)), scores     # the threshold separates the classes
        _CACHE[name] = (stream, planes, scores)
    return _CACHE[name]


def _run(exe, d, data, name, fmt, n, mode, env_extra, args=()):
    d.mkdir()
    path = d / name
    np.asarray(data, np.uint8).tofile(path)
    env = {k: v for k, v in os.environ.items() if not k.startswith("MINIVIDEO_")}
    env.update(env_extra)
    r = subprocess.run([str(exe), "-i", str(path), "-f", fmt, "-n", str(n), "-e", mode, *args], cwd=d, capture_output=True,
                       text=True, timeout=120, env=env)
    assert r.returncode == 0 and "decode did not succeed" not in r.stderr, r.stderr
    return {f: (d / f).read_bytes() for f in sorted(os.listdir(d)) if f != name}, r.stderr


def _names(n_files, n, ext):
    return ["c.%s" % ext] if n == 1 else ["c_%d.%s" % (k, ext) for k in range(n_files)]


def _geom(box=None):
    ow, oh = (16 * W, 16 * H) if box is None else R.fit(16 * W, 16 * H, *box)
    return (0, 0, 16 * W, 16 * H, ow, oh)


def _file(planes_k, fmt, g, quality=75):
    out = R.resample(planes_k, W, H, g)
    if fmt == "yuv420":
        return out.reshape(-1).tobytes()
    if fmt == "bmp":
        return _bmp(R.to_rgb(out, g[4], g[5]).reshape(-1), g[4], g[5])
    return J.encode(out.reshape(-1), g[4], g[5], quality)


def _slots(plain, planes, n):
    """which IDR every file of a run without the switch holds (its planes are the oracle's of exactly one picture)"""
    slots = []
    for name in _names(len(plain), n, "yuv"):
        hit = [k for k in range(planes.shape[0]) if plain[name] == planes[k].tobytes()]
        assert len(hit) == 1, name
        slots.append(hit[0])
    return slots


def _expected(planes, final, n, fmt, g, ext):
    return {name: _file(planes[idr], fmt, g) for name, idr in zip(_names(len(final), n, ext), final)}


@pytest.mark.parametrize("name", ["third", "none", "last_slot", "distributed"])
def test_blank_slots_give_way(tmp_path, name):
    from tests.mp4mux import mux
    busy, n, mode, _ = SCENARIOS[name]
    stream, planes, scores = _content(name)
    plain, _ = _run(CLI, tmp_path / "plain", stream, "c.264", "yuv420", n, mode, {})
    slots = _slots(plain, planes, n)
    if mode == "unfiltered":
        assert slots == list(range(n))
    final, second = L.policy(slots, scores, B.MIN_SCORE, 4)
    assert final != slots and second                                   # the scenario does move a slot
    if name == "third":
        assert final == [2]
    if name == "none":
        assert final == [int(np.argmax(scores[:5]))] and all(scores[i] < B.MIN_SCORE for i in final)
    if name == "last_slot":
        assert final == [0, 1, 4]
    if name == "distributed":
        assert any(not busy[i] for i in slots) and sum(1 for a, b in zip(slots, final) if a != b) >= 2
    want = _expected(planes, final, n, "yuv420", _geom(), "yuv")
    es, err = _run(CLI, tmp_path / "es", stream, "c.264", "yuv420", n, mode, dict(ON, MINIVIDEO_STATS="1"))
    assert es == want
    assert "%d alternates listed, %d entropy-decoded" % (len(second), len(second)) in err, err
    mp4, _ = _run(CLI, tmp_path / "mp4", np.frombuffer(mux(stream, W * 16, H * 16), np.uint8), "c.mp4", "yuv420", n, mode, ON)
    assert mp4 == want
    opt, _ = _run(CLI, tmp_path / "opt", stream, "c.264", "yuv420", n, mode, {"MINIVIDEO_BLANK_VARIANCE": str(B.VARIANCE)}, ["-b"])
    assert opt == want
    one, _ = _run(CLI, tmp_path / "batch1", stream, "c.264", "yuv420", n, mode, dict(ON, MINIVIDEO_BATCH="1"))
    assert one == want
    ctx, _ = _run(CLI, tmp_path / "ctx3", stream, "c.264", "yuv420", n, mode, dict(ON, MINIVIDEO_FAKE_GPUS="3", MINIVIDEO_HOST_THREADS="2"))
    assert ctx == want


def test_stock_front_end(tmp_path):
    if not os.path.exists(STOCK):
        pytest.skip("oracle/_ref/mini_thumbnailer_stock was not built")
    busy, n, mode, _ = SCENARIOS["last_slot"]
    stream, planes, scores = _content("last_slot")
    final, _ = L.policy(list(range(n)), scores, B.MIN_SCORE, 4)
    got, _ = _run(STOCK, tmp_path / "stock", stream, "c.264", "yuv420", n, mode, ON)
    assert got == _expected(planes, final, n, "yuv420", _geom(), "yuv")
    off, _ = _run(STOCK, tmp_path / "off", stream, "c.264", "yuv420", n, mode, {})
    assert off == _expected(planes, list(range(n)), n, "yuv420", _geom(), "yuv")


def test_one_alternate_only(tmp_path):
    busy, n, mode, _ = SCENARIOS["third"]
    stream, planes, scores = _content("third")
    final, second = L.policy([0], scores, B.MIN_SCORE, 1)
    assert second == [1] and final == [0 if scores[0] >= scores[1] else 1]           # the busy third picture is out of reach
    got, err = _run(CLI, tmp_path / "a1", stream, "c.264", "yuv420", n, mode, dict(ON, MINIVIDEO_BLANK_ALTERNATES="1", MINIVIDEO_STATS="1"))
    assert got == _expected(planes, final, n, "yuv420", _geom(), "yuv")
    assert "1 alternates listed, 1 entropy-decoded" in err, err


def test_a_failed_second_pass_write_keeps_the_first_file(tmp_path):
    """pass 2 writes beside the slot's file and renames: with that name taken by a directory every replacement fails, the file of
    pass 1 stays whole (it is what the return value counted) and the call still succeeds"""
    stream, planes, scores = _content("third")
    d = tmp_path / "w"
    d.mkdir()
    (d / "c.yuv.part").mkdir()
    np.asarray(stream, np.uint8).tofile(d / "c.264")
    env = {k: v for k, v in os.environ.items() if not k.startswith("MINIVIDEO_")}
    env.update(ON, MINIVIDEO_STATS="1")
    r = subprocess.run([CLI, "-i", str(d / "c.264"), "-f", "yuv420", "-n", "1", "-e", "unfiltered"], cwd=d, capture_output=True,
                       text=True, timeout=120, env=env)
    assert r.returncode == 0 and "decode did not succeed" not in r.stderr, r.stderr
    assert "Unable to write" in r.stderr and "0 files replaced" in r.stderr, r.stderr
    assert sorted(os.listdir(d)) == ["c.264", "c.yuv", "c.yuv.part"] and os.listdir(d / "c.yuv.part") == []
    assert (d / "c.yuv").read_bytes() == _file(planes[0], "yuv420", _geom())


def test_default_threshold_and_zero(tmp_path):
    """the default variance of 256 (score 4096) lies inside the blank class of this content -- some blank pictures pass it --
    and a variance of 0 calls nothing blank: both follow the restatement"""
    busy, n, mode, _ = SCENARIOS["last_slot"]
    stream, planes, scores = _content("last_slot")
    for var, thr in ((None, 4096), ("0", 0)):
        final, _ = L.policy(list(range(n)), scores, thr, 4)
        env = {"MINIVIDEO_SKIP_BLANK": "1"}
        if var is not None:
            env["MINIVIDEO_BLANK_VARIANCE"] = var
        got, _ = _run(CLI, tmp_path / ("v" + str(thr)), stream, "c.264", "yuv420", n, mode, env)
        assert got == _expected(planes, final, n, "yuv420", _geom(), "yuv")


def test_busy_pictures_only(tmp_path):
    """nothing is blank: the files are those of a run without the switch, and no second pass runs"""
    busy, n, mode, _ = SCENARIOS["busy_only"]
    stream, planes, scores = _content("busy_only")
    for fmt in ("bmp", "yuv420"):
        plain, _ = _run(CLI, tmp_path / ("plain_" + fmt), stream, "c.264", fmt, n, mode, {})
        got, err = _run(CLI, tmp_path / ("on_" + fmt), stream, "c.264", fmt, n, mode, dict(ON, MINIVIDEO_STATS="1"))
        assert got == plain == _expected(planes, [0, 1, 2], n, fmt, _geom(), "yuv" if fmt == "yuv420" else fmt)
        assert "0 of 3 slots score below" in err and "0 alternates listed, 0 entropy-decoded" in err, err
    off, err = _run(CLI, tmp_path / "off", stream, "c.264", "yuv420", n, mode, {"MINIVIDEO_SKIP_BLANK": "0", "MINIVIDEO_STATS": "1"})
    assert off == plain and "blank pictures" not in err


@pytest.mark.parametrize("fmt,args", [("bmp", []), ("jpg", ["-j"]), ("jpg", ["-j", "-s", "160x160"]), ("bmp", ["-s", "160x160"])])
def test_the_same_pictures_whatever_is_written(tmp_path, fmt, args):
    """the score is a property of the source picture: BMP, JPEG and 160-wide thumbnails end on the pictures yuv420 ends on"""
    busy, n, mode, _ = SCENARIOS["last_slot"]
    stream, planes, scores = _content("last_slot")
    final, _ = L.policy(list(range(n)), scores, B.MIN_SCORE, 4)
    g = _geom((160, 160) if "-s" in args else None)
    assert ("-s" not in args) or (g[4], g[5]) != (16 * W, 16 * H)
    got, _ = _run(CLI, tmp_path / "w", stream, "c.264", fmt, n, mode, ON, args)
    assert got == _expected(planes, final, n, fmt, g, fmt)
    third, _ = _run(CLI, tmp_path / "one", _content("third")[0], "c.264", fmt, 1, "unfiltered", ON, args)
    assert third == _expected(_content("third")[1], [2], 1, fmt, g, fmt)
