"""GPU: MINIVIDEO_REPRESENTATIVE=1 through minivideo_decode -- the product CLI, also with its -p option.  The streams
(tests/represent_streams.py) are built so that the reference rule alone (tests/hist_ref.py over the oracle's planes, checked on
the CPU when the stream is made) picks a known picture for every slot by a clear margin.  A slot's file must then be, byte for
byte, the file an unfiltered run WITHOUT the switch writes for that IDR -- in yuv420, bmp, -j jpg and -z png -- so no encoder is
restated here; the stats line says which passes ran and over which pictures."""
import os
import subprocess

import numpy as np
import pytest

from tests import blank_streams as B, represent_streams as S

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CLI = os.path.join(ROOT, "minivideo_amd", "mini_thumbnailer")
ON = {"MINIVIDEO_REPRESENTATIVE": "1", "MINIVIDEO_STATS": "1"}
FORMATS = {"yuv420": ("yuv420", [], "yuv"), "bmp": ("bmp", [], "bmp"), "jpg": ("jpg", ["-j"], "jpg"), "png": ("png", ["-z"], "png")}


def _run(d, stream, fmt, n, env_extra, args=()):
    d.mkdir()
    np.asarray(stream, np.uint8).tofile(d / "c.264")
    env = {k: v for k, v in os.environ.items() if not k.startswith("MINIVIDEO_")}
    env.update(env_extra)
    r = subprocess.run([CLI, "-i", str(d / "c.264"), "-f", fmt, "-n", str(n), "-e", "unfiltered", *args], cwd=d, capture_output=True,
                       text=True, timeout=120, env=env)
    assert r.returncode == 0 and "decode did not succeed" not in r.stderr, r.stderr
    return {f: (d / f).read_bytes() for f in sorted(os.listdir(d)) if f != "c.264"}, r.stderr


def _names(n_files, n, ext):
    return ["c.%s" % ext] if n == 1 else ["c_%d.%s" % (k, ext) for k in range(n_files)]


def _every_picture(tmp_path, stream, n_idr, fmt):
    """the file an unfiltered run without the switch writes for every IDR of the stream"""
    f, args, ext = FORMATS[fmt]
    files, _ = _run(tmp_path / ("all_" + fmt), stream, f, n_idr, {}, args)
    assert sorted(files) == sorted(_names(n_idr, n_idr, ext))
    return [files[name] for name in _names(n_idr, n_idr, ext)]


def _lists(err):
    line = [l for l in err.splitlines() if "representative pictures: pass 2 order:" in l]
    assert len(line) == 1, err
    two, three = line[0].split("pass 2 order:")[1].split("; pass 3 order:")
    return [[] if part.strip() == "none" else [int(v) for v in part.split()] for part in (two, three)]


@pytest.mark.parametrize("fmt", ["yuv420", "bmp", "jpg", "png"])
@pytest.mark.parametrize("name", ["outlier", "second_slot"])
def test_the_slot_gets_the_representative_picture(tmp_path, name, fmt):
    letters, n, final, _ = S.SCENARIOS[name]
    stream, planes, _, _ = S.scenario(name)
    f, args, ext = FORMATS[fmt]
    every = _every_picture(tmp_path, stream, len(letters), fmt)
    if fmt == "yuv420":
        assert every == [p.tobytes() for p in planes]                      # file k of the plain run is IDR k, the oracle's planes
    want = dict(zip(_names(n, n, ext), [every[i] for i in final]))
    plain, err0 = _run(tmp_path / "plain", stream, f, n, {"MINIVIDEO_STATS": "1"}, args)
    assert plain == dict(zip(_names(n, n, ext), every[:n])) and plain != want and "representative pictures" not in err0
    got, err = _run(tmp_path / "on", stream, f, n, ON, args)
    assert got == want
    moved = [b for a, b in zip(range(n), final) if a != b]
    assert _lists(err) == [list(range(n, len(letters))), moved], err        # only the last slot has alternates; pass 3: the winners
    assert "%d slots, %d candidates listed, %d decoded, %d files replaced" % (n, len(letters) - n, len(letters) - n, len(moved)) in err, err


def test_option_batches_and_contexts(tmp_path):
    """-p equals the environment variable; batches of one picture and three contexts give the same files"""
    letters, n, final, _ = S.SCENARIOS["second_slot"]
    stream, planes, _, _ = S.scenario("second_slot")
    want = dict(zip(_names(n, n, "yuv"), [planes[i].tobytes() for i in final]))
    opt, _ = _run(tmp_path / "opt", stream, "yuv420", n, {}, ["-p"])
    assert opt == want
    one, _ = _run(tmp_path / "batch1", stream, "yuv420", n, dict(ON, MINIVIDEO_BATCH="1"))
    assert one == want
    ctx, _ = _run(tmp_path / "ctx3", stream, "yuv420", n, dict(ON, MINIVIDEO_FAKE_GPUS="3", MINIVIDEO_HOST_THREADS="2"))
    assert ctx == want
    few, err = _run(tmp_path / "alts2", stream, "yuv420", n, dict(ON, MINIVIDEO_REPRESENTATIVE_ALTERNATES="2"))
    assert _lists(err)[0] == [2, 3]                                          # p, B, A: three candidates, the rule's own answer
    from tests import hist_ref as R
    recs = S.scenario("second_slot")[3]
    assert few == dict(zip(_names(n, n, "yuv"), [planes[0].tobytes(), planes[[1, 2, 3][R.choose(recs[[1, 2, 3]])]].tobytes()]))


@pytest.mark.parametrize("name", ["primary_wins", "all_slots"])
def test_files_that_stay(tmp_path, name):
    """a slot whose primary wins and slots without alternates keep the files of pass 1, and pass 3 does not run"""
    letters, n, final, _ = S.SCENARIOS[name]
    stream, planes, _, _ = S.scenario(name)
    assert final == list(range(n))
    for fmt in ("yuv420", "bmp"):
        f, args, ext = FORMATS[fmt]
        plain, _ = _run(tmp_path / ("plain_" + fmt), stream, f, n, {}, args)
        got, err = _run(tmp_path / ("on_" + fmt), stream, f, n, ON, args)
        assert got == plain and sorted(got) == sorted(_names(n, n, ext))
        assert _lists(err) == [list(range(n, len(letters))), []] and "0 files replaced" in err and "pass 3 0.000 s (0 entropy-decoded)" in err, err


def test_blank_candidates_are_not_chosen(tmp_path):
    """three blank pictures among five candidates win the vote; with -b as well they are not eligible, two candidates are left
    and the primary stays.  Blank skipping's own pass does not run."""
    letters, n, final, final_b = S.SCENARIOS["blank_majority"]
    stream, planes, scores, _ = S.scenario("blank_majority")
    assert final == [1] and scores[1] < B.MIN_SCORE and final_b == [0] and scores[0] >= B.MIN_SCORE
    got, err = _run(tmp_path / "on", stream, "yuv420", n, ON)
    assert got == {"c.yuv": planes[1].tobytes()} and _lists(err) == [[1, 2, 3, 4], [1]]
    both, err = _run(tmp_path / "both", stream, "yuv420", n, dict(ON, MINIVIDEO_BLANK_VARIANCE=str(B.VARIANCE), MINIVIDEO_BLANK_ALTERNATES="1"), ["-b"])
    assert both == {"c.yuv": planes[0].tobytes()} and _lists(err) == [[1, 2, 3, 4], []]
    assert "blank pictures:" not in err
    # a blank primary among blank and busy alternates: the busy ones are compared
    letters, n, final, final_b = S.SCENARIOS["outlier"]
    stream, planes, scores, _ = S.scenario("outlier")
    assert scores[0] < B.MIN_SCORE
    both, err = _run(tmp_path / "both2", stream, "yuv420", n, dict(ON, MINIVIDEO_SKIP_BLANK="1", MINIVIDEO_BLANK_VARIANCE=str(B.VARIANCE)))
    assert both == {"c.yuv": planes[final_b[0]].tobytes()}


def test_switch_off_is_todays_behaviour(tmp_path):
    """MINIVIDEO_REPRESENTATIVE=0 and unset: the files of a plain run; with MINIVIDEO_SKIP_BLANK alone: blank skipping as it is"""
    from tests import luma_ref as L
    letters, n, _, _ = S.SCENARIOS["outlier"]
    stream, planes, scores, _ = S.scenario("outlier")
    plain, _ = _run(tmp_path / "plain", stream, "yuv420", n, {})
    off, err = _run(tmp_path / "off", stream, "yuv420", n, {"MINIVIDEO_REPRESENTATIVE": "0", "MINIVIDEO_STATS": "1"})
    assert off == plain == {"c.yuv": planes[0].tobytes()} and "representative pictures" not in err
    blank, err = _run(tmp_path / "blank", stream, "yuv420", n, {"MINIVIDEO_SKIP_BLANK": "1", "MINIVIDEO_BLANK_VARIANCE": str(B.VARIANCE),
                                                                 "MINIVIDEO_STATS": "1"})
    final, second = L.policy([0], scores, B.MIN_SCORE, 4)
    assert final == [1] and blank == {"c.yuv": planes[1].tobytes()}          # the first busy picture, not the representative one
    assert "%d alternates listed" % len(second) in err and "representative pictures" not in err


def test_a_failed_replacement_keeps_the_first_file(tmp_path):
    """pass 3 writes beside the slot's file and renames: with that name taken by a directory the replacement fails, the file of
    pass 1 stays whole and the call still succeeds"""
    stream, planes, _, _ = S.scenario("outlier")
    d = tmp_path / "w"
    d.mkdir()
    (d / "c.yuv.part").mkdir()
    np.asarray(stream, np.uint8).tofile(d / "c.264")
    env = {k: v for k, v in os.environ.items() if not k.startswith("MINIVIDEO_")}
    env.update(ON)
    r = subprocess.run([CLI, "-i", str(d / "c.264"), "-f", "yuv420", "-n", "1", "-e", "unfiltered"], cwd=d, capture_output=True, text=True,
                       timeout=120, env=env)
    assert r.returncode == 0 and "decode did not succeed" not in r.stderr, r.stderr
    assert "Unable to write" in r.stderr and "0 files replaced" in r.stderr, r.stderr
    assert sorted(os.listdir(d)) == ["c.264", "c.yuv", "c.yuv.part"] and os.listdir(d / "c.yuv.part") == []
    assert (d / "c.yuv").read_bytes() == planes[0].tobytes()


@pytest.mark.parametrize("var,bad", [("MINIVIDEO_REPRESENTATIVE", "yes"), ("MINIVIDEO_REPRESENTATIVE_ALTERNATES", "0"),
                                     ("MINIVIDEO_REPRESENTATIVE_ALTERNATES", "17")])
def test_malformed_values_fail_the_call(tmp_path, var, bad):
    stream, _, _, _ = S.scenario("all_slots")
    np.asarray(stream, np.uint8).tofile(tmp_path / "c.264")
    env = {k: v for k, v in os.environ.items() if not k.startswith("MINIVIDEO_")}
    env[var] = bad
    r = subprocess.run([CLI, "-i", str(tmp_path / "c.264"), "-f", "yuv420", "-n", "2"], cwd=tmp_path, capture_output=True, text=True,
                       timeout=60, env=env)
    assert var in r.stderr and "'%s'" % bad in r.stderr and "decode did not succeed" in r.stderr, r.stdout + r.stderr
    assert sorted(os.listdir(tmp_path)) == ["c.264"]
