"""The CPU checker against the reference decoder itself: host front end + oracle/recon_ref.c on every stream of the corpus
(tests/refcorpus.py) compared with what upstream MiniVideo's own mini_thumbnailer writes (oracle/_ref/mini_thumbnailer_ref,
built by __graft_entry__.build() where an upstream checkout is present), picture by picture, YUV bytes and RGB pixels.  The
same comparison against the recorded digests (tests/golden/reference_recon.json) runs without the binary."""
import os
import subprocess

import numpy as np
import pytest

from oracle import loader
from tests import refcorpus, refdec
from tests.util import Stream

IDS = [c["id"] for c in refcorpus.CORPUS]


def _oracle(case, stream):
    """front end + oracle: (yuv, rgb) of every picture of the stream, back to back"""
    F = case["n_frames"]
    with Stream(stream) as s:
        assert s.ok and s.idr_count == F, (case["id"], s.error())
        p = s.params(0)
        recs = []
        for k in range(F):
            rc, rec = s.packed(k)
            assert rc == 1, (case["id"], k, s.error())
            recs.append(rec)
    return loader.recon(p, np.concatenate(recs), F, want_rgb=True)


@pytest.mark.parametrize("cid", IDS)
def test_oracle_equals_reference_decoder(cid):
    case = refcorpus.BY_ID[cid]
    refdec.require()
    stream, _ = refcorpus.make(case)
    rec = refcorpus.check_stream(case, stream)
    expected = refcorpus.reference_pictures(case, stream)
    yuv, rgb = _oracle(case, stream)
    refcorpus.compare(case, "oracle", yuv, rgb, expected, rec)


@pytest.mark.parametrize("cid", IDS)
def test_oracle_equals_recorded_reference(cid):
    case = refcorpus.BY_ID[cid]
    stream, _ = refcorpus.make(case)
    rec = refcorpus.check_stream(case, stream)
    assert len(rec["pictures"]) == case["n_frames"]
    yuv, rgb = _oracle(case, stream)
    refcorpus.compare(case, "oracle", yuv, rgb, None, rec)


def test_corpus_covers_what_it_claims():
    cases = refcorpus.CORPUS
    assert {c["profile"] for c in cases} == set(refcorpus.PROFILES)
    for prof in refcorpus.PROFILES:
        shapes = {(c["width_mbs"], c["height_mbs"]) for c in cases if c["profile"] == prof}
        assert set(refcorpus.SHAPES) <= shapes and {(80, 45), (120, 68)} <= shapes, prof
    assert any(c["width_mbs"] == 240 and c["height_mbs"] == 135 for c in cases)
    heights = {c["height_mbs"] for c in cases}
    assert {h % 8 for h in heights} == set(range(8))
    assert {(c["qp_range"][0], c["qp_range"][1]) for c in cases} >= {(0, 51), (0, 3), (34, 38), (48, 51)}
    assert any(c["allow_qp36_i16"] and c["qp_range"] == [34, 38] for c in cases)
    assert {tuple(c["cqp_offsets"]) for c in cases} >= {(-12, -12), (12, 12), (-12, 12)}
    assert any(c["max_level"] >= 2000 for c in cases) and any(not c["dense"] for c in cases)
    assert any(c["sps_pps_every_frame"] for c in cases)
    assert all(c["n_frames"] <= 100 for c in cases)           # the reference's -n range


def test_recorded_reference_is_small_data():
    assert os.path.getsize(refcorpus.GOLDEN) < 256 * 1024
    assert set(refcorpus.golden()["cases"]) == set(IDS)
    assert set(refcorpus.golden()["cli"]) == {s["id"] for s in refcorpus.CLI_SCENARIOS}


def test_reference_tool_is_static():
    """a dynamically linked reference tool could load this repository's libminivideo.so (same name) through
    LD_LIBRARY_PATH and compare the product with itself"""
    exe = refdec.require()
    dyn = subprocess.run(["readelf", "-d", exe], capture_output=True, text=True, check=True).stdout
    needed = [ln for ln in dyn.splitlines() if "(NEEDED)" in ln]
    assert needed, dyn
    assert not any("minivideo" in ln for ln in needed), needed
    with open(exe, "rb") as f:
        assert b"minivideo_decode" in f.read()                # the library is inside


@pytest.mark.parametrize("scn", refcorpus.CLI_SCENARIOS, ids=lambda s: s["id"])
def test_reference_cli_matches_recorded(tmp_path, scn):
    """the reference binary still writes what the fixture recorded for the CLI scenarios (the GPU tests' expected value where
    no binary exists)"""
    exe = refdec.require()
    rec = refcorpus.golden()["cli"][scn["id"]]
    assert rec["scenario"] == scn, "%s: scenario changed: regenerate the fixture" % scn["id"]
    assert refcorpus.md5(refcorpus.cli_input(scn)[1]) == rec["input_md5"], "%s: input changed: regenerate the fixture" % scn["id"]
    name, data = refcorpus.cli_input(scn, for_reference=True)
    assert refcorpus.md5(data) == rec["reference_input_md5"]
    r, files = refdec.run_cli(exe, data, name, fmt=scn["fmt"], n=scn["n"], mode=scn["mode"], cwd=tmp_path / "ref")
    assert r.returncode == rec["returncode"], (scn["id"], r.returncode)
    assert files and refcorpus.cli_digests(files) == rec["files"]


def test_reference_rgb_formats_agree(tmp_path):
    """the readers: BMP, TGA and PNG (and the jpg -> png fallback) of the same pictures give the same pixels, and those are
    the oracle's"""
    refdec.require()
    case = refcorpus.BY_ID["shape-high-11x9"]
    stream, _ = refcorpus.make(case)
    yuv, rgb = _oracle(case, stream)
    F = case["n_frames"]
    rb = rgb.size // F
    for fmt in ("bmp", "tga", "png", "jpg"):
        for k, data in enumerate(refdec.pictures(stream, fmt, F)):
            px, w, h = refdec.read_rgb(fmt, data)
            assert (w, h) == (16 * case["width_mbs"], 16 * case["height_mbs"])
            assert np.array_equal(px, rgb[k * rb:(k + 1) * rb]), (fmt, k)


def test_png_reader_handles_every_filter():
    """read_png on a picture written with each of the five row filters in turn"""
    import struct
    import zlib
    rng = np.random.default_rng(3)
    w, h = 5, 10
    img = rng.integers(0, 256, (h, w * 3), dtype=np.int32)
    raw = b""
    prev = np.zeros(w * 3, np.int32)
    for y in range(h):
        ft = y % 5
        cur = img[y]
        left = np.concatenate([np.zeros(3, np.int32), cur[:-3]])
        upleft = np.concatenate([np.zeros(3, np.int32), prev[:-3]])
        if ft == 0:
            pred = np.zeros_like(cur)
        elif ft == 1:
            pred = left
        elif ft == 2:
            pred = prev
        elif ft == 3:
            pred = (left + prev) >> 1
        else:
            pred = np.array([refdec._paeth(int(a), int(b), int(c)) for a, b, c in zip(left, prev, upleft)], np.int32)
        raw += bytes([ft]) + ((cur - pred) & 255).astype(np.uint8).tobytes()
        prev = cur

    def chunk(t, body):
        return struct.pack(">I", len(body)) + t + body + struct.pack(">I", zlib.crc32(t + body) & 0xffffffff)

    png = (b"\x89PNG\r\n\x1a\n" + chunk(b"IHDR", struct.pack(">IIBBBBB", w, h, 8, 2, 0, 0, 0))
           + chunk(b"IDAT", zlib.compress(raw)) + chunk(b"IEND", b""))
    px, pw, ph = refdec.read_png(png)
    assert (pw, ph) == (w, h) and np.array_equal(px, img.astype(np.uint8).reshape(-1))
