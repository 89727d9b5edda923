"""One corpus of seeded generator streams that every reference test shares (tests/test_reference_diff.py on the oracle,
tests/test_gpu_reference_diff.py on the kernels and the CLI), the digests the reference decoder gave for it
(tests/golden/reference_recon.json, written by tests/golden/make_reference_recon.py), and the CLI scenarios.

A case is a dict of gen.make_stream() arguments plus an id.  What it covers:
  * all six profiles, on the shapes the kernels' tests use (1x1 ... 64x5, 7x35);
  * heights 4 ... 15, every residue mod 4 and mod 8: the band seams of the wide / quad_wide / pipe / pipe1 forms;
  * 720p and 1080p on every profile, 2160p on High;
  * QP over 0..51 and narrow at 0..3, 34..38 (Intra16x16 at QP 36 allowed), 48..51;
  * chroma QP offsets (-12, -12), (12, 12), (-12, 12) and (12, -12);
  * large coefficient levels (clipping), sparse pictures, SPS / PPS before every picture."""
import hashlib
import json
import os

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden", "reference_recon.json")

PROFILES = ("baseline", "main_cavlc", "high_cavlc", "main", "high_4x4", "high")
SHAPES = ((1, 1), (2, 1), (1, 2), (3, 2), (5, 3), (11, 9), (20, 17), (64, 5), (7, 35))
OFFSETS = ((0, 0), (-12, -12), (12, 12), (-12, 12), (12, -12))


def _case(cid, W, H, F, seed, profile, qp_range=(0, 51), cqp_offsets=(0, 0), max_level=32, dense=True,
          sps_pps_every_frame=False, allow_qp36_i16=False):
    return {"id": cid, "width_mbs": W, "height_mbs": H, "n_frames": F, "seed": seed, "profile": profile, "dense": dense,
            "qp_range": list(qp_range), "cqp_offsets": list(cqp_offsets), "max_level": max_level,
            "sps_pps_every_frame": sps_pps_every_frame, "allow_qp36_i16": allow_qp36_i16}


def _corpus():
    out = []
    for pi, prof in enumerate(PROFILES):
        for si, (W, H) in enumerate(SHAPES):
            out.append(_case("shape-%s-%dx%d" % (prof, W, H), W, H, 2, 1000 + 10 * si + pi, prof,
                             cqp_offsets=OFFSETS[(si + pi) % len(OFFSETS)], allow_qp36_i16=(si % 2 == 1)))
    for prof in ("baseline", "main", "high"):
        for H in range(4, 16):
            out.append(_case("height-%s-6x%d" % (prof, H), 6, H, 2, 2000 + H, prof, cqp_offsets=OFFSETS[H % len(OFFSETS)]))
    for pi, prof in enumerate(PROFILES):
        out.append(_case("720p-%s" % prof, 80, 45, 1 + pi % 2, 3000 + pi, prof, qp_range=(10, 40)))
        out.append(_case("1080p-%s" % prof, 120, 68, 1 + (pi + 1) % 2, 3100 + pi, prof, qp_range=(10, 40)))
    out.append(_case("2160p-high", 240, 135, 2, 3200, "high", qp_range=(10, 40), cqp_offsets=(-3, 5)))
    for pi, prof in enumerate(PROFILES):
        for qi, qr in enumerate(((0, 3), (34, 38), (48, 51))):
            out.append(_case("qp%d-%d-%s" % (qr[0], qr[1], prof), 9, 6, 3, 4000 + 10 * pi + qi, prof, qp_range=qr,
                             cqp_offsets=OFFSETS[1 + (pi + qi) % 4], allow_qp36_i16=(qr == (34, 38))))
    for pi, prof in enumerate(PROFILES):
        out.append(_case("level2000-%s" % prof, 10, 7, 2, 5000 + pi, prof, max_level=2000, cqp_offsets=(-12, 12)))
        out.append(_case("sparse-%s" % prof, 13, 8, 3, 5100 + pi, prof, dense=False))
        out.append(_case("spspps-%s" % prof, 8, 5, 3, 5200 + pi, prof, sps_pps_every_frame=True, cqp_offsets=(12, 12)))
    return out


CORPUS = _corpus()
# 17 pictures each (prime: in a batch that repeats them, no two pictures of one group of four or eight are the same), for
# the batches of tests/test_gpu_reference_diff.py; in the corpus too, so that the oracle is held to them as well
BATCH_CASES = [_case("batch-%s-5x%d" % (prof, H), 5, H, 17, 6000 + H, prof, cqp_offsets=(-12, 12))
               for prof, H in (("high", 17), ("high", 68), ("baseline", 17))]
CORPUS += BATCH_CASES
BY_ID = {c["id"]: c for c in CORPUS}


def make(case):
    """(stream bytes as a uint8 array, packed records) of a corpus case"""
    from minivideo_amd import gen
    return gen.make_stream(case["width_mbs"], case["height_mbs"], case["n_frames"], seed=case["seed"], profile=case["profile"],
                           dense=case["dense"], cqp_offsets=tuple(case["cqp_offsets"]),
                           sps_pps_every_frame=case["sps_pps_every_frame"], qp_range=tuple(case["qp_range"]),
                           max_level=case["max_level"], allow_qp36_i16=case["allow_qp36_i16"])


def md5(b):
    if isinstance(b, np.ndarray):
        b = np.ascontiguousarray(b).tobytes()
    return hashlib.md5(b).hexdigest()


_GOLDEN = None


def golden():
    global _GOLDEN
    if _GOLDEN is None:
        with open(GOLDEN) as f:
            _GOLDEN = json.load(f)
    return _GOLDEN


def golden_case(case):
    """the recorded entry of a case; fails with 'regenerate' when the fixture no longer describes the corpus"""
    rec = golden()["cases"].get(case["id"])
    assert rec is not None, "%s not in %s: regenerate the fixture (tests/golden/make_reference_recon.py)" % (case["id"], GOLDEN)
    args = {k: v for k, v in case.items() if k != "id"}
    assert rec["args"] == args, "%s: arguments changed: regenerate the fixture (tests/golden/make_reference_recon.py)" % case["id"]
    return rec


def check_stream(case, stream):
    rec = golden_case(case)
    assert md5(stream) == rec["stream_md5"], ("%s: the generator's stream changed (md5): regenerate the fixture "
                                              "(tests/golden/make_reference_recon.py)" % case["id"])
    return rec


def reference_pictures(case, stream):
    """the reference decoder's pictures of a case: [(yuv420 bytes as uint8, RGB pixels from its BMP)], or None where the binary
    was not built (the recorded digests are the expected value there)"""
    from tests import refdec
    if not refdec.available():
        return None
    F = case["n_frames"]
    ys = refdec.pictures(stream, "yuv420", F)
    bs = refdec.pictures(stream, "bmp", F)
    W, H = 16 * case["width_mbs"], 16 * case["height_mbs"]
    out = []
    for y, b in zip(ys, bs):
        px, w, h = refdec.read_bmp(b)
        assert (w, h) == (W, H), (case["id"], w, h)
        out.append((np.frombuffer(y, np.uint8), px))
    return out


def locate(case, plane_kind, off):
    """picture-relative offset -> 'plane Y, macroblock 12 (x 3, y 1), pixel (50, 17)'"""
    W, H = case["width_mbs"], case["height_mbs"]
    if plane_kind == "rgb":
        pix, ch = divmod(off, 3)
        y, x = divmod(pix, 16 * W)
        return "RGB channel %d, macroblock %d (x %d, y %d), pixel (%d, %d)" % (ch, (y // 16) * W + x // 16, x // 16, y // 16, x, y)
    luma = 256 * W * H
    if off < luma:
        name, s, o = "Y", 16, off
    else:
        o = off - luma
        c, o = divmod(o, 64 * W * H)
        name, s = ("Cb", "Cr")[c], 8
    y, x = divmod(o, s * W)
    return "plane %s, macroblock %d (x %d, y %d), pixel (%d, %d)" % (name, (y // s) * W + x // s, x // s, y // s, x, y)


def compare(case, what, got_yuv, got_rgb, expected, rec):
    """got_yuv / got_rgb: all pictures of the case back to back; expected: reference_pictures() or None (then the recorded
    digests).  Raises naming the first differing picture, plane, macroblock and pixel."""
    F = case["n_frames"]
    yb = got_yuv.size // F
    rb = got_rgb.size // F
    for k in range(F):
        gy, gr = got_yuv[k * yb:(k + 1) * yb], got_rgb[k * rb:(k + 1) * rb]
        if expected is not None:
            ey, er = expected[k]
            for kind, g, e in (("yuv", gy, ey), ("rgb", gr, er)):
                assert g.size == e.size, "%s %s: picture %d: %d bytes, reference %d" % (case["id"], what, k, g.size, e.size)
                bad = np.nonzero(g != e)[0]
                if bad.size:
                    o = int(bad[0])
                    raise AssertionError("%s %s: picture %d: %d %s bytes differ from the reference decoder; first at %s "
                                         "(got %d, reference %d)" % (case["id"], what, k, bad.size, kind.upper(),
                                                                      locate(case, kind, o), g[o], e[o]))
        else:
            pic = rec["pictures"][k]
            assert md5(gy) == pic["yuv420"], "%s %s: picture %d: YUV differs from the reference's recorded yuv420 (md5)" % (
                case["id"], what, k)
            assert md5(gr) == pic["bmp_rgb"], "%s %s: picture %d: RGB differs from the reference's recorded BMP pixels (md5)" % (
                case["id"], what, k)


# ---- CLI scenarios: the whole product against the reference tool, file for file ----

def _mixed_stream(W, H, F, seed, profile):
    """F one-picture streams concatenated with one SPS / PPS at the start, every third picture sparse: pictures of
    different sizes, so that the reference's size filter (filter.c:94-211) has something to drop"""
    from minivideo_amd import gen
    parts = []
    for k in range(F):
        st, _ = gen.make_stream(W, H, 1, seed=seed + k, profile=profile, dense=(k % 3 != 1), want_packed=False)
        b = st.tobytes()
        if k:
            b = b[b.index(b"\x00\x00\x00\x01\x65"):]
        parts.append(b.rstrip(b"\x00") if k < F - 1 else b)
    return b"".join(parts)


def _broken_stream():
    """the stream of test_gpu_api.py::test_cli_skips_broken_picture: the 2nd IDR's slice type made P"""
    from minivideo_amd import gen
    stream, _ = gen.make_stream(6, 4, 4, seed=35, profile="baseline")
    b = bytearray(stream.tobytes())
    idx = [i for i in range(len(b) - 5) if b[i:i + 5] == b"\x00\x00\x00\x01\x65"]
    b[idx[1] + 5] = 0xA0
    return bytes(b)


def cli_input(scn, for_reference=False):
    """(file name, bytes) of a CLI scenario's input.  for_reference: what the reference tool is given instead -- for an MP4
    scenario the same stream as Annex B under the same base name: the reference hands an MP4 track's length-prefixed
    samples to its NAL parser as they are ("Unsupported NAL Unit (nal_unit_type 0)") and writes no picture, where the
    product demuxes them"""
    from minivideo_amd import gen
    src = scn["input"]
    if src == "mixed120":
        data = _mixed_stream(6, 4, 120, 700, "baseline")
    elif src == "broken":
        data = _broken_stream()
    else:
        W, H, F, seed, prof = src
        data = gen.make_stream(W, H, F, seed=seed, profile=prof, want_packed=False)[0].tobytes()
        if scn.get("mp4") and for_reference:
            return os.path.splitext(scn["name"])[0] + ".264", data
        if scn.get("mp4"):
            from tests.mp4mux import mux
            data = mux(np.frombuffer(data, np.uint8), W * 16, H * 16, extra_non_sync=True, samples_per_chunk=3)
    return scn["name"], data


def _cli_scenarios():
    out = []
    for fmt in ("yuv420", "yuv444", "bmp", "tga", "png", None):
        for prof in ("baseline", "high"):
            out.append({"id": "fmt-%s-%s" % (fmt or "default", prof), "input": [7, 5, 3, 800, prof], "name": "p.264",
                        "fmt": fmt, "n": 3, "mode": None})
    out.append({"id": "one-picture-bmp", "input": [9, 6, 2, 801, "high"], "name": "movie.h264", "fmt": "bmp", "n": None,
                "mode": None})
    for n in (1, 5, 100):
        out.append({"id": "n%d" % n, "input": "mixed120", "name": "long.264", "fmt": "yuv420", "n": n, "mode": None})
    for mode in ("unfiltered", "ordered", "distributed"):
        out.append({"id": "mode-%s" % mode, "input": "mixed120", "name": "sel.264", "fmt": "yuv420", "n": 7, "mode": mode})
    out.append({"id": "mode-ordered-n100", "input": "mixed120", "name": "sel.264", "fmt": "yuv420", "n": 100, "mode": "ordered"})
    out.append({"id": "annexb", "input": [12, 9, 4, 37, "high"], "name": "clip.264", "fmt": "yuv420", "n": 4, "mode": None})
    out.append({"id": "mp4", "input": [12, 9, 4, 37, "high"], "mp4": True, "name": "clip.mp4", "fmt": "yuv420", "n": 4,
                "mode": None})
    out.append({"id": "mp4-bmp", "input": [12, 9, 4, 37, "high"], "mp4": True, "name": "clip.mp4", "fmt": "bmp", "n": 4,
                "mode": "distributed"})
    # the reference decodes the broken picture's slice as a P slice and dies of SIGSEGV after writing the first picture's file
    # (the product skips the picture instead: INTEGRATION.md); what it wrote before is still compared (prefix=True)
    out.append({"id": "broken-picture-n1", "input": "broken", "name": "s.264", "fmt": "yuv420", "n": 1, "mode": None})
    out.append({"id": "broken-picture", "input": "broken", "name": "s.264", "fmt": "yuv420", "n": 3, "mode": None,
                "prefix": True})
    return out


CLI_SCENARIOS = _cli_scenarios()


def file_digest(fname, data):
    """what is compared of a file: its bytes, or its pixels for PNG (zlib streams of two encoders need not agree)"""
    if fname.endswith(".png"):
        from tests import refdec
        px, w, h = refdec.read_png(data)
        return "png %dx%d %s" % (w, h, md5(px))
    return md5(data)


def cli_digests(files):
    return {k: file_digest(k, v) for k, v in sorted(files.items())}
