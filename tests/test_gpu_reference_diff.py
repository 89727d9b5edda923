"""GPU against the reference decoder itself (upstream MiniVideo's mini_thumbnailer, oracle/_ref/mini_thumbnailer_ref): the
reference's files are the expected value here, the oracle is not used.  Where the binary was not built (no upstream checkout
on the box that built the tree) the digests it recorded in tests/golden/reference_recon.json are.

  * every corpus case (tests/refcorpus.py) on every kernel form, fused and separate colour conversion;
  * batches of distinct neighbours through the automatic form choice, every multi-picture form launched;
  * the product's CLI and the stock upstream main.cpp on the product's library against the reference tool, file for file."""
import os

import numpy as np
import pytest

from minivideo_amd import HotPath
from tests import refcorpus, refdec
from tests.util import Stream

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CLI = os.path.join(ROOT, "minivideo_amd", "mini_thumbnailer")
STOCK_CLI = os.path.join(ROOT, "oracle", "_ref", "mini_thumbnailer_stock")


def _front_end(stream, F):
    with Stream(stream) as s:
        assert s.ok and s.idr_count == F, s.error()
        p = s.params(0)
        recs = []
        for k in range(F):
            rc, rec = s.packed(k)
            assert rc == 1, (k, s.error())
            recs.append(rec)
    return p, np.concatenate(recs)


_EXPECTED = {}


def _expected(case, stream):
    """the reference's pictures of a case, decoded once per session (every form compares with the same files)"""
    if case["id"] not in _EXPECTED:
        _EXPECTED[case["id"]] = refcorpus.reference_pictures(case, stream)
    return _EXPECTED[case["id"]]


@pytest.mark.parametrize("cid", [c["id"] for c in refcorpus.CORPUS])
def test_kernels_equal_reference_decoder(hot, cid):
    case = refcorpus.BY_ID[cid]
    stream, _ = refcorpus.make(case)
    rec = refcorpus.check_stream(case, stream)
    expected = _expected(case, stream)
    p, packed = _front_end(stream, case["n_frames"])
    try:
        for fused in (True, False):
            hot.set_fused_color(fused)
            yuv, rgb = hot.recon_host(p, packed, case["n_frames"], want_rgb=True)
            refcorpus.compare(case, "%s (%s colour)" % (hot.last_launch()[0], "fused" if fused else "separate"),
                              yuv, rgb, expected, rec)
    finally:
        hot.set_fused_color(True)


# ---- batches of distinct neighbours through the automatic choice ----

# batch sizes: ints are pictures, floats multiples of the device's CUs (made odd, so that no size is a multiple of four or
# eight), on both sides of pick_layout's thresholds (launch_plan.hip).  With C CUs, rows of 5 macroblocks: High, 17 rows: pipe1
# up to 46 C row-waves (2.7 C pictures), quad_wide up to 3.36 C pictures, quad above, quad_wide again beyond 4 C; 68 rows:
# wide between 46 C and 76 C row-waves; Baseline: pipe for one picture, pipe1 up to 18 C row-waves (1.06 C pictures), pipe up
# to 2 C, quad_wide up to 3.36 C, quad, quad_wide again beyond 4 C, oct from about 6.8 C
BATCH_SIZES = {
    "batch-high-5x17": (1, 5, 2.65, 2.76, 3.3, 3.42, 3.9, 4.4, 7.9),
    "batch-high-5x68": (0.62, 0.72, 0.8, 1.15),
    "batch-baseline-5x17": (1, 3, 1.0, 1.1, 1.9, 2.1, 3.3, 3.42, 3.9, 6.5, 7.1, 7.9),
}
AUTO_FORMS = {"pipe", "pipe1", "wide", "quad_wide", "quad", "oct"}   # every form the automatic choice has


def _n_cus():
    import torch
    return torch.cuda.get_device_properties(0).multi_processor_count


def test_auto_batches_of_distinct_pictures_equal_reference():
    C = _n_cus()
    launched = {}
    h = HotPath(0)
    try:
        h.set_layout("auto")
        for case in refcorpus.BATCH_CASES:
            key, F = case["id"], case["n_frames"]
            stream, _ = refcorpus.make(case)
            rec = refcorpus.check_stream(case, stream)
            ref = _expected(case, stream)
            p, packed = _front_end(stream, F)
            pb = packed.size // F
            for f in BATCH_SIZES[key]:
                n = f if isinstance(f, int) else int(f * C) | 1
                idx = np.arange(n) % F
                yuv, rgb = h.recon_host(p, packed.reshape(F, pb)[idx].reshape(-1), n, want_rgb=True)
                form, waves = h.last_launch()
                launched.setdefault(form, []).append("%s x %d" % (key, n))
                print("auto: %s, %d pictures -> %s (%d waves)" % (key, n, form, waves))
                yuv = yuv.reshape(n, -1)
                rgb = rgb.reshape(n, -1)
                for i in range(n):
                    k = int(idx[i])
                    if ref is not None:
                        ok_y, ok_rgb = np.array_equal(yuv[i], ref[k][0]), np.array_equal(rgb[i], ref[k][1])
                    else:
                        pic = rec["pictures"][k]
                        ok_y, ok_rgb = refcorpus.md5(yuv[i]) == pic["yuv420"], refcorpus.md5(rgb[i]) == pic["bmp_rgb"]
                    if not (ok_y and ok_rgb):
                        where = ""
                        if ref is not None:
                            kind, g, e = ("yuv", yuv[i], ref[k][0]) if not ok_y else ("rgb", rgb[i], ref[k][1])
                            where = ", first at " + refcorpus.locate(case, kind, int(np.nonzero(g != e)[0][0]))
                        raise AssertionError("%s: batch of %d on %s: picture %d (stream picture %d): %s differs from the "
                                             "reference%s" % (key, n, form, i, k, "YUV" if not ok_y else "RGB", where))
    finally:
        h.close()
    print("auto routing launched: " + "; ".join("%s: %s" % (k, ", ".join(v)) for k, v in sorted(launched.items())))
    missing = AUTO_FORMS - set(launched)
    assert not missing, "auto routing never launched %s on %d CUs (launched: %s)" % (sorted(missing), C, sorted(launched))


# ---- the product against the reference tool, file for file ----

def _cli_check(exe, scn, tmp_path, tag):
    rec = refcorpus.golden()["cli"][scn["id"]]
    name, data = refcorpus.cli_input(scn)
    assert refcorpus.md5(data) == rec["input_md5"], "%s: input changed: regenerate the fixture" % scn["id"]
    if refdec.available():
        ref_name, ref_data = refcorpus.cli_input(scn, for_reference=True)   # (MP4: the same stream as Annex B)
        r, ref_files = refdec.run_cli(refdec.REF_CLI, ref_data, ref_name, fmt=scn["fmt"], n=scn["n"], mode=scn["mode"],
                                      cwd=tmp_path / "ref")
        assert r.returncode == rec["returncode"], (scn["id"], r.returncode)
        want = refcorpus.cli_digests(ref_files)
    else:
        ref_files, want = None, rec["files"]
    r, files = refdec.run_cli(exe, data, name, fmt=scn["fmt"], n=scn["n"], mode=scn["mode"], cwd=tmp_path / tag)
    assert r.returncode == 0, (tag, r.stderr.decode(errors="replace")[-2000:])
    got = refcorpus.cli_digests(files)
    if scn.get("prefix"):   # the reference died part way (refcorpus.py): what it wrote before must be ours
        assert want and set(want) <= set(got), (tag, sorted(want), sorted(got))
        got = {k: got[k] for k in want}
    if got != want:
        diff = sorted(set(got) ^ set(want))
        assert not diff, "%s %s: file names differ from the reference tool's: %s" % (tag, scn["id"], diff)
        bad = [k for k in want if got[k] != want[k]]
        detail = ""
        if ref_files is not None and not bad[0].endswith(".png"):
            a, b = np.frombuffer(files[bad[0]], np.uint8), np.frombuffer(ref_files[bad[0]], np.uint8)
            if a.size == b.size:
                detail = " (first differing byte at %d of %d)" % (int(np.nonzero(a != b)[0][0]), a.size)
        raise AssertionError("%s %s: %d of %d files differ from the reference tool's, first %s%s" % (
            tag, scn["id"], len(bad), len(want), bad[0], detail))


@pytest.mark.parametrize("scn", refcorpus.CLI_SCENARIOS, ids=lambda s: s["id"])
def test_cli_equals_reference_tool(tmp_path, scn):
    _cli_check(CLI, scn, tmp_path, "product")


@pytest.mark.parametrize("scn", refcorpus.CLI_SCENARIOS, ids=lambda s: s["id"])
def test_stock_main_equals_reference_tool(tmp_path, scn):
    """upstream mini_thumbnailer/src/main.cpp unchanged on the product's library (oracle/_ref/mini_thumbnailer_stock)"""
    if not os.path.exists(STOCK_CLI):
        pytest.skip("oracle/_ref/mini_thumbnailer_stock not built (needs an upstream checkout at build time)")
    _cli_check(STOCK_CLI, scn, tmp_path, "stock")
