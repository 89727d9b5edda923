"""The drop-in boundary (config 0 plumbing): the reference's own mini_thumbnailer/src/main.cpp, compiled and linked
unchanged against include/minivideo.h + libminivideo.so by build() (oracle/Makefile, binary in oracle/_ref/; compiled here if
build() did not find the upstream sources and they can be found now), runs; and the
public enums of include/minivideo.h carry the reference's values (tests/golden/reference_enums.json)."""
import json
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
STOCK = os.path.join(ROOT, "oracle", "_ref", "mini_thumbnailer_stock")


def _stock_cli(tmp_path):
    """the binary build() made; else, where the upstream sources can be read now, the same compile into tmp_path"""
    if os.path.exists(STOCK):
        return STOCK
    from minivideo_amd import build
    ref = build.reference_dir()
    if ref is None:
        pytest.skip("oracle/_ref/mini_thumbnailer_stock not built and no upstream MiniVideo checkout found "
                    "($MINIVIDEO_REFERENCE, BASELINE.json reference_path, reference/ beside the repository or in ~)")
    exe = tmp_path / "mini_thumbnailer_stock"
    main = os.path.join(ref, build.STOCK_MAIN)
    pkg = os.path.join(ROOT, "minivideo_amd")
    subprocess.check_call(["g++", "-O1", "-I" + os.path.join(ROOT, "include"), "-I" + os.path.dirname(main), main,
                           "-L" + pkg, "-lminivideo", "-Wl,-rpath," + pkg, "-o", str(exe)])
    return exe


def test_stock_mini_thumbnailer_builds_and_runs(tmp_path):
    exe = _stock_cli(tmp_path)
    kat = os.path.join(ROOT, "tests", "golden", "kat_cavlc_2mb.264")
    r = subprocess.run([str(exe), "-i", kat, "-f", "yuv420"], cwd=tmp_path, capture_output=True, text=True, timeout=60)
    assert r.returncode == 0                     # exit status reflects minivideo_close (main.cpp:285-298)
    assert "Working..." in r.stdout
    import ctypes as C
    from minivideo_amd import lib
    if lib().mvhp_device_count() == 0:
        # no GPU here: decode must refuse loudly (no CPU reconstruction path), and write nothing
        assert "no HIP device" in r.stderr
        assert not (tmp_path / "kat_cavlc_2mb.yuv").exists()


def _enums(path):
    """{enum name: {constant: value}} of a C header, read as text (implicit values count up from the previous one)"""
    import re
    text = re.sub(r"/\*.*?\*/", "", open(path, errors="replace").read(), flags=re.S)
    text = re.sub(r"//[^\n]*", "", text)
    out = {}
    for m in re.finditer(r"typedef\s+enum\s+(\w+)?\s*\{(.*?)\}\s*(\w+)\s*;", text, flags=re.S):
        vals, nxt = {}, 0
        for item in m.group(2).split(","):
            item = item.strip()
            if not item:
                continue
            name, _, val = (s.strip() for s in item.partition("="))
            nxt = int(val, 0) if val else nxt
            vals[name] = nxt
            nxt += 1
        out[m.group(3)] = vals
    return out


REF_ENUMS = os.path.join(ROOT, "tests", "golden", "reference_enums.json")


def test_public_enums_have_the_reference_values(tmp_path):
    """every enum constant include/minivideo.h declares exists in the reference's public headers with the same value
    (minivideo.h:42-52 error codes, avcodecs.h picture / container / codec enums, avutils.h:143-149 extraction modes, ...);
    the three enums a thumbnailer passes or could receive are complete.  The values are asserted by the COMPILER on our header
    (static_assert in a translation unit).  The reference's were read from its public headers as text (they cannot be compiled
    on their own: they include a CMake-generated file) and are stored, complete for every enum our header declares, in
    tests/golden/reference_enums.json."""
    ref = json.load(open(REF_ENUMS))
    ours = _enums(os.path.join(ROOT, "include", "minivideo.h"))
    assert {"MiniVideoErrorCodes_e", "PictureFormat_e", "PictureRepartition_e"} <= set(ours)
    lines = ['#include "minivideo.h"']
    for enum, vals in ours.items():
        assert enum in ref, enum
        for name, _ in vals.items():
            assert name in ref[enum], (enum, name)
            lines.append(f'static_assert({name} == {ref[enum][name]}, "{enum}::{name}");')
    for enum in ("MiniVideoErrorCodes_e", "PictureFormat_e", "PictureRepartition_e"):
        assert set(ours[enum]) == set(ref[enum]), (enum, set(ours[enum]) ^ set(ref[enum]))
    assert ref["MiniVideoErrorCodes_e"] == {"ERROR_UNKNOWN": 1, "ERROR_CONTAINER_UNKNOWN": 10, "ERROR_CONTAINER_FAILURE": 11,
                                            "ERROR_CODEC_UNKNOWN": 20, "ERROR_CODEC_FAILURE": 21}
    lines.append("int main() { return 0; }")
    src = tmp_path / "enums.cpp"
    src.write_text("\n".join(lines) + "\n")
    subprocess.check_call(["g++", "-std=c++17", "-fsyntax-only", "-I" + os.path.join(ROOT, "include"), str(src)])
