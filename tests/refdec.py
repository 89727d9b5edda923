"""The reference decoder as a test oracle: runs upstream MiniVideo's own mini_thumbnailer (built statically from an upstream
checkout by oracle/Makefile, target _ref/mini_thumbnailer_ref) and reads the files it writes.

The tool ignores -o and writes <basename>[_k].<ext> into its working directory (export.c:627-708), so every run gets a
fresh temporary directory.  Readers for the formats it writes: yuv420 / yuv444 (raw planes), BMP (bottom-up BGR rows padded to
four bytes), TGA (stb_image_write's RLE, bottom-up BGR) and PNG (pixels only: zlib + the five row filters)."""
import os
import struct
import subprocess
import tempfile
import zlib

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
REF_CLI = os.path.join(ROOT, "oracle", "_ref", "mini_thumbnailer_ref")
HOW_TO_BUILD = ("reference decoder oracle/_ref/mini_thumbnailer_ref missing: build it from an upstream MiniVideo checkout "
                "with __graft_entry__.build() (MINIVIDEO_REFERENCE=<checkout>) or "
                "make -C oracle REFERENCE=<checkout> _ref/mini_thumbnailer_ref")


def available():
    return os.access(REF_CLI, os.X_OK)


def require():
    """skips the calling test where the reference binary was not built (no upstream checkout)"""
    if not available():
        pytest.skip(HOW_TO_BUILD)
    return REF_CLI


def run_cli(exe, data, name, fmt=None, n=None, mode=None, timeout=300, cwd=None):
    """Runs a mini_thumbnailer-compatible binary on `data` (bytes or uint8 array) saved as `name` in a working directory of
    its own (`cwd`, else a fresh temporary one).  Returns (CompletedProcess, {file name: bytes}) of every file it wrote
    there besides the input."""
    args = []
    if fmt is not None:
        args += ["-f", fmt]
    if n is not None:
        args += ["-n", str(n)]
    if mode is not None:
        args += ["-e", mode]
    data = data.tobytes() if isinstance(data, np.ndarray) else bytes(data)

    def go(d):
        path = os.path.join(d, name)
        with open(path, "wb") as f:
            f.write(data)
        r = subprocess.run([exe, "-i", path] + args, cwd=d, capture_output=True, timeout=timeout)
        files = {}
        for fn in sorted(os.listdir(d)):
            if fn != name:
                with open(os.path.join(d, fn), "rb") as f:
                    files[fn] = f.read()
        return r, files

    if cwd is not None:
        os.makedirs(cwd, exist_ok=True)
        return go(str(cwd))
    with tempfile.TemporaryDirectory(prefix="refdec_") as d:
        return go(d)


def decode(data, fmt, n, name="s.264", mode=None, timeout=300):
    """The reference's files for `data`: {name: bytes}.  A run that fails (exit status, or a file missing) raises: a
    reference that cannot decode a stream of the corpus is a finding, never a skip."""
    r, files = run_cli(require(), data, name, fmt=fmt, n=n, mode=mode, timeout=timeout)
    if r.returncode != 0:
        raise AssertionError("reference decoder exited %d on %s (-f %s -n %s):\n%s" % (
            r.returncode, name, fmt, n, (r.stdout + r.stderr).decode(errors="replace")[-2000:]))
    return files


def picture_names(name, fmt, count):
    """file names the reference gives `count` pictures: <base>.<ext> for one picture, <base>_k.<ext> otherwise
    (export.c:627-708; jpg falls back to png without libjpeg, yuv420 / yuv444 are .yuv)"""
    base = os.path.splitext(name)[0]
    ext = {"yuv420": "yuv", "yuv444": "yuv", "jpg": "png", None: "png"}.get(fmt, fmt)
    if count == 1:
        return [base + "." + ext]
    return ["%s_%d.%s" % (base, k, ext) for k in range(count)]


def pictures(data, fmt, count, name="s.264"):
    """the reference's `count` pictures of `data` in `fmt`, in order, as bytes; fails unless exactly those files appear"""
    files = decode(data, fmt, count, name=name)
    want = picture_names(name, fmt, count)
    assert sorted(files) == sorted(want), "reference wrote %s, expected %s" % (sorted(files), want)
    return [files[k] for k in want]


# ---- readers: each returns (pixels as uint8[h * w * 3] in RGB order, top row first, w, h) ----

def read_bmp(data):
    assert data[:2] == b"BM", "not a BMP"
    off = struct.unpack("<I", data[10:14])[0]
    hsz, w, h, planes, bpp = struct.unpack("<IiiHH", data[14:30])
    comp = struct.unpack("<I", data[30:34])[0]
    assert (planes, bpp, comp) == (1, 24, 0), (planes, bpp, comp)
    stride = (w * 3 + 3) & ~3
    bottom_up = h > 0
    h = abs(h)
    assert len(data) >= off + stride * h, "BMP truncated"
    rows = np.frombuffer(data, np.uint8, stride * h, off).reshape(h, stride)[:, :w * 3].reshape(h, w, 3)
    if bottom_up:
        rows = rows[::-1]
    return np.ascontiguousarray(rows[:, :, ::-1]).reshape(-1), w, h


def read_tga(data):
    idlen, cmap, itype = data[0], data[1], data[2]
    w, h, bpp, desc = struct.unpack("<HHBB", data[12:18])
    assert cmap == 0 and itype in (2, 10) and bpp == 24, (cmap, itype, bpp)
    pos = 18 + idlen
    n = w * h
    out = np.zeros((n, 3), np.uint8)
    if itype == 2:
        out[:] = np.frombuffer(data, np.uint8, n * 3, pos).reshape(n, 3)
    else:
        i = 0
        while i < n:
            c = data[pos]
            pos += 1
            ln = (c & 127) + 1
            assert i + ln <= n, "TGA packet runs past the picture"
            if c & 128:
                out[i:i + ln] = np.frombuffer(data, np.uint8, 3, pos)
                pos += 3
            else:
                out[i:i + ln] = np.frombuffer(data, np.uint8, 3 * ln, pos).reshape(ln, 3)
                pos += 3 * ln
            i += ln
    img = out.reshape(h, w, 3)
    if not desc & 0x20:                       # origin bottom left
        img = img[::-1]
    if desc & 0x10:                           # origin right
        img = img[:, ::-1]
    return np.ascontiguousarray(img[:, :, ::-1]).reshape(-1), w, h


def _paeth(a, b, c):
    p = a + b - c
    pa, pb, pc = abs(p - a), abs(p - b), abs(p - c)
    if pa <= pb and pa <= pc:
        return a
    return b if pb <= pc else c


def read_png(data):
    assert data[:8] == b"\x89PNG\r\n\x1a\n", "not a PNG"
    pos, idat, w, h = 8, b"", 0, 0
    while pos < len(data):
        n, typ = struct.unpack(">I4s", data[pos:pos + 8])
        body = data[pos + 8:pos + 8 + n]
        assert struct.unpack(">I", data[pos + 8 + n:pos + 12 + n])[0] == (zlib.crc32(typ + body) & 0xffffffff), typ
        if typ == b"IHDR":
            w, h, depth, ctype, _, _, interlace = struct.unpack(">IIBBBBB", body[:13])
            assert (depth, ctype, interlace) == (8, 2, 0), (depth, ctype, interlace)
        elif typ == b"IDAT":
            idat += body
        elif typ == b"IEND":
            break
        pos += 12 + n
    stride = w * 3
    raw = np.frombuffer(zlib.decompress(idat), np.uint8).reshape(h, stride + 1)
    out = np.zeros((h, stride), np.uint8)
    prev = np.zeros(stride, np.int32)
    for y in range(h):
        ft = raw[y, 0]
        line = raw[y, 1:].astype(np.int32)
        if ft == 0:
            cur = line
        elif ft == 2:
            cur = (line + prev) & 255
        elif ft == 1:                         # left neighbour: a running sum per channel
            cur = (np.cumsum(line.reshape(w, 3), axis=0) & 255).reshape(-1)
        elif ft in (3, 4):                    # left and upper neighbours: byte by byte (small pictures only)
            cur = np.zeros(stride, np.int32)
            for x in range(stride):
                a = cur[x - 3] if x >= 3 else 0
                b = prev[x]
                c = prev[x - 3] if x >= 3 else 0
                pred = (a + b) >> 1 if ft == 3 else _paeth(a, b, c)
                cur[x] = (line[x] + pred) & 255
        else:
            raise AssertionError("PNG filter type %d" % ft)
        out[y] = cur
        prev = cur
    return out.reshape(-1), w, h


def read_rgb(fmt, data):
    """pixels of a picture file in any of the reference's RGB formats"""
    if fmt == "bmp":
        return read_bmp(data)
    if fmt == "tga":
        return read_tga(data)
    return read_png(data)
