"""Helpers of the orientation tests: MP4 files with a display matrix.  tests/mp4mux.py writes the identity; these patch the nine
32-bit matrix words behind b"tkhd" in its output (version 0: 40 bytes behind the box body)."""
import ctypes as C
import struct

import numpy as np

from minivideo_amd.hotpath import lib
from tests.mp4mux import mux

ONE, NEG, W1 = 0x00010000, 0xFFFF0000, 0x40000000
# {a, b, u; c, d, v; x, y, w} of the four rotations, by clockwise quarter turns
ROTATIONS = {
    0: (ONE, 0, 0, 0, ONE, 0, 0, 0, W1),
    1: (0, ONE, 0, NEG, 0, 0, 0, 0, W1),
    2: (NEG, 0, 0, 0, NEG, 0, 0, 0, W1),
    3: (0, NEG, 0, ONE, 0, 0, 0, 0, W1),
}


def patch_matrix(mp4, words):
    """the file with the nine matrix words of its (version 0) tkhd box replaced"""
    b = bytearray(mp4)
    at = b.find(b"tkhd") + 4 + 40
    assert at >= 44 and b[at - 40] == 0, "a version 0 tkhd box"
    b[at:at + 36] = struct.pack(">9I", *[w & 0xFFFFFFFF for w in words])
    return bytes(b)


def tkhd_version1(mp4):
    """the same file with a version 1 tkhd box (64-bit times and duration: the matrix lies 52 bytes behind the box body); the
    boxes that contain it grow by 12 bytes.  For files with mdat in front of moov: no chunk offset moves"""
    b = bytes(mp4)
    at = b.find(b"tkhd") - 4
    size = struct.unpack(">I", b[at:at + 4])[0]
    body = b[at + 8:at + size]
    assert body[0] == 0 and b.find(b"mdat") < b.find(b"moov")
    flags = body[1:4]
    creation, modification, track, reserved, duration = struct.unpack(">IIIII", body[4:24])
    v1 = bytes([1]) + flags + struct.pack(">QQIIQ", creation, modification, track, reserved, duration) + body[24:]
    out = bytearray(b[:at] + struct.pack(">I", 8 + len(v1)) + b"tkhd" + v1 + b[at + size:])
    for name in (b"moov", b"trak"):
        p = out.find(name) - 4
        out[p:p + 4] = struct.pack(">I", struct.unpack(">I", out[p:p + 4])[0] + 12)
    return bytes(out)


def patch_matrix_v1(mp4, words):
    b = bytearray(mp4)
    at = b.find(b"tkhd") + 4 + 52
    assert b[at - 52] == 1, "a version 1 tkhd box"
    b[at:at + 36] = struct.pack(">9I", *[w & 0xFFFFFFFF for w in words])
    return bytes(b)


def truncate_tkhd(mp4, keep=20):
    """the tkhd box (version 0) cut `keep` bytes into its matrix; what is left of it becomes a `free` box, so the walk goes on"""
    b = bytearray(mp4)
    at = b.find(b"tkhd") - 4
    size = struct.unpack(">I", b[at:at + 4])[0]
    new = 8 + 40 + keep
    assert size - new >= 8
    b[at:at + 4] = struct.pack(">I", new)
    b[at + new:at + new + 8] = struct.pack(">I4s", size - new, b"free")
    return bytes(b)


def rotated_mp4(annexb, width, height, turns, **kw):
    return patch_matrix(mux(annexb, width, height, **kw), ROTATIONS[turns])


class Mp4Stream:
    """mvhp_stream_open_mp4 over bytes (kept alive with the handle)"""

    def __init__(self, data):
        self.L = L = lib()
        L.mvhp_stream_open_mp4.restype = C.c_int
        L.mvhp_stream_open_mp4.argtypes = [C.c_void_p, C.c_size_t, C.POINTER(C.c_void_p)]
        self.data = np.frombuffer(bytes(data), np.uint8).copy()
        self.h = C.c_void_p()
        self.ok = L.mvhp_stream_open_mp4(self.data.ctypes.data, self.data.size, C.byref(self.h)) == 1

    def __enter__(self):
        return self

    def __exit__(self, *a):
        if self.h:
            self.L.mvhp_stream_close(self.h)
            self.h = None
