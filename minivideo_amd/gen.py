"""ctypes binding of libmvgen.so, the synthetic H.264 IDR stream generator.

TEST / BENCH INFRASTRUCTURE: produces legal Annex-B streams of random syntax
elements plus the packed records a correct front end must derive from them."""
import ctypes as C
import os

import numpy as np

_HERE = os.path.dirname(os.path.abspath(__file__))
_LIB = None


class GenCfg(C.Structure):
    _fields_ = [
        ("width_mbs", C.c_int32), ("height_mbs", C.c_int32), ("n_frames", C.c_int32),
        ("seed", C.c_uint64),
        ("profile_idc", C.c_int32), ("cabac", C.c_int32), ("transform8x8", C.c_int32), ("dense", C.c_int32),
        ("cqp_offset_cb", C.c_int32), ("cqp_offset_cr", C.c_int32),
        ("sps_pps_every_frame", C.c_int32), ("allow_qp36_i16", C.c_int32),
        ("qp_min", C.c_int32), ("qp_max", C.c_int32), ("max_level", C.c_int32),
    ]


def lib():
    global _LIB
    if _LIB is None:
        path = os.path.join(_HERE, "libmvgen.so")
        if not os.path.exists(path):
            raise RuntimeError(f"{path} missing: run __graft_entry__.build()")
        L = C.CDLL(path)
        L.mvgen_stream.restype = C.c_size_t
        L.mvgen_stream.argtypes = [C.POINTER(GenCfg), C.c_void_p, C.c_size_t, C.c_void_p]
        L.mvgen_stream_ex.restype = C.c_size_t
        L.mvgen_stream_ex.argtypes = [C.POINTER(GenCfg), C.c_int32, C.c_int32, C.c_int32, C.c_void_p, C.c_size_t, C.c_void_p,
                                      C.c_void_p]
        L.mvgen_stream_dbk.restype = C.c_size_t
        L.mvgen_stream_dbk.argtypes = [C.POINTER(GenCfg), C.c_int32, C.c_int32, C.c_int32, C.c_int32, C.c_int32, C.c_int32,
                                       C.c_void_p, C.c_size_t, C.c_void_p, C.c_void_p]
        L.mvgen_stream_crop.restype = C.c_size_t
        L.mvgen_stream_crop.argtypes = [C.POINTER(GenCfg), C.c_int32, C.c_void_p, C.c_void_p, C.c_size_t, C.c_void_p]
        L.mvgen_stream_vui.restype = C.c_size_t
        L.mvgen_stream_vui.argtypes = [C.POINTER(GenCfg), C.c_int32, C.c_void_p, C.c_int32, C.c_int32, C.c_void_p, C.c_void_p,
                                       C.c_size_t, C.c_void_p]
        _LIB = L
    return _LIB


def make_stream_crop(width_mbs, height_mbs, n_frames, crops, seed=1, profile="baseline", dense=True, cqp_offsets=(0, 0),
                     sps_pps_every_frame=False, qp_range=(24, 32), max_level=32, allow_qp36_i16=False):
    """make_stream with SPS frame cropping: `crops` is a list of (left, right, top, bottom) offsets; SPS k of the stream (one
    per picture with sps_pps_every_frame) carries crops[k % len(crops)].  The macroblocks are those of make_stream with the same
    arguments.  Returns (stream, packed[n, W*H, 800])."""
    prof = {"baseline": (66, 0, 0), "main": (77, 1, 0), "main_cavlc": (77, 0, 0), "high": (100, 1, 1),
            "high_cavlc": (100, 0, 1), "high_4x4": (100, 1, 0)}[profile]
    cfg = GenCfg(width_mbs, height_mbs, n_frames, seed, prof[0], prof[1], prof[2], 1 if dense else 0,
                 cqp_offsets[0], cqp_offsets[1], int(sps_pps_every_frame), int(allow_qp36_i16),
                 qp_range[0], qp_range[1], max_level)
    L = lib()
    cr = np.ascontiguousarray(np.array(crops, np.int32).reshape(-1, 4))
    packed = np.zeros((n_frames, width_mbs * height_mbs, 800), np.uint8)
    n = L.mvgen_stream_crop(C.byref(cfg), cr.shape[0], cr.ctypes.data, None, 0, packed.ctypes.data)
    if n == 0:
        raise ValueError("generator rejected the configuration")
    out = np.zeros(n, np.uint8)
    assert L.mvgen_stream_crop(C.byref(cfg), cr.shape[0], cr.ctypes.data, out.ctypes.data, n, packed.ctypes.data) == n
    return out, packed


def vui_record(sar=None, overscan=None, full_range=None, matrix=None, chroma_loc=None, timing=False, video_format=5,
               primaries=2, transfer=2):
    """One VUI record for make_stream_vui.  sar: None (no aspect_ratio_info), an aspect_ratio_idc, or (w, h) = idc 255 with that
    extended pair; overscan: None or the overscan_appropriate_flag; full_range / matrix: None leaves the syntax out (a matrix
    alone writes video_signal_type with video_full_range_flag 0); chroma_loc: None, a type for both fields or (top, bottom);
    timing: a timing_info tail behind the fields the front end reads."""
    r = [0] * 16
    if sar is not None:
        r[0] = 1
        if isinstance(sar, tuple):
            r[1], r[2], r[3] = 255, int(sar[0]), int(sar[1])
        else:
            r[1] = int(sar)
    if overscan is not None:
        r[4] = 2 if overscan else 1
    if full_range is not None or matrix is not None:
        r[5], r[6], r[7] = 1, int(video_format), int(bool(full_range))
        if matrix is not None:
            r[8], r[9], r[10], r[11] = 1, int(primaries), int(transfer), int(matrix)
    if chroma_loc is not None:
        top, bottom = chroma_loc if isinstance(chroma_loc, tuple) else (chroma_loc, chroma_loc)
        r[12], r[13], r[14] = 1, int(top), int(bottom)
    r[15] = int(bool(timing))
    return r


def make_stream_vui(width_mbs, height_mbs, n_frames, vuis, keep_bits=-1, crops=None, seed=1, profile="baseline", dense=True,
                    cqp_offsets=(0, 0), sps_pps_every_frame=False, qp_range=(24, 32), max_level=32, allow_qp36_i16=False):
    """make_stream with a VUI in every SPS: `vuis` is a list of vui_record()s; SPS k of the stream (one per picture with
    sps_pps_every_frame) carries vuis[k % len(vuis)] and, with `crops` (as make_stream_crop), crops[k % len(crops)].
    keep_bits >= 0 cuts every SPS off after that many bits of its VUI.  The macroblocks are those of make_stream with the same
    arguments.  Returns (stream, packed[n, W*H, 800])."""
    prof = {"baseline": (66, 0, 0), "main": (77, 1, 0), "main_cavlc": (77, 0, 0), "high": (100, 1, 1),
            "high_cavlc": (100, 0, 1), "high_4x4": (100, 1, 0)}[profile]
    cfg = GenCfg(width_mbs, height_mbs, n_frames, seed, prof[0], prof[1], prof[2], 1 if dense else 0,
                 cqp_offsets[0], cqp_offsets[1], int(sps_pps_every_frame), int(allow_qp36_i16),
                 qp_range[0], qp_range[1], max_level)
    L = lib()
    vr = np.ascontiguousarray(np.array(vuis, np.int32).reshape(-1, 16))
    cr = np.ascontiguousarray(np.array(crops if crops else [], np.int32).reshape(-1, 4))
    packed = np.zeros((n_frames, width_mbs * height_mbs, 800), np.uint8)

    def call(out, cap):
        return L.mvgen_stream_vui(C.byref(cfg), vr.shape[0], vr.ctypes.data, int(keep_bits), cr.shape[0],
                                  cr.ctypes.data if cr.shape[0] else None, out, cap, packed.ctypes.data)
    n = call(None, 0)
    if n == 0:
        raise ValueError("generator rejected the configuration")
    out = np.zeros(n, np.uint8)
    assert call(out.ctypes.data, n) == n
    return out, packed


def make_stream(width_mbs, height_mbs, n_frames, seed=1, profile="baseline", dense=True, cqp_offsets=(0, 0),
                sps_pps_every_frame=False, qp_range=(24, 32), max_level=32, allow_qp36_i16=False, want_packed=True):
    """profile: 'baseline' (66, CAVLC), 'main' (77, CABAC), 'high' (100, CABAC, 8x8),
    'high_cavlc' (100, CAVLC, 8x8).  Returns (stream bytes as uint8 array, packed[n, W*H, 800] or None)."""
    prof = {"baseline": (66, 0, 0), "main": (77, 1, 0), "main_cavlc": (77, 0, 0), "high": (100, 1, 1),
            "high_cavlc": (100, 0, 1), "high_4x4": (100, 1, 0)}[profile]
    cfg = GenCfg(width_mbs, height_mbs, n_frames, seed, prof[0], prof[1], prof[2], 1 if dense else 0,
                 cqp_offsets[0], cqp_offsets[1], int(sps_pps_every_frame), int(allow_qp36_i16),
                 qp_range[0], qp_range[1], max_level)
    L = lib()
    packed = np.zeros((n_frames, width_mbs * height_mbs, 800), np.uint8) if want_packed else None
    n = L.mvgen_stream(C.byref(cfg), None, 0, packed.ctypes.data if want_packed else None)
    if n == 0:
        raise ValueError("generator rejected the configuration")
    out = np.zeros(n, np.uint8)
    n2 = L.mvgen_stream(C.byref(cfg), out.ctypes.data, n, packed.ctypes.data if want_packed else None)
    assert n2 == n
    return out, packed


def make_stream_ex(width_mbs, height_mbs, n_frames, seed=1, profile="baseline", slices=1, pcm_permille=0, scaling=0, dense=True,
                   cqp_offsets=(0, 0), sps_pps_every_frame=False, qp_range=(24, 32), max_level=32, allow_qp36_i16=True, deblock=None):
    """Streams OUTSIDE the reference's envelope (what MVHP_STREAM_SPEC decodes by the standard): `slices` slices
    per picture, pcm_permille / 1000 of the macroblocks I_PCM, scaling lists in the SPS (scaling & 1) and / or the PPS (scaling & 2;
    'high*' profiles only).  Returns (stream, packed[n, W*H, 800], weights[112] = scaling4[3][16] | scaling8[64] in raster order).

    deblock: None (no deblocking syntax: the PPS leaves deblocking_filter_control_present_flag 0, the stream is byte-identical to
    the one without the argument) or e.g. dict(idc=(0, 1, 2), offsets=(-6, 6)): every slice draws disable_deblocking_filter_idc
    from `idc` and both offsets (div2) from the closed range `offsets`; the records carry them (mvhp_mb_header_t::flags bits 1-2,
    dbk_offsets).  The macroblocks are those of the same call without `deblock`."""
    prof = {"baseline": (66, 0, 0), "main": (77, 1, 0), "main_cavlc": (77, 0, 0), "high": (100, 1, 1),
            "high_cavlc": (100, 0, 1), "high_4x4": (100, 1, 0)}[profile]
    cfg = GenCfg(width_mbs, height_mbs, n_frames, seed, prof[0], prof[1], prof[2], 1 if dense else 0,
                 cqp_offsets[0], cqp_offsets[1], int(sps_pps_every_frame), int(allow_qp36_i16),
                 qp_range[0], qp_range[1], max_level)
    L = lib()
    packed = np.zeros((n_frames, width_mbs * height_mbs, 800), np.uint8)
    weights = np.zeros(112, np.uint8)
    if deblock is None:
        def call(out, cap):
            return L.mvgen_stream_ex(C.byref(cfg), slices, pcm_permille, scaling, out, cap, packed.ctypes.data, weights.ctypes.data)
    else:
        mask = sum(1 << int(k) for k in deblock.get("idc", (0,)))
        lo, hi = deblock.get("offsets", (0, 0))

        def call(out, cap):
            return L.mvgen_stream_dbk(C.byref(cfg), slices, pcm_permille, scaling, mask, lo, hi, out, cap, packed.ctypes.data,
                                      weights.ctypes.data)
    n = call(None, 0)
    if n == 0:
        raise ValueError("generator rejected the configuration")
    out = np.zeros(n, np.uint8)
    n2 = call(out.ctypes.data, n)
    assert n2 == n
    return out, packed, weights
