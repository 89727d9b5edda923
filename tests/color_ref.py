"""NumPy / Python-integer restatement of the display rules (DESIGN.md 3 "Display aspect and colour"; color_convert.hip,
resample_taps.h, stream_abi.cpp): the colour coefficients from exact rationals, chroma in sixteenths by siting, the colour
equation, the resolve rule that maps a stream's VUI to parameters, and the aspect rule.  Written from the text of the header,
not from the library: the coefficients are derived here with `fractions`, nothing is copied.  The vectorised chroma blend is
checked against a plain per-sample loop in tests/test_color.py."""
from fractions import Fraction

import numpy as np

BT601, BT709 = 0, 1
NEAREST, LEFT, CENTER = 0, 1, 2
MODES = ("auto", "bt601", "bt709", "bt601-full", "bt709-full")
KR_KB = {BT601: (Fraction(299, 1000), Fraction(114, 1000)), BT709: (Fraction(2126, 10000), Fraction(722, 10000))}
# Table E-1: aspect_ratio_idc -> sample aspect ratio
SAR_TABLE = {1: (1, 1), 2: (12, 11), 3: (10, 11), 4: (16, 11), 5: (40, 33), 6: (24, 11), 7: (20, 11), 8: (32, 11), 9: (80, 33),
             10: (18, 11), 11: (15, 11), 12: (64, 33), 13: (160, 99), 14: (4, 3), 15: (3, 2), 16: (2, 1)}


def exact(matrix, full_range):
    """the exact rationals (ly, crv, cbu, gcb, gcr) of R = ly (Y - yoff) + crv (Cr - 128) etc., and yoff"""
    kr, kb = KR_KB[matrix]
    kg = 1 - kr - kb
    ls = Fraction(1) if full_range else Fraction(255, 219)
    cs = Fraction(1) if full_range else Fraction(255, 224)
    return (ls, 2 * (1 - kr) * cs, 2 * (1 - kb) * cs, 2 * kb * (1 - kb) / kg * cs, 2 * kr * (1 - kr) / kg * cs), (0 if full_range else 16)


def coefficients(matrix, full_range):
    """(cy, crv, cbu, gcb, gcr, yoff): round(2^14 x), halves up"""
    x, yoff = exact(matrix, full_range)
    return tuple(int((v * (1 << 14) + Fraction(1, 2)).__floor__()) for v in x) + (yoff,)


def sar(idc, ext=(0, 0)):
    """the sample aspect ratio an aspect_ratio_idc means, reduced; (0, 0) = unspecified"""
    w, h = ext if idc == 255 else SAR_TABLE.get(idc, (0, 0))
    if w == 0 or h == 0:
        return 0, 0
    f = Fraction(w, h)
    return f.numerator, f.denominator


def aspect(cw, ch, a, b):
    """the aspect rule: cw x ch with samples a : b as wide as high (0 in either: 1 : 1) -> (ow, oh)"""
    if a == 0 or b == 0 or a == b:
        return cw, ch
    if a > b:
        return cw, max(2, 2 * ((ch * b + a) // (2 * a)))
    return max(2, 2 * ((cw * a + b) // (2 * b))), ch


def resolve(display, coded_w, coded_h, mode):
    """(matrix, full_range, siting) for a stream that says `display` (a dict with signal_present, full_range,
    matrix_coefficients, chroma_loc; None = nothing) under mode 0 .. 4 or one of MODES"""
    if isinstance(mode, str):
        mode = MODES.index(mode)
    d = display or {"signal_present": 0, "full_range": 0, "matrix_coefficients": 2, "chroma_loc": 0}
    if mode == 0:
        mc = d["matrix_coefficients"]
        if mc == 1:
            matrix = BT709
        elif mc in (5, 6):
            matrix = BT601
        else:
            matrix = BT709 if (coded_w >= 1280 or coded_h > 576) else BT601
        full = 1 if (d["signal_present"] and d["full_range"]) else 0
    else:
        matrix = BT709 if mode in (2, 4) else BT601
        full = 1 if mode >= 3 else 0
    return matrix, full, (CENTER if d["chroma_loc"] & 1 else LEFT)


def chroma16(C, siting):
    """chroma planes (n, ch, cw) -> the chroma of every luma sample in sixteenths, (n, 2 ch, 2 cw) int64"""
    C = np.asarray(C).astype(np.int64)
    n, ch, cw = C.shape
    if siting == NEAREST:
        return 16 * C.repeat(2, 1).repeat(2, 2)
    up = np.concatenate([C[:, :1], C[:, :-1]], 1)          # row j - 1, clamped
    down = np.concatenate([C[:, 1:], C[:, -1:]], 1)        # row j + 1
    V = np.empty((n, 2 * ch, cw), np.int64)
    V[:, 0::2] = up + 3 * C
    V[:, 1::2] = 3 * C + down
    left = np.concatenate([V[:, :, :1], V[:, :, :-1]], 2)  # column k - 1
    right = np.concatenate([V[:, :, 1:], V[:, :, -1:]], 2)
    out = np.empty((n, 2 * ch, 2 * cw), np.int64)
    if siting == LEFT:
        out[:, :, 0::2] = 4 * V
        out[:, :, 1::2] = 2 * V + 2 * right
    else:
        out[:, :, 0::2] = left + 3 * V
        out[:, :, 1::2] = 3 * V + right
    return out


def chroma16_loop(C, siting, x, y):
    """one sample of chroma16 for one plane (ch, cw), as the header words it"""
    ch, cw = C.shape
    j, k = y >> 1, x >> 1
    if siting == NEAREST:
        return 16 * int(C[j, k])
    rows = ((j - 1, 1), (j, 3)) if y % 2 == 0 else ((j, 3), (j + 1, 1))
    if siting == LEFT:
        cols = ((k, 4),) if x % 2 == 0 else ((k, 2), (k + 1, 2))
    else:
        cols = ((k - 1, 1), (k, 3)) if x % 2 == 0 else ((k, 3), (k + 1, 1))
    return sum(wy * wx * int(C[min(max(r, 0), ch - 1), min(max(c, 0), cw - 1)]) for r, wy in rows for c, wx in cols)


def equation(Y, cb16, cr16, matrix, full_range):
    """int64 arrays (same shape): luma and chroma in sixteenths -> (R, G, B) uint8"""
    cy, crv, cbu, gcb, gcr, yoff = coefficients(matrix, full_range)
    yp = 16 * cy * (np.asarray(Y).astype(np.int64) - yoff)
    cb, cr = np.asarray(cb16).astype(np.int64) - 2048, np.asarray(cr16).astype(np.int64) - 2048
    half = 1 << 17
    r = (yp + crv * cr + half) >> 18
    g = (yp - gcb * cb - gcr * cr + half) >> 18
    b = (yp + cbu * cb + half) >> 18
    return tuple(np.clip(v, 0, 255).astype(np.uint8) for v in (r, g, b))


def to_rgb(planes, w, h, matrix, full_range, siting):
    """dense planar pictures (n x w*h*3/2) -> RGB8 (n x w*h*3)"""
    planes = np.ascontiguousarray(planes, np.uint8).reshape(-1, w * h * 3 // 2)
    n, q = planes.shape[0], (w // 2) * (h // 2)
    Y = planes[:, :w * h].reshape(n, h, w)
    Cb = planes[:, w * h:w * h + q].reshape(n, h // 2, w // 2)
    Cr = planes[:, w * h + q:].reshape(n, h // 2, w // 2)
    r, g, b = equation(Y, chroma16(Cb, siting), chroma16(Cr, siting), matrix, full_range)
    return np.stack([r, g, b], -1).reshape(n, -1)


def float_rgb(Y, Cb, Cr, matrix, full_range):
    """the float64 equations of the same matrix and range, unrounded and unclamped: (R, G, B)"""
    (ly, crv, cbu, gcb, gcr), yoff = exact(matrix, full_range)
    y = float(ly) * (np.asarray(Y, np.float64) - yoff)
    cb, cr = np.asarray(Cb, np.float64) - 128.0, np.asarray(Cr, np.float64) - 128.0
    return y + float(crv) * cr, y - float(gcb) * cb - float(gcr) * cr, y + float(cbu) * cb
