"""NumPy restatement of the tensor output (csrc/hip/tensor_pack.hip, mvhp_tensor_dev; include/minivideo_hotpath.h "Tensor output").

The arithmetic is one binary32 fused multiply-add per sample, so there are only 256 x 3 different values: value_table() makes them
EXACTLY -- c * scale + bias as a fractions.Fraction, then the nearest binary32 chosen by exact comparison of a candidate and its
two neighbours, ties to even -- never through float64 arithmetic followed by astype(float32), which can round twice.  float16 is
NumPy's own round-to-nearest-even conversion (subnormals kept, overflow to infinity); bfloat16 is rounded in integers on the bit
pattern.  Placement, layouts and the B,G,R order are plain indexing."""
from fractions import Fraction

import numpy as np

F32, F16, BF16 = 0, 1, 2
NCHW, NHWC = 0, 1
ELEMENT_BYTES = {F32: 4, F16: 2, BF16: 2}

_MAX = Fraction(2) ** 128 - Fraction(2) ** 104   # the largest binary32
_OVER = Fraction(2) ** 128 - Fraction(2) ** 103  # half an ulp above it: from here on (ties to even) the result is infinity


def _bits(f):
    return int(np.float32(f).view(np.uint32))


def round_to_f32(x, zero_negative=False):
    """the binary32 nearest to the Fraction x, ties to even; an exact 0 gets the sign zero_negative says"""
    if x == 0:
        return np.float32(-0.0 if zero_negative else 0.0)
    if abs(x) >= _OVER:
        return np.float32(-np.inf if x < 0 else np.inf)
    with np.errstate(over="ignore", under="ignore"):
        cand = np.float32(float(max(min(x, _MAX), -_MAX)))
    best = None
    for c in (np.nextafter(cand, np.float32(-np.inf)), cand, np.nextafter(cand, np.float32(np.inf))):
        if not np.isfinite(c):
            continue
        d = abs(Fraction(float(c)) - x)
        even = (_bits(c) & 1) == 0
        if best is None or d < best[0] or (d == best[0] and even and not best[1]):
            best = (d, even, c)
    c = best[2]
    if c == 0:   # a value that rounds to zero keeps its own sign
        return np.float32(-0.0 if x < 0 else 0.0)
    return np.float32(c)


def fma_f32(c, scale, bias):
    """fmaf((float)c, scale, bias) for a sample c and two binary32 numbers, exactly"""
    scale, bias = np.float32(scale), np.float32(bias)
    assert np.isfinite(scale) and np.isfinite(bias)
    x = Fraction(int(c)) * Fraction(float(scale)) + Fraction(float(bias))
    # an exact zero: the sum of two zeros of one sign keeps it; everything else (opposite zeros, exact cancellation) is +0
    product_zero = c == 0 or scale == 0
    product_negative = bool(np.signbit(scale))   # ((float)c is +0 or positive)
    neg = product_zero and bias == 0 and product_negative and bool(np.signbit(bias))
    return round_to_f32(x, neg)


def value_table(scale, bias):
    """float32 [256, 3]: the value of every sample of every colour"""
    t = np.empty((256, 3), np.float32)
    for k in range(3):
        for c in range(256):
            t[c, k] = fma_f32(c, scale[k], bias[k])
    return t


def to_bf16_bits(a):
    """float32 array -> uint16 array of bfloat16 bit patterns, round to nearest even in integers"""
    u = np.ascontiguousarray(a, np.float32).view(np.uint32).astype(np.uint64)
    return ((u + 0x7fff + ((u >> 16) & 1)) >> 16).astype(np.uint16)


def convert(a, dtype):
    """float32 array -> the array of the element type (bfloat16 as uint16 bit patterns)"""
    a = np.ascontiguousarray(a, np.float32)
    if dtype == F32:
        return a
    if dtype == F16:
        with np.errstate(over="ignore", under="ignore"):
            return a.astype(np.float16)
    return to_bf16_bits(a)


def tensor_bytes(src_w, src_h, canvas, dtype):
    cw, ch = canvas if canvas else (src_w, src_h)
    return 3 * cw * ch * ELEMENT_BYTES[dtype]


def pack(rgb, canvas=None, dtype=F32, layout=NCHW, bgr=False, pad=(0, 0, 0), scale=(1, 1, 1), bias=(0, 0, 0), table=None):
    """rgb: uint8 [n, h, w, 3] -> uint8 [n, tensor_bytes]: the raw bytes of the n tensors.  table: value_table(scale, bias), when
    the caller has it already"""
    rgb = np.asarray(rgb, np.uint8)
    n, h, w, _ = rgb.shape
    cw, ch = canvas if canvas else (w, h)
    assert cw >= w and ch >= h
    tab = value_table(scale, bias) if table is None else table
    out = np.empty((n, ch, cw, 3), np.float32)
    ox, oy = (cw - w) // 2, (ch - h) // 2
    for k in range(3):
        out[..., k] = tab[pad[k], k]
        out[:, oy:oy + h, ox:ox + w, k] = tab[rgb[..., k], k]
    if bgr:
        out = out[..., ::-1]
    if layout == NCHW:
        out = out.transpose(0, 3, 1, 2)
    return np.ascontiguousarray(convert(out, dtype)).view(np.uint8).reshape(n, -1)


IMAGENET_MEAN, IMAGENET_STD = (0.485, 0.456, 0.406), (0.229, 0.224, 0.225)


def constants(mean, std):
    """scale = 1 / (255 std), bias = -mean / std in double, each then converted to float32"""
    mean, std = np.asarray(mean, np.float64), np.asarray(std, np.float64)
    return (1.0 / (255.0 * std)).astype(np.float32), (-mean / std).astype(np.float32)
