"""NumPy restatement of the output-geometry pass (DESIGN.md 3 "Output geometry"; resample.hip / resample_taps.h): the tap
weights, the size rule, crop + area-average resampling of the planes (vertical pass first) and the colour conversion of the
output planes (the reference's integer formula, 2x2-nearest chroma).  Checked against plain per-sample loops in
tests/test_thumbnail.py."""
import numpy as np

ONE = 1 << 14


def fit(cw, ch, bw, bh):
    """the size rule: cw x ch (even) into a bw x bh box (each >= 2) -> (ow, oh)"""
    if cw <= bw and ch <= bh:
        return cw, ch
    if cw * bh >= ch * bw:
        ow = bw & ~1
        oh = min(max(2 * ((ch * ow + cw) // (2 * cw)), 2), bh & ~1)
    else:
        oh = bh & ~1
        ow = min(max(2 * ((cw * oh + ch) // (2 * ch)), 2), bw & ~1)
    return ow, oh


def taps(S, D):
    """weight matrix W[D, S] (int64): W[j, i] = F(C(i + 1)) - F(C(i)), C(i) = clamp(i D - j S, 0, S),
    F(c) = (c 2^14 + S // 2) // S"""
    j = np.arange(D, dtype=np.int64)[:, None]
    i = np.arange(S + 1, dtype=np.int64)[None, :]
    c = np.clip(i * D - j * S, 0, S)
    F = (c * ONE + S // 2) // S
    return F[:, 1:] - F[:, :-1]


def resample_plane(plane, x0, y0, sw, sh, dw, dh):
    """one plane (2-D uint8) -> its cropped rectangle resampled to dw x dh"""
    src = plane[y0:y0 + sh, x0:x0 + sw].astype(np.int64)
    t = (taps(sh, dh) @ src + 32) >> 6                  # vertical: 16-bit, 8 fractional bits
    return ((t @ taps(sw, dw).T + (1 << 21)) >> 22).astype(np.uint8)


def resample(yuv, width_mbs, height_mbs, geom):
    """coded pictures (n x W*H*384 bytes) -> output planes (n x ow*oh*3/2), geom = (cx, cy, cw, ch, ow, oh)"""
    cx, cy, cw, ch, ow, oh = geom
    Wp, Hp = 16 * width_mbs, 16 * height_mbs
    yuv = np.ascontiguousarray(yuv, np.uint8).reshape(-1, Wp * Hp * 3 // 2)
    out = np.zeros((yuv.shape[0], ow * oh * 3 // 2), np.uint8)
    for f in range(yuv.shape[0]):
        Y = yuv[f, :Wp * Hp].reshape(Hp, Wp)
        Cb = yuv[f, Wp * Hp:Wp * Hp * 5 // 4].reshape(Hp // 2, Wp // 2)
        Cr = yuv[f, Wp * Hp * 5 // 4:].reshape(Hp // 2, Wp // 2)
        out[f, :ow * oh] = resample_plane(Y, cx, cy, cw, ch, ow, oh).reshape(-1)
        q = (ow // 2) * (oh // 2)
        out[f, ow * oh:ow * oh + q] = resample_plane(Cb, cx // 2, cy // 2, cw // 2, ch // 2, ow // 2, oh // 2).reshape(-1)
        out[f, ow * oh + q:] = resample_plane(Cr, cx // 2, cy // 2, cw // 2, ch // 2, ow // 2, oh // 2).reshape(-1)
    return out


def to_rgb(planes, ow, oh):
    """output planes (n x ow*oh*3/2) -> RGB8 (n x ow*oh*3): export_utils.c:300-302, chroma (x / 2, y / 2)"""
    planes = np.ascontiguousarray(planes, np.uint8).reshape(-1, ow * oh * 3 // 2)
    n, q = planes.shape[0], (ow // 2) * (oh // 2)
    Y = planes[:, :ow * oh].reshape(n, oh, ow).astype(np.int32)
    Cb = planes[:, ow * oh:ow * oh + q].reshape(n, oh // 2, ow // 2).astype(np.int32).repeat(2, 1).repeat(2, 2)
    Cr = planes[:, ow * oh + q:].reshape(n, oh // 2, ow // 2).astype(np.int32).repeat(2, 1).repeat(2, 2)
    ly = (298 * Y) >> 8
    r = ly + ((408 * Cr) >> 8) - 222
    g = ly - ((100 * Cb) >> 8) - ((208 * Cr) >> 8) + 135
    b = ly + ((516 * Cb) >> 8) - 276
    return np.clip(np.stack([r, g, b], -1), 0, 255).astype(np.uint8).reshape(n, -1)


# ---- plain per-sample loops: what the vectorised forms above are checked against ----
def weight_loop(S, D, j, i):
    def F(c):
        return (c * ONE + S // 2) // S

    def C(k):
        return min(max(k * D - j * S, 0), S)
    return F(C(i + 1)) - F(C(i))


def resample_plane_loop(plane, x0, y0, sw, sh, dw, dh):
    t = [[0] * sw for _ in range(dh)]
    for j in range(dh):
        for x in range(sw):
            acc = sum(weight_loop(sh, dh, j, i) * int(plane[y0 + i, x0 + x]) for i in range(sh))
            t[j][x] = (acc + 32) >> 6
    out = np.zeros((dh, dw), np.uint8)
    for j in range(dh):
        for k in range(dw):
            acc = sum(weight_loop(sw, dw, k, i) * t[j][i] for i in range(sw))
            out[j, k] = (acc + (1 << 21)) >> 22
    return out
