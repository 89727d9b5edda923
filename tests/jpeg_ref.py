"""NumPy restatement of the JPEG encoder of csrc/hip/jpeg_encode.hip (DESIGN.md 3 "JPEG output"), and a small baseline
entropy decoder for the files it writes.  Integer arithmetic only, every intermediate within int32 (asserted); the kernel, this
file and DESIGN.md state the same thing:

  samples   planar Y | Cb | Cr of w x h (both even), taken as they are; MCU = 16x16 luma (blocks Y00 Y01 Y10 Y11) + 8x8 Cb + 8x8 Cr,
            MCUs in raster order; samples beyond the picture repeat the last column / row
  transform s = sample - 128;  M[u][x] = round(2^14 * c(u)/2 * cos((2x+1) u pi / 16)), c(0) = 1/sqrt 2, else 1
            rows:     t[y][u] = (sum_x M[u][x] * s[y][x] + 2^7) >> 8             (arithmetic shift: 6 fractional bits)
            columns:  z[v][u] = sum_y M[v][y] * t[y][u]                            (20 fractional bits)
            bounds:   sum_x |M[u][x]| <= 46344, so |sum| <= 128 * 46344 < 2^23, |t| <= 23173, |z| <= 46344 * 23173 < 2^30.01
  quantiser level = sign(z) * ((|z| + (q << 19)) / (q << 20)), q = table entry of (v, u): z / 2^20 / q rounded to nearest, ties away
            from zero; |z| + (255 << 19) < 2^30.2
  entropy   Annex K.3 tables, DC predictors reset and bytes aligned (padding bits 1) at every restart interval
"""
import functools

import numpy as np

K1_LUMA = np.array([16, 11, 10, 16, 24, 40, 51, 61, 12, 12, 14, 19, 26, 58, 60, 55, 14, 13, 16, 24, 40, 57, 69, 56,
                    14, 17, 22, 29, 51, 87, 80, 62, 18, 22, 37, 56, 68, 109, 103, 77, 24, 35, 55, 64, 81, 104, 113, 92,
                    49, 64, 78, 87, 103, 121, 120, 101, 72, 92, 95, 98, 112, 100, 103, 99], dtype=np.int64)
K2_CHROMA = np.array([17, 18, 24, 47, 99, 99, 99, 99, 18, 21, 26, 66, 99, 99, 99, 99, 24, 26, 56, 99, 99, 99, 99, 99,
                      47, 66, 99, 99, 99, 99, 99, 99] + [99] * 32, dtype=np.int64)

DC_BITS = ([0, 1, 5, 1, 1, 1, 1, 1, 1, 0, 0, 0, 0, 0, 0, 0], [0, 3, 1, 1, 1, 1, 1, 1, 1, 1, 1, 0, 0, 0, 0, 0])
DC_VALS = (list(range(12)), list(range(12)))
AC_BITS = ([0, 2, 1, 3, 3, 2, 4, 3, 5, 5, 4, 4, 0, 0, 1, 0x7d], [0, 2, 1, 2, 4, 4, 3, 4, 7, 5, 4, 4, 0, 1, 2, 0x77])
AC_VALS = ([
    0x01, 0x02, 0x03, 0x00, 0x04, 0x11, 0x05, 0x12, 0x21, 0x31, 0x41, 0x06, 0x13, 0x51, 0x61, 0x07, 0x22, 0x71, 0x14, 0x32,
    0x81, 0x91, 0xa1, 0x08, 0x23, 0x42, 0xb1, 0xc1, 0x15, 0x52, 0xd1, 0xf0, 0x24, 0x33, 0x62, 0x72, 0x82, 0x09, 0x0a, 0x16,
    0x17, 0x18, 0x19, 0x1a, 0x25, 0x26, 0x27, 0x28, 0x29, 0x2a, 0x34, 0x35, 0x36, 0x37, 0x38, 0x39, 0x3a, 0x43, 0x44, 0x45,
    0x46, 0x47, 0x48, 0x49, 0x4a, 0x53, 0x54, 0x55, 0x56, 0x57, 0x58, 0x59, 0x5a, 0x63, 0x64, 0x65, 0x66, 0x67, 0x68, 0x69,
    0x6a, 0x73, 0x74, 0x75, 0x76, 0x77, 0x78, 0x79, 0x7a, 0x83, 0x84, 0x85, 0x86, 0x87, 0x88, 0x89, 0x8a, 0x92, 0x93, 0x94,
    0x95, 0x96, 0x97, 0x98, 0x99, 0x9a, 0xa2, 0xa3, 0xa4, 0xa5, 0xa6, 0xa7, 0xa8, 0xa9, 0xaa, 0xb2, 0xb3, 0xb4, 0xb5, 0xb6,
    0xb7, 0xb8, 0xb9, 0xba, 0xc2, 0xc3, 0xc4, 0xc5, 0xc6, 0xc7, 0xc8, 0xc9, 0xca, 0xd2, 0xd3, 0xd4, 0xd5, 0xd6, 0xd7, 0xd8,
    0xd9, 0xda, 0xe1, 0xe2, 0xe3, 0xe4, 0xe5, 0xe6, 0xe7, 0xe8, 0xe9, 0xea, 0xf1, 0xf2, 0xf3, 0xf4, 0xf5, 0xf6, 0xf7, 0xf8,
    0xf9, 0xfa], [
    0x00, 0x01, 0x02, 0x03, 0x11, 0x04, 0x05, 0x21, 0x31, 0x06, 0x12, 0x41, 0x51, 0x07, 0x61, 0x71, 0x13, 0x22, 0x32, 0x81,
    0x08, 0x14, 0x42, 0x91, 0xa1, 0xb1, 0xc1, 0x09, 0x23, 0x33, 0x52, 0xf0, 0x15, 0x62, 0x72, 0xd1, 0x0a, 0x16, 0x24, 0x34,
    0xe1, 0x25, 0xf1, 0x17, 0x18, 0x19, 0x1a, 0x26, 0x27, 0x28, 0x29, 0x2a, 0x35, 0x36, 0x37, 0x38, 0x39, 0x3a, 0x43, 0x44,
    0x45, 0x46, 0x47, 0x48, 0x49, 0x4a, 0x53, 0x54, 0x55, 0x56, 0x57, 0x58, 0x59, 0x5a, 0x63, 0x64, 0x65, 0x66, 0x67, 0x68,
    0x69, 0x6a, 0x73, 0x74, 0x75, 0x76, 0x77, 0x78, 0x79, 0x7a, 0x82, 0x83, 0x84, 0x85, 0x86, 0x87, 0x88, 0x89, 0x8a, 0x92,
    0x93, 0x94, 0x95, 0x96, 0x97, 0x98, 0x99, 0x9a, 0xa2, 0xa3, 0xa4, 0xa5, 0xa6, 0xa7, 0xa8, 0xa9, 0xaa, 0xb2, 0xb3, 0xb4,
    0xb5, 0xb6, 0xb7, 0xb8, 0xb9, 0xba, 0xc2, 0xc3, 0xc4, 0xc5, 0xc6, 0xc7, 0xc8, 0xc9, 0xca, 0xd2, 0xd3, 0xd4, 0xd5, 0xd6,
    0xd7, 0xd8, 0xd9, 0xda, 0xe2, 0xe3, 0xe4, 0xe5, 0xe6, 0xe7, 0xe8, 0xe9, 0xea, 0xf2, 0xf3, 0xf4, 0xf5, 0xf6, 0xf7, 0xf8,
    0xf9, 0xfa])

HEADER_BYTES = 625   # SOI 2, APP0 18, DQT 134, SOF0 19, DHT 33 + 183 + 33 + 183, DRI 6, SOS 14
STATUS_OK, STATUS_TOO_BIG = 0, 1


def _zigzag():
    order = sorted(range(64), key=lambda i: (i // 8 + i % 8, (i // 8) if (i // 8 + i % 8) % 2 else (i % 8)))
    return np.array(order)


ZIGZAG = _zigzag()      # ZIGZAG[k] = row-major index (v * 8 + u) of the k-th coefficient in zigzag order


def dct_matrix():
    u, x = np.arange(8)[:, None], np.arange(8)[None, :]
    c = np.where(u == 0, np.sqrt(0.5), 1.0)
    return np.rint(16384.0 * c / 2 * np.cos((2 * x + 1) * u * np.pi / 16)).astype(np.int64)


def quant_tables(quality):
    """(2, 64) in row-major order: the Annex K.1 / K.2 tables scaled by the IJG rule"""
    q = min(max(int(quality), 1), 100)
    scale = 5000 // q if q < 50 else 200 - 2 * q
    return np.stack([np.clip((b * scale + 50) // 100, 1, 255) for b in (K1_LUMA, K2_CHROMA)])


def mcu_blocks(yuv, w, h):
    """(mcus, 6, 8, 8) uint8 samples in coding order, edges repeated"""
    assert w % 2 == 0 and h % 2 == 0 and w >= 2 and h >= 2
    yuv = np.asarray(yuv, dtype=np.uint8).reshape(-1)
    assert yuv.size == w * h * 3 // 2
    mw, mh = (w + 15) // 16, (h + 15) // 16
    Y = yuv[:w * h].reshape(h, w)
    cw, ch = w // 2, h // 2
    Cb = yuv[w * h:w * h + cw * ch].reshape(ch, cw)
    Cr = yuv[w * h + cw * ch:].reshape(ch, cw)

    def pad(P, H, W):
        return P[np.minimum(np.arange(H), P.shape[0] - 1)][:, np.minimum(np.arange(W), P.shape[1] - 1)]

    Yp = pad(Y, mh * 16, mw * 16).reshape(mh, 2, 8, mw, 2, 8).transpose(0, 3, 1, 4, 2, 5).reshape(mh * mw, 4, 8, 8)
    Cbp = pad(Cb, mh * 8, mw * 8).reshape(mh, 8, mw, 8).transpose(0, 2, 1, 3).reshape(mh * mw, 1, 8, 8)
    Crp = pad(Cr, mh * 8, mw * 8).reshape(mh, 8, mw, 8).transpose(0, 2, 1, 3).reshape(mh * mw, 1, 8, 8)
    return np.concatenate([Yp, Cbp, Crp], axis=1)


def transform(blocks):
    """(..., 8, 8) samples -> z[v][u] with 20 fractional bits (int64 holding values that fit int32)"""
    M = dct_matrix()
    s = blocks.astype(np.int64) - 128
    t = np.einsum("ux,...yx->...yu", M, s)
    assert np.abs(t).max(initial=0) + 128 < 2 ** 31
    t = (t + 128) >> 8
    z = np.einsum("vy,...yu->...vu", M, t)
    assert np.abs(z).max(initial=0) + (255 << 19) < 2 ** 31
    return z


def quantise(z, qt):
    """z (mcus, 6, 8, 8), qt (2, 64) row-major -> levels (mcus, 6, 64) in zigzag order"""
    q = np.stack([qt[0]] * 4 + [qt[1]] * 2).reshape(1, 6, 8, 8)
    lv = np.sign(z) * ((np.abs(z) + (q << 19)) // (q << 20))
    return lv.reshape(z.shape[0], 6, 64)[:, :, ZIGZAG]


def quantised(yuv, w, h, quality):
    return quantise(transform(mcu_blocks(yuv, w, h)), quant_tables(quality))


def _codes(bits, vals):
    """Annex C: value -> (code, length)"""
    out, code, k = {}, 0, 0
    for ln in range(1, 17):
        for _ in range(bits[ln - 1]):
            out[vals[k]] = (code, ln)
            code += 1
            k += 1
        code <<= 1
    return out


DC_CODES = [_codes(DC_BITS[i], DC_VALS[i]) for i in range(2)]
AC_CODES = [_codes(AC_BITS[i], AC_VALS[i]) for i in range(2)]


def header(w, h, quality, restart_mcus):
    qt = quant_tables(quality)
    b = bytearray(b"\xff\xd8")
    b += b"\xff\xe0\x00\x10JFIF\x00\x01\x01\x00\x00\x01\x00\x01\x00\x00"
    b += b"\xff\xdb\x00\x84\x00" + bytes(qt[0][ZIGZAG].tolist()) + b"\x01" + bytes(qt[1][ZIGZAG].tolist())
    b += b"\xff\xc0\x00\x11\x08" + bytes([h >> 8, h & 255, w >> 8, w & 255]) + b"\x03\x01\x22\x00\x02\x11\x01\x03\x11\x01"
    for tc, bits, vals in ((0x00, DC_BITS[0], DC_VALS[0]), (0x10, AC_BITS[0], AC_VALS[0]),
                           (0x01, DC_BITS[1], DC_VALS[1]), (0x11, AC_BITS[1], AC_VALS[1])):
        n = 2 + 1 + 16 + len(vals)
        b += b"\xff\xc4" + bytes([n >> 8, n & 255, tc]) + bytes(bits) + bytes(vals)
    b += b"\xff\xdd\x00\x04" + bytes([restart_mcus >> 8, restart_mcus & 255])
    b += b"\xff\xda\x00\x0c\x03\x01\x00\x02\x11\x03\x11\x00\x3f\x00"
    assert len(b) == HEADER_BYTES
    return bytes(b)


def default_restart(w):
    return (w + 15) // 16


class _Events:
    """what the entropy coder met (the GPU tests assert that their content reaches every case)"""

    def __init__(self):
        self.dc_cat, self.ac_cat, self.runs = set(), set(), set()
        self.no_eob = self.zero_blocks = self.stuffed = self.stuffed_at_end = 0


def _interval(levels, ev):
    """levels (m, 6, 64) of one restart interval -> its bytes (stuffed, padded with 1-bits), without the marker"""
    acc, nb = 0, 0
    pred = [0, 0, 0]
    for mcu in levels.tolist():
        for k, blk in enumerate(mcu):
            comp = 0 if k < 4 else k - 3
            tab = 1 if comp else 0
            d = blk[0] - pred[comp]
            pred[comp] = blk[0]
            cat = abs(d).bit_length()
            code, ln = DC_CODES[tab][cat]
            acc, nb = (acc << ln) | code, nb + ln
            if cat:
                acc, nb = (acc << cat) | ((d if d >= 0 else d - 1) & ((1 << cat) - 1)), nb + cat
            if ev is not None:
                ev.dc_cat.add(cat)
                if not any(blk[1:]):
                    ev.zero_blocks += 1
            run, last = 0, 0
            for i in range(1, 64):
                v = blk[i]
                if v == 0:
                    run += 1
                    continue
                if ev is not None:
                    ev.runs.add(run)
                while run >= 16:
                    code, ln = AC_CODES[tab][0xf0]
                    acc, nb = (acc << ln) | code, nb + ln
                    run -= 16
                sz = abs(v).bit_length()
                assert sz <= 10, "AC level outside baseline range"
                code, ln = AC_CODES[tab][(run << 4) | sz]
                acc, nb = (acc << ln) | code, nb + ln
                acc, nb = (acc << sz) | ((v if v >= 0 else v - 1) & ((1 << sz) - 1)), nb + sz
                if ev is not None:
                    ev.ac_cat.add(sz)
                run, last = 0, i
            if last != 63:
                code, ln = AC_CODES[tab][0x00]
                acc, nb = (acc << ln) | code, nb + ln
            elif ev is not None:
                ev.no_eob += 1
    pad = (-nb) % 8
    acc, nb = (acc << pad) | ((1 << pad) - 1), nb + pad
    raw = acc.to_bytes(nb // 8, "big")
    if ev is not None:
        ev.stuffed += raw.count(b"\xff")
        ev.stuffed_at_end += raw.endswith(b"\xff")
    return raw.replace(b"\xff", b"\xff\x00")


def encode_levels(levels, w, h, quality, restart_mcus=None, events=None):
    R = default_restart(w) if restart_mcus is None else int(restart_mcus)
    assert 1 <= R <= 65535
    out = bytearray(header(w, h, quality, R))
    n = levels.shape[0]
    for r, m0 in enumerate(range(0, n, R)):
        out += _interval(levels[m0:m0 + R], events)
        out += b"\xff\xd9" if m0 + R >= n else bytes([0xff, 0xd0 + (r & 7)])
    return bytes(out)


def encode(yuv, w, h, quality=75, restart_mcus=None, events=None):
    """planar Y | Cb | Cr of w x h -> the JPEG file"""
    return encode_levels(quantised(yuv, w, h, quality), w, h, quality, restart_mcus, events)


def events(yuv, w, h, quality=75, restart_mcus=None):
    ev = _Events()
    encode(yuv, w, h, quality, restart_mcus, ev)
    return ev


def blob_layout(lengths, capacity):
    """the batch rule: pictures in order at 16-byte-aligned offsets; one that does not fit gets (offset, 0, STATUS_TOO_BIG) and
    takes no room"""
    table, pos = [], 0
    for ln in lengths:
        if pos + ln <= capacity:
            table.append((pos, ln, STATUS_OK))
            pos = (pos + ln + 15) & ~15
        else:
            table.append((pos, 0, STATUS_TOO_BIG))
    return table


# ---------------------------------------------------------------------------------------------------------------------
# a baseline entropy decoder for exactly this kind of file: back to the quantised levels
# ---------------------------------------------------------------------------------------------------------------------
class _Bits:
    def __init__(self, data):
        self.v = int.from_bytes(data, "big") if data else 0
        self.n = len(data) * 8

    def take(self, k):
        assert k <= self.n, "entropy-coded segment ends early"
        self.n -= k
        return (self.v >> self.n) & ((1 << k) - 1)


def _decode_symbol(bits, table):
    code = 0
    for ln in range(1, 17):
        code = (code << 1) | bits.take(1)
        if (code, ln) in table:
            return table[(code, ln)]
    raise AssertionError("no Huffman code matches")


def _extend(v, k):
    return v if k == 0 or v >> (k - 1) else v - (1 << k) + 1


def decode_levels(data):
    """-> dict(w, h, restart, qt (2, 64) row-major, levels (mcus, 6, 64) zigzag).  Checks the marker order, the RSTm sequence,
    that padding bits are ones and that the file ends with EOI."""
    assert data[:2] == b"\xff\xd8"
    i, qt, huff, info = 2, {}, {}, {}
    seen = []
    while True:
        assert data[i] == 0xff
        m, L = data[i + 1], (data[i + 2] << 8) | data[i + 3]
        seg = data[i + 4:i + 2 + L]
        seen.append(m)
        if m == 0xdb:
            p = 0
            while p < len(seg):
                assert seg[p] >> 4 == 0
                t = np.zeros(64, dtype=np.int64)
                t[ZIGZAG] = list(seg[p + 1:p + 65])
                qt[seg[p] & 15] = t
                p += 65
        elif m == 0xc0:
            assert seg[0] == 8 and seg[5] == 3
            info["h"], info["w"] = (seg[1] << 8) | seg[2], (seg[3] << 8) | seg[4]
            assert bytes(seg[6:15]) == b"\x01\x22\x00\x02\x11\x01\x03\x11\x01"
        elif m == 0xc4:
            p = 0
            while p < len(seg):
                bits = list(seg[p + 1:p + 17])
                vals = list(seg[p + 17:p + 17 + sum(bits)])
                huff[seg[p]] = {cl: v for v, cl in _codes(bits, vals).items()}
                p += 17 + len(vals)
        elif m == 0xdd:
            info["restart"] = (seg[0] << 8) | seg[1]
        elif m == 0xda:
            assert bytes(seg) == b"\x03\x01\x00\x02\x11\x03\x11\x00\x3f\x00"
            i += 2 + L
            break
        i += 2 + L
    assert seen == [0xe0, 0xdb, 0xc0, 0xc4, 0xc4, 0xc4, 0xc4, 0xdd, 0xda], seen
    w, h, R = info["w"], info["h"], info["restart"]
    n = ((w + 15) // 16) * ((h + 15) // 16)
    levels = np.zeros((n, 6, 64), dtype=np.int64)
    body = data[i:]
    assert body.endswith(b"\xff\xd9")
    # split at markers (an 0xFF followed by anything but 0x00)
    parts, start, p, rst = [], 0, 0, 0
    while p < len(body) - 1:
        if body[p] == 0xff and body[p + 1] != 0:
            parts.append(body[start:p])
            if body[p + 1] == 0xd9:
                assert p + 2 == len(body)
                break
            assert body[p + 1] == 0xd0 + (rst & 7), "RSTm out of order"
            rst += 1
            start = p + 2
            p += 2
        else:
            p += 1
    assert len(parts) == (n + R - 1) // R
    for r, part in enumerate(parts):
        bits = _Bits(part.replace(b"\xff\x00", b"\xff"))
        pred = [0, 0, 0]
        for mcu in range(r * R, min((r + 1) * R, n)):
            for k in range(6):
                comp = 0 if k < 4 else k - 3
                tab = 1 if comp else 0
                cat = _decode_symbol(bits, huff[tab])
                pred[comp] += _extend(bits.take(cat), cat)
                levels[mcu, k, 0] = pred[comp]
                pos = 1
                while pos < 64:
                    rs = _decode_symbol(bits, huff[0x10 | tab])
                    run, sz = rs >> 4, rs & 15
                    if sz == 0:
                        if run == 15:
                            pos += 16
                            continue
                        assert run == 0
                        break
                    pos += run
                    assert pos < 64
                    levels[mcu, k, pos] = _extend(bits.take(sz), sz)
                    pos += 1
        k = bits.n
        assert k < 8 and bits.take(k) == (1 << k) - 1, "padding bits are not ones"
    return {"w": w, "h": h, "restart": R, "qt": np.stack([qt[0], qt[1]]), "levels": levels}


# ---------------------------------------------------------------------------------------------------------------------
# test content, built in the coefficient domain: 8x8 tiles that are the inverse transform (float, clipped, rounded) of
# chosen coefficients, so that at quality 100 (quantisers of 1) the entropy coder meets every case -- see events()
# ---------------------------------------------------------------------------------------------------------------------
def _idct_tiles(coef):
    """(n, 64) coefficients in zigzag order -> (n, 8, 8) uint8 samples"""
    u, x = np.arange(8)[:, None], np.arange(8)[None, :]
    C = np.where(u == 0, np.sqrt(0.5), 1.0) / 2 * np.cos((2 * x + 1) * u * np.pi / 16)
    nat = np.zeros((coef.shape[0], 64))
    nat[:, ZIGZAG] = coef
    s = np.einsum("vy,nvu,ux->nyx", C, nat.reshape(-1, 8, 8), C)
    return np.clip(np.rint(s + 128), 0, 255).astype(np.uint8)


@functools.lru_cache(maxsize=None)
def tile_pool(seed):
    rng = np.random.default_rng(seed)
    coef = []
    for dc in (-1024, 1016, -1024, 1016, 0, 400):          # flat tiles: DC differences of category 11, all-zero AC
        c = np.zeros(64)
        c[0] = dc
        coef.append(c)
    for cat in range(1, 11):                                # one AC coefficient in the middle of every category
        for pos in (1, 2, 5):
            c = np.zeros(64)
            c[0] = rng.integers(-200, 200)
            c[pos] = (3 << cat) // 4 * (1 if pos != 2 else -1)
            if cat == 10:
                c[0], c[pos] = 0, 1400                      # clipped to a square wave: about 900
            coef.append(c)
    tiles = [_idct_tiles(np.array(coef))]
    ones = np.ones((2, 64), dtype=np.int64)
    for run in (15, 16, 17, 33):                            # two coefficients `run` zeros apart.  Rounding the samples adds +-1
        n = 2000                                            # levels of its own, so keep the tiles that the model codes with
        a = rng.integers(1, 62 - run, n)                    # exactly that run
        c = np.zeros((n, 64))
        c[:, 0] = 8 * rng.integers(-60, 60, n)
        c[np.arange(n), a] = rng.integers(3, 40, n)
        c[np.arange(n), a + run + 1] = rng.integers(3, 40, n) * rng.choice([-1, 1], n)
        t = _idct_tiles(c)
        lv = quantise(transform(t[:, None]), ones)[:, 0]
        between = (np.arange(64)[None, :] > a[:, None]) & (np.arange(64)[None, :] <= (a + run)[:, None])
        good = ((lv != 0) & between).sum(axis=1) == 0
        good &= (lv[np.arange(n), a] != 0) & (lv[np.arange(n), a + run + 1] != 0)
        assert good.sum() >= 4, run
        tiles.append(t[good][:12])
    tiles.append(rng.integers(0, 256, (64, 8, 8), dtype=np.uint8))   # dense noise: no EOB, 0xFF bytes
    return np.concatenate(tiles)


@functools.lru_cache(maxsize=None)
def model_file(w, h, seed, quality, restart_mcus=None):
    """the model's file of content(w, h, seed): computed once per session, shared by the tests"""
    return encode(content(w, h, seed), w, h, quality, restart_mcus)


def content(w, h, seed):
    """planar Y | Cb | Cr of w x h: tiles of one of four pools in an order shuffled by the seed, cut at the picture's edges"""
    rng = np.random.default_rng(seed + 1000)
    pool = tile_pool(seed & 3)
    planes = []
    for pw, ph in ((w, h), (w // 2, h // 2), (w // 2, h // 2)):
        tw, th = (pw + 7) // 8, (ph + 7) // 8
        pick = pool[rng.permutation(max(tw * th, len(pool)))[:tw * th] % len(pool)]
        plane = pick.reshape(th, tw, 8, 8).transpose(0, 2, 1, 3).reshape(th * 8, tw * 8)
        planes.append(plane[:ph, :pw].reshape(-1))
    return np.concatenate(planes)
