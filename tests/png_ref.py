"""The PNG encoder's file format (png_encode.hip, DESIGN.md 3 "PNG output") restated in NumPy / plain Python.  A file is a function
of the RGB samples alone:

  container   signature, IHDR (8 bit, colour type 2, no interlace), one IDAT per segment, IEND
  filtering   per row the type 0 .. 4 with the least sum of min(f, 256 - f) over the row's 3 w filtered bytes, ties to the lowest
              type; the row above row 0 is zeros, and a segment's first row is filtered against the picture's real row above
  segments    R = max(1, 32768 // (3 w + 1)) rows each, the last one maybe shorter; each is one deflate block that starts on a byte
  dynamic     HLIT = 257, HDIST = 1, HCLEN = 19; code-length code = symbols 0 .. 15 at four bits; 257 lengths at four bits, one
              distance length of 0, the literals, end-of-block, then an empty stored block (3 bits, padding, 00 00 FF FF) that
              carries BFINAL on the last segment
  lengths     Huffman over the segment's histogram (256 literals + end-of-block with count 1): nodes ordered by (count, index),
              internal nodes numbered behind the leaves in order of creation; while the longest code passes 15 bits every
              non-zero count becomes (c + 1) >> 1 and the construction runs again; canonical codes
  stored      a segment whose dynamic block would not be shorter is one stored block (5 bytes + data)
  checksums   78 01 opens the first segment's IDAT, the Adler-32 of all filtered bytes closes the last one
"""
import functools
import heapq
import struct
import zlib

import numpy as np

SIGNATURE = b"\x89PNG\r\n\x1a\n"
HEADER_BYTES = 33                      # signature + IHDR chunk
DYN_HEADER_BITS = 17 + 19 * 3 + 257 * 4 + 4
CL_ORDER = (16, 17, 18, 0, 8, 7, 9, 6, 10, 5, 11, 4, 12, 3, 13, 2, 14, 1, 15)
STATUS_OK, STATUS_TOO_BIG = 0, 1
MAX_WIDTH = 21844                      # 3 w + 1 <= 65535: a row fits a stored block


def segment_rows(w):
    return max(1, 32768 // (3 * w + 1))


def max_bytes(w, h):
    """every segment stored: signature + IHDR + IEND (45), per segment chunk framing (12) and block header (5), zlib header and
    Adler-32 (6), the filtered bytes"""
    R = segment_rows(w)
    return 45 + 6 + 17 * ((h + R - 1) // R) + h * (3 * w + 1)


def chunk(kind, payload):
    return struct.pack(">I", len(payload)) + kind + payload + struct.pack(">I", zlib.crc32(kind + payload))


# ---------------------------------------------------------------------------------------------------------------------
# filtering
# ---------------------------------------------------------------------------------------------------------------------
def filter_rows(rgb, w, h):
    """(h, 3 w) uint8 -> (types (h,), filtered (h, 3 w) uint8 of the chosen types, cost (h, 5))"""
    x = np.asarray(rgb, dtype=np.uint8).reshape(h, 3 * w).astype(np.int32)
    a = np.zeros_like(x)
    a[:, 3:] = x[:, :-3]
    b = np.zeros_like(x)
    b[1:] = x[:-1]
    c = np.zeros_like(x)
    c[:, 3:] = b[:, :-3]
    p = a + b - c
    pa, pb, pc = np.abs(p - a), np.abs(p - b), np.abs(p - c)
    paeth = np.where((pa <= pb) & (pa <= pc), a, np.where(pb <= pc, b, c))
    f = np.stack([x, x - a, x - b, x - ((a + b) >> 1), x - paeth]) & 255          # (5, h, 3 w)
    cost = np.where(f < 128, f, 256 - f).sum(axis=2).T                           # (h, 5)
    types = cost.argmin(axis=1)                                                  # (the first least one: ties to the lowest type)
    return types.astype(np.uint8), f[types, np.arange(h)].astype(np.uint8), cost


# ---------------------------------------------------------------------------------------------------------------------
# code lengths
# ---------------------------------------------------------------------------------------------------------------------
def huffman_depths(counts):
    """depths of the leaves with a non-zero count.  Nodes are ordered by (count, index); leaves carry their symbol as index,
    internal nodes 257, 258, ... in order of creation."""
    heap = [(int(c), i) for i, c in enumerate(counts) if c]
    assert len(heap) >= 2
    heapq.heapify(heap)
    parent = {}
    nxt = len(counts)
    while len(heap) > 1:
        c0, i0 = heapq.heappop(heap)
        c1, i1 = heapq.heappop(heap)
        parent[i0] = parent[i1] = nxt
        heapq.heappush(heap, (c0 + c1, nxt))
        nxt += 1
    depth = {nxt - 1: 0}
    for i in range(nxt - 2, len(counts) - 1, -1):
        depth[i] = depth[parent[i]] + 1
    out = np.zeros(len(counts), dtype=np.int64)
    for i, c in enumerate(counts):
        if c:
            out[i] = depth[parent[i]] + 1
    return out


def code_lengths(hist):
    """hist: 256 literal counts -> (257 lengths of at most 15 bits, number of halvings)"""
    counts = np.concatenate([np.asarray(hist, dtype=np.int64), [1]])
    halvings = 0
    while True:
        lens = huffman_depths(counts)
        if lens.max() <= 15:
            return lens, halvings
        counts = np.where(counts > 0, (counts + 1) >> 1, 0)
        halvings += 1


def canonical_codes(lens):
    """RFC 1951 3.2.2"""
    bl = np.bincount(lens, minlength=16)
    bl[0] = 0
    nxt = np.zeros(17, dtype=np.int64)
    code = 0
    for b in range(1, 16):
        code = (code + bl[b - 1]) << 1
        nxt[b] = code
    codes = np.zeros(len(lens), dtype=np.int64)
    for s, l in enumerate(lens):
        if l:
            codes[s] = nxt[l]
            nxt[l] += 1
    return codes


class _BitWriter:
    def __init__(self):
        self.acc, self.n, self.out = 0, 0, bytearray()

    def bits(self, v, n):           # plain integers: least significant bit first
        self.acc |= int(v) << self.n
        self.n += n
        while self.n >= 8:
            self.out.append(self.acc & 255)
            self.acc >>= 8
            self.n -= 8

    def code(self, c, n):           # Huffman codes: most significant bit first
        self.bits(int(format(int(c), "0%db" % n)[::-1], 2), n)

    def align(self):
        if self.n:
            self.bits(0, 8 - self.n)


def dynamic_block(data, lens, last):
    codes = canonical_codes(lens)
    w = _BitWriter()
    w.bits(0, 1)
    w.bits(2, 2)
    w.bits(0, 5)                    # HLIT = 257
    w.bits(0, 5)                    # HDIST = 1
    w.bits(15, 4)                   # HCLEN = 19
    for s in CL_ORDER:
        w.bits(4 if s < 16 else 0, 3)
    for l in lens:
        w.code(l, 4)                # (the code-length code: sixteen codes of four bits, symbol = code)
    w.code(0, 4)                    # one distance length: 0
    for v in data:
        w.code(codes[v], lens[v])
    w.code(codes[256], lens[256])
    w.bits(1 if last else 0, 1)     # the empty stored block
    w.bits(0, 2)
    w.align()
    return bytes(w.out) + b"\x00\x00\xff\xff"


def stored_block(data, last):
    n = len(data)
    assert n <= 65535
    return bytes([1 if last else 0]) + struct.pack("<HH", n, n ^ 0xffff) + bytes(data)


class Trace:
    """what the encoder met: one record per segment"""
    def __init__(self):
        self.types, self.cost, self.ties, self.segments = None, None, None, []   # per row; segments: one dict each


def encode(rgb, w, h, trace=None):
    """(h, w, 3) or flat RGB8 -> the file's bytes"""
    assert w >= 1 and h >= 1 and w <= MAX_WIDTH
    types, filt, cost = filter_rows(rgb, w, h)
    stream = np.concatenate([types[:, None], filt], axis=1)                      # (h, 3 w + 1)
    R = segment_rows(w)
    S = (h + R - 1) // R
    out = [SIGNATURE, chunk(b"IHDR", struct.pack(">IIBBBBB", w, h, 8, 2, 0, 0, 0))]
    if trace is not None:
        trace.types, trace.cost = types, cost
        trace.ties = [int((cost[y] == cost[y].min()).sum()) > 1 for y in range(h)]
    for s in range(S):
        data = stream[s * R:min((s + 1) * R, h)].reshape(-1)
        hist = np.bincount(data, minlength=256)
        lens, halvings = code_lengths(hist)
        bits = DYN_HEADER_BITS + int((hist * lens[:256]).sum()) + int(lens[256]) + 3
        dyn_bytes = (bits + 7) // 8 + 4
        last = s == S - 1
        if dyn_bytes < 5 + data.size:
            block = dynamic_block(data, lens, last)
            assert len(block) == dyn_bytes
        else:
            block = stored_block(data, last)
        payload = (b"\x78\x01" if s == 0 else b"") + block
        if last:
            payload += struct.pack(">I", zlib.adler32(stream.tobytes()))
        out.append(chunk(b"IDAT", payload))
        if trace is not None:
            trace.segments.append(dict(rows=data.size // (3 * w + 1), bytes=int(data.size), dynamic=dyn_bytes < 5 + data.size,
                                       halvings=halvings, used=int((hist > 0).sum()), lens=lens, chunk=len(out[-1])))
    out.append(chunk(b"IEND", b""))
    f = b"".join(out)
    assert len(f) <= max_bytes(w, h)
    return f


def blob_layout(lengths, cap):
    """the encoder's placement rule: pictures in order, each at the next multiple of 16; one that would pass `cap` is flagged, gets
    length 0 and takes no room.  -> [(offset, length, status)]"""
    out, pos = [], 0
    for n in lengths:
        if pos + n <= cap:
            out.append((pos, n, STATUS_OK))
            pos = (pos + n + 15) & ~15
        else:
            out.append((pos, 0, STATUS_TOO_BIG))
    return out


# ---------------------------------------------------------------------------------------------------------------------
# test content
# ---------------------------------------------------------------------------------------------------------------------
def smooth(w, h, seed, sigma=2.0):
    """a smooth colour field with Gaussian noise of `sigma`: what a decoded photograph looks like to the filters"""
    rng = np.random.default_rng(seed)
    y, x = np.mgrid[0:h, 0:w].astype(np.float64)
    u, v = x / max(w - 1, 1), y / max(h - 1, 1)
    ch = [128 + 90 * np.sin(2.1 * u + 1.3 * v + 0.7 * k + seed) * np.cos(1.7 * v - 0.9 * u + 0.4 * k) for k in range(3)]
    img = np.stack(ch, axis=2) + rng.normal(0, sigma, (h, w, 3))
    return np.clip(np.rint(img), 0, 255).astype(np.uint8)


def content(w, h, seed):
    """(h, w, 3): bands of rows built so that the filters choose every type, flat rows tie, a band of noise falls back to the
    stored form and a flat band uses one literal (tests/test_png.py asserts each on the model's trace, at the sizes it names)"""
    rng = np.random.default_rng(seed + 77)
    img = np.zeros((h, w, 3), dtype=np.uint8)
    base = rng.integers(0, 256, (w, 3))
    kinds = ("noise", "sub", "up", "avg", "paeth", "flat", "smooth")
    band = max(1, h // (2 * len(kinds)))
    for y in range(h):
        kind = kinds[(y // band + seed) % len(kinds)]
        if kind == "noise":                                                       # type 0, and a segment of it is stored
            img[y] = rng.integers(0, 256, (w, 3))
        elif kind == "sub":                                                       # a ramp along the row under a fresh offset
            img[y] = (np.arange(w)[:, None] * np.array([3, 5, 7]) + rng.integers(0, 256, 3)) & 255
        elif kind == "up":                                                        # the row above again (noise along the row)
            img[y] = img[y - 1] if y else base
        elif kind == "avg":                                                       # halfway between left and above
            prev = img[y - 1].astype(np.int64) if y else np.zeros((w, 3), dtype=np.int64)
            row = np.zeros((w, 3), dtype=np.int64)
            for xx in range(w):
                left = row[xx - 1] if xx else 0
                row[xx] = ((left + prev[xx]) >> 1) + (1 if xx % 5 == 0 else 0)
            img[y] = row & 255
        elif kind == "paeth":                                                     # steps: the gradient predictor follows edges
            prev = img[y - 1].astype(np.int64) if y else base.astype(np.int64)
            shift = np.roll(prev, 1, axis=0)
            shift[0] = prev[0]
            img[y] = np.where((np.arange(w)[:, None] // 3 + y) % 2 == 0, prev, shift) & 255
        elif kind == "flat":
            img[y] = 0 if (y // band) % 2 else 200
        else:
            img[y] = smooth(w, 1, seed + y)[0]
    return img


def fibonacci(w, h, seed):
    """rows whose differences along the row (what the Sub filter leaves) take 20 values with counts that grow like a Fibonacci series in every segment:
    the plain Huffman tree of such a histogram is deeper than 15 bits, so the counts are halved"""
    rng = np.random.default_rng(seed)
    R = segment_rows(w)
    fib = [int(np.ceil(1.63 ** k)) for k in range(20)]   # (each count at least the sum of all two or more places below it)
    values = [0, 1, 255, 2, 254, 3, 253, 4, 252, 5, 251, 6, 250, 7, 249, 8, 248, 9, 247, 10, 246, 11]
    res = np.zeros((h, 3 * w), dtype=np.int64)
    for y0 in range(0, h, R):
        rows = min(R, h - y0)
        pool = np.concatenate([np.full(c, v) for v, c in zip(values, fib[::-1])])
        pool = np.concatenate([pool, np.zeros(max(0, rows * 3 * w - pool.size), dtype=np.int64)])[:rows * 3 * w]
        res[y0:y0 + rows] = rng.permutation(pool).reshape(rows, 3 * w)
    img = np.cumsum(res.reshape(h, w, 3), axis=1) & 255                           # (per channel along the row)
    return img.astype(np.uint8)


@functools.lru_cache(maxsize=None)
def model_file(w, h, seed, kind="content"):
    """the model's file of content / smooth (w, h, seed): computed once per session, shared by the tests"""
    return encode(picture(w, h, seed, kind), w, h)


@functools.lru_cache(maxsize=None)
def _picture(w, h, seed, kind):
    if kind == "content":
        p = content(w, h, seed)
    elif kind == "smooth":
        p = smooth(w, h, seed)
    elif kind == "smooth3":
        p = smooth(w, h, seed, 3.0)
    elif kind == "noise":
        p = np.random.default_rng(seed).integers(0, 256, (h, w, 3), dtype=np.uint8)
    elif kind == "flat":
        p = np.full((h, w, 3), seed & 255, dtype=np.uint8)
    elif kind == "fib":
        p = fibonacci(w, h, seed)
    elif kind == "mixed":                                                         # smooth, the middle third of the rows noise
        p = smooth(w, h, seed).copy()
        p[h // 3:2 * h // 3] = np.random.default_rng(seed).integers(0, 256, (2 * h // 3 - h // 3, w, 3), dtype=np.uint8)
    else:
        raise ValueError(kind)
    p.setflags(write=False)
    return p


def picture(w, h, seed, kind="content"):
    return _picture(w, h, seed, kind)
