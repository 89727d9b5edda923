"""A plain, exact model of H.264 intra reconstruction for one picture of packed records (include/minivideo_hotpath.h), written
from the clauses of ITU-T H.264 and not from oracle/recon_ref.c or the kernels.  TEST INFRASTRUCTURE: the authority for the
opt-in spec mode (pictures of several slices, scaling matrices, I_PCM, the standard's luma-DC rule), which the reference decoder
cannot be; tests/test_spec_model.py anchors it to the reference where the two overlap.

Clauses (frame macroblocks, 4:2:0, 8-bit, no MBAFF):
  6.4.8 / 6.4.12   availability of mbAddrA / B / C / D: picture geometry, and -- under MVHP_PARAM_SLICES -- the record's
                   `unavail` bits ("exists, but belongs to another slice")
  8.3.1.2          Intra4x4 sample prediction, the 13 neighbours p[x, y], the rule for luma4x4BlkIdx 3 and 11, the substitution
                   of p[3, -1] for p[4..7, -1]
  8.3.2.2          Intra8x8: the 25 neighbours, substitution of p[7, -1], the reference sample filter 8.3.2.2.1 with each of
                   its "not available" branches, the nine modes on p'
  8.3.3, 8.3.4     Intra16x16 and chroma prediction;  8.3.5  I_PCM
  8.5.9            LevelScale(m, i, j) = weightScale(i, j) * normAdjust(m, i, j), normAdjust from the v tables and position rules
  8.5.10, 8.5.11   luma DC (qP >= 36 shifts left) and chroma DC with Table 8-15
  8.5.12, 8.5.13   scaling and the 4x4 / 8x8 transforms;  8.5.14  u = Clip1(pred + r)

Conventions of the standard kept here: a matrix element c_ij has ROW i and COLUMN j (8.5.12.2 transforms "each (horizontal)
row" over j first; 8.5.14 places r_ij at x = xO + j, y = yO + i), prediction samples are pred[x, y], neighbours p[x, y] with
x = -1 / y = -1 the column left of / the row above the block.  The weight matrices of mvhp_stream_params_t are raster
[i * 4 + j] / [i * 8 + j] by the header's definition.

Formulation: every prediction mode is the standard's equation over a map p[(x, y)] that holds the AVAILABLE neighbours only --
a mode that reads a sample that is not available raises SpecModelError (the reference "predicts 0" there; the standard forbids
the stream); the DC transforms are matrix products; one 1-D butterfly per transform size, applied along rows and then columns.

Arithmetic: Python integers for prediction, numpy int64 for the residuals of a whole picture at once; nothing wraps.  The model
records the largest magnitude at each stage and classifies every macroblock:
  CONFORMANT  every scaled coefficient d_ij, DC-transform value and transform intermediate (e .. h, 8.5.10 - 8.5.13) lies within
              -2^15 .. 2^15 - 1, the bound the standard sets for 8-bit video;
  INT32_SAFE  not conformant, but every value the straightforward evaluation forms (products level * LevelScale, the rounding
              add, the shifted products, every intermediate, h + 32) fits in int32;
  BEYOND      something does not fit in int32.

ONE non-standard switch: luma_dc_from (default 36, the standard's `qP >= 36` of 8.5.10).  37 reproduces the reference decoder's
`qP > 36` defect: at QP'Y = 36 it evaluates (f * LevelScale + (1 << -1)) >> 0 in C int, observable as two's-complement
arithmetic with the shift count taken modulo 32.  For exactly those macroblocks (Intra16x16, QP'Y 36, luma_dc_from 37) the luma
residual is computed with explicit 32-bit wrapping, they are flagged in Result.defect and classified on the wrapped values.  The
switch exists only so that the anchor to the reference leaves no picture out."""
import numpy as np

SLICES, SCALING = 4, 8                      # MVHP_PARAM_SLICES, MVHP_PARAM_SCALING
SPEC_LUMA_DC = 2                            # MVHP_PARAM_SPEC_LUMA_DC
UNAVAIL_A, UNAVAIL_B, UNAVAIL_C, UNAVAIL_D = 1, 2, 4, 8
I4x4, I8x8, I16x16, IPCM = 0, 1, 2, 3
CONFORMANT, INT32_SAFE, BEYOND = 0, 1, 2
CLASS_NAMES = ("conformant", "int32-safe", "beyond")
LIM16, LIM32 = (1 << 15) - 1, (1 << 31) - 1


class SpecModelError(ValueError):
    """the records are not a legal picture (a prediction mode whose neighbours are not available, an unknown kind or mode)"""


# ---- 8.5.9: normAdjust from the v tables and the position rules ------------------------------------------------------------
_V4 = ((10, 16, 13), (11, 18, 14), (13, 20, 16), (14, 23, 18), (16, 25, 20), (18, 29, 23))
_V8 = ((20, 18, 32, 19, 25, 24), (22, 19, 35, 21, 28, 26), (26, 23, 42, 24, 33, 31),
       (28, 25, 45, 26, 35, 33), (32, 28, 51, 30, 40, 38), (36, 32, 58, 34, 46, 43))


def _norm_adjust4(m):
    out = np.zeros((4, 4), np.int64)
    for i in range(4):
        for j in range(4):
            if i % 2 == 0 and j % 2 == 0:
                out[i, j] = _V4[m][0]
            elif i % 2 == 1 and j % 2 == 1:
                out[i, j] = _V4[m][1]
            else:
                out[i, j] = _V4[m][2]
    return out


def _norm_adjust8(m):
    out = np.zeros((8, 8), np.int64)
    for i in range(8):
        for j in range(8):
            if i % 4 == 0 and j % 4 == 0:
                k = 0
            elif i % 2 == 1 and j % 2 == 1:
                k = 1
            elif i % 4 == 2 and j % 4 == 2:
                k = 2
            elif (i % 4 == 0 and j % 2 == 1) or (i % 2 == 1 and j % 4 == 0):
                k = 3
            elif (i % 4 == 0 and j % 4 == 2) or (i % 4 == 2 and j % 4 == 0):
                k = 4
            else:
                k = 5
            out[i, j] = _V8[m][k]
    return out


_NA4 = np.stack([_norm_adjust4(m) for m in range(6)])        # [m, i, j]
_NA8 = np.stack([_norm_adjust8(m) for m in range(6)])

# Table 8-15: QPc as a function of qPI
_QPC = list(range(30)) + [29, 30, 31, 32, 32, 33, 34, 34, 35, 35, 36, 36, 37, 37, 37, 38, 38, 38, 39, 39, 39, 39]

# 6.4.3: inverse 4x4 luma block scan, luma4x4BlkIdx -> (x, y)
_BLK4 = [(8 * ((b // 4) % 2) + 4 * ((b % 4) % 2), 8 * ((b // 4) // 2) + 4 * ((b % 4) // 2)) for b in range(16)]

_H4 = np.array([[1, 1, 1, 1], [1, 1, -1, -1], [1, -1, -1, 1], [1, -1, 1, -1]], np.int64)      # 8.5.10
_A2 = np.array([[1, 1], [1, -1]], np.int64)                                                  # 8.5.11.1


class _Track:
    """per-macroblock magnitudes: mag(v) = max(v, -v - 1), so that v fits n bits signed exactly when mag(v) <= 2^(n-1) - 1"""

    def __init__(self, n):
        self.scaled = np.zeros(n, np.int64)       # d_ij, f_ij / dcY / dcC of the DC transforms
        self.transform = np.zeros(n, np.int64)    # e, f, g, h (and the 8x8 transform's further stages)
        self.preshift = np.zeros(n, np.int64)     # h + 32
        self.product = np.zeros(n, np.int64)      # level * LevelScale, + rounding term, << shift

    def see(self, stage, v, sel):
        if v.size == 0:
            return
        v = v.reshape(v.shape[0], -1)
        m = np.maximum(v, -v - 1).max(axis=1)
        cur = getattr(self, stage)
        cur[sel] = np.maximum(cur[sel], m)


def _w32(v):
    """two's-complement wrap to 32 bits (the luma_dc_from = 37 defect path only)"""
    return ((v + (1 << 31)) & 0xFFFFFFFF) - (1 << 31)


def _ident(v):
    return v


def _t4(d, see, wrap=_ident):
    """8.5.12.2, one dimension, along the last axis"""
    d0, d1, d2, d3 = (d[..., k] for k in range(4))
    e = [wrap(d0 + d2), wrap(d0 - d2), wrap((d1 >> 1) - d3), wrap(d1 + (d3 >> 1))]
    f = [wrap(e[0] + e[3]), wrap(e[1] + e[2]), wrap(e[1] - e[2]), wrap(e[0] - e[3])]
    out = np.stack(f, axis=-1)
    see(np.stack(e, axis=-1))
    see(out)
    return out


def _t8(d, see):
    """8.5.13.2, one dimension, along the last axis"""
    a = [d[..., k] for k in range(8)]
    b = [a[0] + a[4],
         -a[3] + a[5] - a[7] - (a[7] >> 1),
         a[0] - a[4],
         a[1] + a[7] - a[3] - (a[3] >> 1),
         (a[2] >> 1) - a[6],
         -a[1] + a[7] + a[5] + (a[5] >> 1),
         a[2] + (a[6] >> 1),
         a[3] + a[5] + a[1] + (a[1] >> 1)]
    c = [b[0] + b[6], b[1] + (b[7] >> 2), b[2] + b[4], b[3] + (b[5] >> 2),
         b[2] - b[4], (b[3] >> 2) - b[5], b[0] - b[6], b[7] - (b[1] >> 2)]
    g = [c[0] + c[7], c[2] + c[5], c[4] + c[3], c[6] + c[1], c[6] - c[1], c[4] - c[3], c[2] - c[5], c[0] - c[7]]
    out = np.stack(g, axis=-1)
    see(np.stack(b, axis=-1))
    see(np.stack(c, axis=-1))
    see(out)
    return out


def _scale(c, ls, qp, full, trk, sel, wrap=_ident):
    """8.5.12.1 (full = 4: qP >= 24 shifts left) / 8.5.13.1 (full = 6: qP >= 36).  c, ls: [n, ..., i, j]; qp: [n]"""
    sh = qp // 6 - full
    shape = (-1,) + (1,) * (c.ndim - 1)
    up = np.maximum(sh, 0).reshape(shape)
    down = np.maximum(-sh, 0).reshape(shape)
    prod = wrap(c * ls)
    rnd = np.where(down > 0, np.int64(1) << np.maximum(down - 1, 0), 0)
    left = wrap(prod << up)
    summed = wrap(prod + rnd)
    d = np.where(down > 0, summed >> down, left)
    trk.see("product", prod, sel)
    trk.see("product", np.where(down > 0, summed, left), sel)
    return d


def _residuals(p, rec, luma_dc_from):
    """the residual stage of a whole picture: r_luma[n, 16, 16] and r_chroma[2][n, 8, 8] as [n, y, x], and the magnitudes"""
    n = rec.shape[0]
    kind = rec[:, 0]
    qp = rec[:, 1].astype(np.int64)
    coef = np.ascontiguousarray(rec[:, 32:]).view(np.int16).astype(np.int64)
    if p.flags & SCALING:
        w4 = np.frombuffer(bytes(p.scaling4), np.uint8).astype(np.int64).reshape(3, 4, 4)
        w8 = np.frombuffer(bytes(p.scaling8), np.uint8).astype(np.int64).reshape(8, 8)
    else:
        w4 = np.full((3, 4, 4), 16, np.int64)
        w8 = np.full((8, 8), 16, np.int64)
    ls4 = w4[:, None] * _NA4[None]              # [plane, m, i, j]
    ls8 = w8[None] * _NA8                       # [m, i, j]
    trk = _Track(n)
    r_luma = np.zeros((n, 16, 16), np.int64)
    defect = np.zeros(n, bool)

    def luma4(sel, wrap):
        idx = np.nonzero(sel)[0]
        if idx.size == 0:
            return
        q = qp[idx]
        c = coef[idx, :256].reshape(-1, 16, 4, 4).copy()
        ls = ls4[0][q % 6][:, None]             # [n, 1, i, j]
        is16 = kind[idx] == I16x16
        # 8.5.10: c = the 4x4 matrix of DC levels; the level of the block at raster position (i, j) sits in slot 0 of that
        # block (minivideo_hotpath.h), blocks in luma4x4BlkIdx order; it is no coefficient of the block's own scaling (8.5.2)
        cdc = np.zeros((idx.size, 4, 4), np.int64)
        for b, (x, y) in enumerate(_BLK4):
            cdc[:, y // 4, x // 4] = c[:, b, 0, 0]
        c[is16, :, 0, 0] = 0
        d = _scale(c, ls, q, 4, trk, idx, wrap)
        if is16.any():
            f = wrap(np.matmul(np.matmul(_H4, cdc), _H4))
            ls00 = ls4[0][q % 6, 0, 0][:, None, None]
            prod = wrap(f * ls00)
            s = (q // 6)[:, None, None]
            up = np.maximum(s - 6, 0)
            down = np.maximum(6 - s, 0)
            left = wrap(prod << up)
            rnd = np.int64(1) << np.maximum(down - 1, 0)
            summed = wrap(prod + rnd)
            dc = np.where(q[:, None, None] >= 36, left, summed >> down)
            bad = q == 36 if luma_dc_from == 37 else np.zeros(q.shape, bool)
            if wrap is _w32:
                # the reference at QP'Y 36: (f * LevelScale + (1 << (-1 & 31))) >> (0 & 31) in 32-bit two's complement
                dc = np.where(bad[:, None, None], _w32(prod + (1 << 31)), dc)
            trk.see("scaled", f, idx)
            trk.see("product", prod, idx)
            trk.see("product", np.where(q[:, None, None] >= 36, left, summed), idx)
            trk.see("scaled", dc, idx)
            for b, (x, y) in enumerate(_BLK4):
                d[:, b, 0, 0] = np.where(is16, dc[:, y // 4, x // 4], d[:, b, 0, 0])
        trk.see("scaled", d, idx)
        see = lambda v: trk.see("transform", v, idx)
        f = _t4(d, see, wrap)                                               # rows: along j
        h = np.swapaxes(_t4(np.swapaxes(f, -1, -2), see, wrap), -1, -2)     # columns: along i
        pre = wrap(h + 32)
        trk.see("preshift", pre, idx)
        r = pre >> 6
        for b, (x, y) in enumerate(_BLK4):
            r_luma[idx, y:y + 4, x:x + 4] = r[:, b]

    if luma_dc_from not in (36, 37):
        raise SpecModelError("luma_dc_from is 36 (the standard) or 37 (the reference's defect)")
    not8 = (kind == I4x4) | (kind == I16x16)
    if luma_dc_from == 37:
        defect = (kind == I16x16) & (qp == 36)
    luma4(not8 & ~defect, _ident)
    luma4(defect, _w32)

    idx = np.nonzero(kind == I8x8)[0]
    if idx.size:
        q = qp[idx]
        c = coef[idx, :256].reshape(-1, 4, 8, 8)
        d = _scale(c, ls8[q % 6][:, None], q, 6, trk, idx)
        trk.see("scaled", d, idx)
        see = lambda v: trk.see("transform", v, idx)
        g = _t8(d, see)
        m = np.swapaxes(_t8(np.swapaxes(g, -1, -2), see), -1, -2)
        pre = m + 32
        trk.see("preshift", pre, idx)
        r = pre >> 6
        for b in range(4):
            x, y = 8 * (b % 2), 8 * (b // 2)
            r_luma[idx, y:y + 8, x:x + 8] = r[:, b]

    r_chroma = []
    idx = np.nonzero(kind != IPCM)[0]
    for pl in (0, 1):
        rc = np.zeros((n, 8, 8), np.int64)
        if idx.size:
            off = int(p.chroma_qp_index_offset if pl == 0 else p.second_chroma_qp_index_offset)
            qpi = np.clip(qp[idx] + off, 0, 51)                            # 8.5.8 (8-bit: QpBdOffsetC = 0)
            q = np.array(_QPC, np.int64)[qpi]
            c = coef[idx, 256 + 64 * pl:320 + 64 * pl].reshape(-1, 4, 4, 4).copy()
            ls = ls4[1 + pl][q % 6]
            cdc = c[:, :, 0, 0].reshape(-1, 2, 2).copy()                   # 8.5.11.1: c = [[DC0, DC1], [DC2, DC3]]
            c[:, :, 0, 0] = 0
            d = _scale(c, ls[:, None], q, 4, trk, idx)
            f = np.matmul(np.matmul(_A2, cdc), _A2)
            prod = f * ls[:, 0, 0][:, None, None]
            shifted = prod << (q // 6)[:, None, None]
            dcc = shifted >> 5                                             # 8.5.11.2
            trk.see("scaled", f, idx)
            trk.see("product", prod, idx)
            trk.see("product", shifted, idx)
            trk.see("scaled", dcc, idx)
            d[:, :, 0, 0] = dcc.reshape(-1, 4)
            trk.see("scaled", d, idx)
            see = lambda v: trk.see("transform", v, idx)
            f = _t4(d, see)
            h = np.swapaxes(_t4(np.swapaxes(f, -1, -2), see), -1, -2)
            pre = h + 32
            trk.see("preshift", pre, idx)
            r = pre >> 6
            for b in range(4):
                x, y = 4 * (b % 2), 4 * (b // 2)
                rc[idx, y:y + 4, x:x + 4] = r[:, b]
        r_chroma.append(rc)
    return r_luma, r_chroma, trk, defect


# ---- prediction: the standard's equations over p[(x, y)] -------------------------------------------------------------------
class _P(dict):
    def __missing__(self, key):
        raise SpecModelError("prediction reads p[%d, %d], which is not available" % key)


def _all(p, keys):
    for k in keys:
        if k not in p:
            return False
    return True


def _pred4x4(mode, p):
    """8.3.1.2.1 - 8.3.1.2.9 -> pred[y][x]"""
    R = range(4)
    if mode == 0:
        return [[p[x, -1] for x in R] for y in R]
    if mode == 1:
        return [[p[-1, y] for x in R] for y in R]
    if mode == 2:
        top, left = _all(p, [(x, -1) for x in R]), _all(p, [(-1, y) for y in R])
        if top and left:
            v = (sum(p[x, -1] for x in R) + sum(p[-1, y] for y in R) + 4) >> 3
        elif left:
            v = (sum(p[-1, y] for y in R) + 2) >> 2
        elif top:
            v = (sum(p[x, -1] for x in R) + 2) >> 2
        else:
            v = 128
        return [[v] * 4 for y in R]
    if mode == 3:
        return [[(p[6, -1] + 3 * p[7, -1] + 2) >> 2 if x == 3 and y == 3 else
                 (p[x + y, -1] + 2 * p[x + y + 1, -1] + p[x + y + 2, -1] + 2) >> 2 for x in R] for y in R]
    if mode == 4:
        return [[(p[x - y - 2, -1] + 2 * p[x - y - 1, -1] + p[x - y, -1] + 2) >> 2 if x > y else
                 (p[-1, y - x - 2] + 2 * p[-1, y - x - 1] + p[-1, y - x] + 2) >> 2 if x < y else
                 (p[0, -1] + 2 * p[-1, -1] + p[-1, 0] + 2) >> 2 for x in R] for y in R]
    if mode == 5:
        def vr(x, y):
            z = 2 * x - y
            if z in (0, 2, 4, 6):
                return (p[x - (y >> 1) - 1, -1] + p[x - (y >> 1), -1] + 1) >> 1
            if z in (1, 3, 5):
                return (p[x - (y >> 1) - 2, -1] + 2 * p[x - (y >> 1) - 1, -1] + p[x - (y >> 1), -1] + 2) >> 2
            if z == -1:
                return (p[-1, 0] + 2 * p[-1, -1] + p[0, -1] + 2) >> 2
            return (p[-1, y - 1] + 2 * p[-1, y - 2] + p[-1, y - 3] + 2) >> 2
        return [[vr(x, y) for x in R] for y in R]
    if mode == 6:
        def hd(x, y):
            z = 2 * y - x
            if z in (0, 2, 4, 6):
                return (p[-1, y - (x >> 1) - 1] + p[-1, y - (x >> 1)] + 1) >> 1
            if z in (1, 3, 5):
                return (p[-1, y - (x >> 1) - 2] + 2 * p[-1, y - (x >> 1) - 1] + p[-1, y - (x >> 1)] + 2) >> 2
            if z == -1:
                return (p[-1, 0] + 2 * p[-1, -1] + p[0, -1] + 2) >> 2
            return (p[x - 1, -1] + 2 * p[x - 2, -1] + p[x - 3, -1] + 2) >> 2
        return [[hd(x, y) for x in R] for y in R]
    if mode == 7:
        return [[(p[x + (y >> 1), -1] + p[x + (y >> 1) + 1, -1] + 1) >> 1 if y % 2 == 0 else
                 (p[x + (y >> 1), -1] + 2 * p[x + (y >> 1) + 1, -1] + p[x + (y >> 1) + 2, -1] + 2) >> 2
                 for x in R] for y in R]
    if mode == 8:
        def hu(x, y):
            z = x + 2 * y
            if z in (0, 2, 4):
                return (p[-1, y + (x >> 1)] + p[-1, y + (x >> 1) + 1] + 1) >> 1
            if z in (1, 3):
                return (p[-1, y + (x >> 1)] + 2 * p[-1, y + (x >> 1) + 1] + p[-1, y + (x >> 1) + 2] + 2) >> 2
            if z == 5:
                return (p[-1, 2] + 3 * p[-1, 3] + 2) >> 2
            return p[-1, 3]
        return [[hu(x, y) for x in R] for y in R]
    raise SpecModelError("Intra4x4PredMode %d" % mode)


def _filter8x8(p):
    """8.3.2.2.1: p -> p' (the samples that are available stay available)"""
    q = _P()
    if _all(p, [(x, -1) for x in range(8)]):        # (p[8..15, -1] are available then: substitution, 8.3.2.2)
        if (-1, -1) in p:
            q[0, -1] = (p[-1, -1] + 2 * p[0, -1] + p[1, -1] + 2) >> 2
        else:
            q[0, -1] = (3 * p[0, -1] + p[1, -1] + 2) >> 2
        for x in range(1, 15):
            q[x, -1] = (p[x - 1, -1] + 2 * p[x, -1] + p[x + 1, -1] + 2) >> 2
        q[15, -1] = (p[14, -1] + 3 * p[15, -1] + 2) >> 2
    if (-1, -1) in p:
        if (0, -1) not in p or (-1, 0) not in p:
            if (0, -1) in p:
                q[-1, -1] = (3 * p[-1, -1] + p[0, -1] + 2) >> 2
            elif (-1, 0) in p:
                q[-1, -1] = (3 * p[-1, -1] + p[-1, 0] + 2) >> 2
            else:
                q[-1, -1] = p[-1, -1]
        else:
            q[-1, -1] = (p[0, -1] + 2 * p[-1, -1] + p[-1, 0] + 2) >> 2
    if _all(p, [(-1, y) for y in range(8)]):
        if (-1, -1) in p:
            q[-1, 0] = (p[-1, -1] + 2 * p[-1, 0] + p[-1, 1] + 2) >> 2
        else:
            q[-1, 0] = (3 * p[-1, 0] + p[-1, 1] + 2) >> 2
        for y in range(1, 7):
            q[-1, y] = (p[-1, y - 1] + 2 * p[-1, y] + p[-1, y + 1] + 2) >> 2
        q[-1, 7] = (p[-1, 6] + 3 * p[-1, 7] + 2) >> 2
    return q


def _pred8x8(mode, p):
    """8.3.2.2.2 - 8.3.2.2.10 on the filtered samples p' -> pred[y][x]"""
    R = range(8)
    if mode == 0:
        return [[p[x, -1] for x in R] for y in R]
    if mode == 1:
        return [[p[-1, y] for x in R] for y in R]
    if mode == 2:
        top, left = _all(p, [(x, -1) for x in R]), _all(p, [(-1, y) for y in R])
        if top and left:
            v = (sum(p[x, -1] for x in R) + sum(p[-1, y] for y in R) + 8) >> 4
        elif left:
            v = (sum(p[-1, y] for y in R) + 4) >> 3
        elif top:
            v = (sum(p[x, -1] for x in R) + 4) >> 3
        else:
            v = 128
        return [[v] * 8 for y in R]
    if mode == 3:
        return [[(p[14, -1] + 3 * p[15, -1] + 2) >> 2 if x == 7 and y == 7 else
                 (p[x + y, -1] + 2 * p[x + y + 1, -1] + p[x + y + 2, -1] + 2) >> 2 for x in R] for y in R]
    if mode == 4:
        return [[(p[x - y - 2, -1] + 2 * p[x - y - 1, -1] + p[x - y, -1] + 2) >> 2 if x > y else
                 (p[-1, y - x - 2] + 2 * p[-1, y - x - 1] + p[-1, y - x] + 2) >> 2 if x < y else
                 (p[0, -1] + 2 * p[-1, -1] + p[-1, 0] + 2) >> 2 for x in R] for y in R]
    if mode == 5:
        def vr(x, y):
            z = 2 * x - y
            if z >= 0 and z % 2 == 0:
                return (p[x - (y >> 1) - 1, -1] + p[x - (y >> 1), -1] + 1) >> 1
            if z > 0:
                return (p[x - (y >> 1) - 2, -1] + 2 * p[x - (y >> 1) - 1, -1] + p[x - (y >> 1), -1] + 2) >> 2
            if z == -1:
                return (p[-1, 0] + 2 * p[-1, -1] + p[0, -1] + 2) >> 2
            return (p[-1, y - 2 * x - 1] + 2 * p[-1, y - 2 * x - 2] + p[-1, y - 2 * x - 3] + 2) >> 2
        return [[vr(x, y) for x in R] for y in R]
    if mode == 6:
        def hd(x, y):
            z = 2 * y - x
            if z >= 0 and z % 2 == 0:
                return (p[-1, y - (x >> 1) - 1] + p[-1, y - (x >> 1)] + 1) >> 1
            if z > 0:
                return (p[-1, y - (x >> 1) - 2] + 2 * p[-1, y - (x >> 1) - 1] + p[-1, y - (x >> 1)] + 2) >> 2
            if z == -1:
                return (p[-1, 0] + 2 * p[-1, -1] + p[0, -1] + 2) >> 2
            return (p[x - 2 * y - 1, -1] + 2 * p[x - 2 * y - 2, -1] + p[x - 2 * y - 3, -1] + 2) >> 2
        return [[hd(x, y) for x in R] for y in R]
    if mode == 7:
        return [[(p[x + (y >> 1), -1] + p[x + (y >> 1) + 1, -1] + 1) >> 1 if y % 2 == 0 else
                 (p[x + (y >> 1), -1] + 2 * p[x + (y >> 1) + 1, -1] + p[x + (y >> 1) + 2, -1] + 2) >> 2
                 for x in R] for y in R]
    if mode == 8:
        def hu(x, y):
            z = x + 2 * y
            if z < 13 and z % 2 == 0:
                return (p[-1, y + (x >> 1)] + p[-1, y + (x >> 1) + 1] + 1) >> 1
            if z < 13:
                return (p[-1, y + (x >> 1)] + 2 * p[-1, y + (x >> 1) + 1] + p[-1, y + (x >> 1) + 2] + 2) >> 2
            if z == 13:
                return (p[-1, 6] + 3 * p[-1, 7] + 2) >> 2
            return p[-1, 7]
        return [[hu(x, y) for x in R] for y in R]
    raise SpecModelError("Intra8x8PredMode %d" % mode)


def _clip1(v):
    return 0 if v < 0 else (255 if v > 255 else v)


def _pred16x16(mode, p):
    """8.3.3.1 - 8.3.3.4 -> pred[y][x]"""
    R = range(16)
    if mode == 0:
        return [[p[x, -1] for x in R] for y in R]
    if mode == 1:
        return [[p[-1, y] for x in R] for y in R]
    if mode == 2:
        top, left = _all(p, [(x, -1) for x in R]), _all(p, [(-1, y) for y in R])
        if top and left:
            v = (sum(p[x, -1] for x in R) + sum(p[-1, y] for y in R) + 16) >> 5
        elif left:
            v = (sum(p[-1, y] for y in R) + 8) >> 4
        elif top:
            v = (sum(p[x, -1] for x in R) + 8) >> 4
        else:
            v = 128
        return [[v] * 16 for y in R]
    if mode == 3:
        H = sum((k + 1) * (p[8 + k, -1] - p[6 - k, -1]) for k in range(8))
        V = sum((k + 1) * (p[-1, 8 + k] - p[-1, 6 - k]) for k in range(8))
        a = 16 * (p[-1, 15] + p[15, -1])
        b = (5 * H + 32) >> 6
        c = (5 * V + 32) >> 6
        return [[_clip1((a + b * (x - 7) + c * (y - 7) + 16) >> 5) for x in R] for y in R]
    raise SpecModelError("Intra16x16PredMode %d" % mode)


def _pred_chroma(mode, p):
    """8.3.4.1 - 8.3.4.4 for 4:2:0 (MbWidthC = MbHeightC = 8, xCF = yCF = 0) -> pred[y][x]"""
    R = range(8)
    if mode == 0:
        out = [[0] * 8 for y in R]
        for blk in range(4):
            xO, yO = 4 * (blk % 2), 4 * (blk // 2)
            tk, lk = [(xO + k, -1) for k in range(4)], [(-1, yO + k) for k in range(4)]
            top, left = _all(p, tk), _all(p, lk)
            st = sum(p[k] for k in tk) if top else 0
            sl = sum(p[k] for k in lk) if left else 0
            if (xO, yO) == (0, 0) or (xO > 0 and yO > 0):
                v = (st + sl + 4) >> 3 if top and left else (sl + 2) >> 2 if left else (st + 2) >> 2 if top else 128
            elif xO > 0 and yO == 0:
                v = (st + 2) >> 2 if top else (sl + 2) >> 2 if left else 128
            else:
                v = (sl + 2) >> 2 if left else (st + 2) >> 2 if top else 128
            for y in range(4):
                for x in range(4):
                    out[yO + y][xO + x] = v
        return out
    if mode == 1:
        return [[p[-1, y] for x in R] for y in R]
    if mode == 2:
        return [[p[x, -1] for x in R] for y in R]
    if mode == 3:
        H = sum((k + 1) * (p[4 + k, -1] - p[2 - k, -1]) for k in range(4))
        V = sum((k + 1) * (p[-1, 4 + k] - p[-1, 2 - k]) for k in range(4))
        a = 16 * (p[-1, 7] + p[7, -1])
        b = (34 * H + 32) >> 6
        c = (34 * V + 32) >> 6
        return [[_clip1((a + b * (x - 3) + c * (y - 3) + 16) >> 5) for x in R] for y in R]
    raise SpecModelError("intra_chroma_pred_mode %d" % mode)


class Result:
    """yuv: planar Y | Cb | Cr (uint8); cls[n]: CONFORMANT / INT32_SAFE / BEYOND per macroblock; defect[n]: macroblocks
    reconstructed under the luma_dc_from = 37 switch; scaled / transform / preshift / product [n]: largest magnitude per stage
    (mag(v) = max(v, -v - 1))"""

    def __init__(self, yuv, trk, defect):
        self.yuv = yuv
        self.defect = defect
        self.scaled, self.transform, self.preshift, self.product = trk.scaled, trk.transform, trk.preshift, trk.product
        conf = np.maximum(trk.scaled, trk.transform)
        every = np.maximum(np.maximum(conf, trk.preshift), trk.product)
        self.cls = np.where(every > LIM32, BEYOND, np.where(conf > LIM16, INT32_SAFE, CONFORMANT)).astype(np.uint8)

    def maxima(self):
        return {k: int(getattr(self, k).max()) if getattr(self, k).size else 0
                for k in ("scaled", "transform", "preshift", "product")}


def classify(params, records, luma_dc_from=36):
    """the residual stage alone: Result without a picture (yuv = None)"""
    rec = np.ascontiguousarray(records, np.uint8).reshape(-1, 800)
    _, _, trk, defect = _residuals(params, rec, luma_dc_from)
    return Result(None, trk, defect)


def dc_from(params):
    """the luma_dc_from that states what a set of parameters asks for: 36 with MVHP_PARAM_SPEC_LUMA_DC, else the reference's 37"""
    return 36 if params.flags & SPEC_LUMA_DC else 37


def reconstruct(params, records, luma_dc_from=36):
    """one picture: mvhp_stream_params_t (any object with its fields) + records[W * H, 800] -> Result"""
    W, H = int(params.width_mbs), int(params.height_mbs)
    rec = np.ascontiguousarray(records, np.uint8).reshape(-1, 800)
    if rec.shape[0] != W * H:
        raise SpecModelError("%d records for %d x %d macroblocks" % (rec.shape[0], W, H))
    r_luma, r_chroma, trk, defect = _residuals(params, rec, luma_dc_from)
    use_slices = bool(params.flags & SLICES)
    planes = [[bytearray(16 * W) for _ in range(16 * H)],
              [bytearray(8 * W) for _ in range(8 * H)], [bytearray(8 * W) for _ in range(8 * H)]]
    rl = r_luma.tolist()
    rcs = [r.tolist() for r in r_chroma]
    hdr = rec[:, :32].tolist()

    for addr in range(W * H):
        h = hdr[addr]
        kind, cmode, i16mode = h[0], h[3], h[4]
        un = h[6] if use_slices else 0
        modes = h[12:28]
        mbx, mby = addr % W, addr // W
        # 6.4.8 + 6.4.12 (Table 6-3, frame macroblocks): mbAddrA = CurrMbAddr - 1, B = - W, C = - W + 1, D = - W - 1, each
        # available when it is in the picture, not beyond a picture edge, and in the slice of the current macroblock
        avail = {"A": mbx > 0 and not un & UNAVAIL_A,
                 "B": mby > 0 and not un & UNAVAIL_B,
                 "C": mby > 0 and mbx < W - 1 and not un & UNAVAIL_C,
                 "D": mby > 0 and mbx > 0 and not un & UNAVAIL_D}

        def neighbours(plane, size, xO, yO, locs, skip=None):
            """p[(x, y)] of the available ones among the locations `locs`, relative to the block at (xO, yO) of the current
            macroblock of `size` samples (6.4.12: which macroblock covers (xN, yN), Table 6-3)"""
            p = _P()
            X0, Y0 = mbx * size, mby * size
            for (x, y) in locs:
                xN, yN = xO + x, yO + y
                if yN > size - 1:
                    continue
                if xN < 0:
                    who = "D" if yN < 0 else "A"
                elif xN <= size - 1:
                    who = "B" if yN < 0 else "cur"
                else:
                    who = "C" if yN < 0 else None     # right of the macroblock: later in decoding order
                if who is None or (who != "cur" and not avail[who]):
                    continue
                if skip is not None and skip(x, y):
                    continue
                p[x, y] = plane[Y0 + yN][X0 + xN]
            return p

        def put(plane, size, xO, yO, pred, res, n):
            X0, Y0 = mbx * size + xO, mby * size + yO
            for i in range(n):
                row = plane[Y0 + i]
                pr, rr = pred[i], res[yO + i]
                for j in range(n):
                    row[X0 + j] = _clip1(pr[j] + rr[xO + j])                  # 8.5.14: u_ij = Clip1(pred[xO + j, yO + i] + r_ij)

        if kind == IPCM:
            # 8.3.5: the samples are the picture; their arrangement in the record is defined in minivideo_hotpath.h
            area = rec[addr, 32:]
            for j in range(8):
                planes[0][16 * mby + 2 * j][16 * mbx:16 * mbx + 16] = area[64 * j:64 * j + 16].tobytes()
                planes[0][16 * mby + 2 * j + 1][16 * mbx:16 * mbx + 16] = area[64 * j + 16:64 * j + 32].tobytes()
                planes[1][8 * mby + j][8 * mbx:8 * mbx + 8] = area[64 * j + 32:64 * j + 40].tobytes()
                planes[2][8 * mby + j][8 * mbx:8 * mbx + 8] = area[64 * j + 40:64 * j + 48].tobytes()
            continue
        if kind == I4x4:
            locs = [(-1, y) for y in range(-1, 4)] + [(x, -1) for x in range(8)]
            for b, (xO, yO) in enumerate(_BLK4):
                skip = (lambda x, y: x > 3) if b in (3, 11) else None          # 8.3.1.2: not available for these two blocks
                p = neighbours(planes[0], 16, xO, yO, locs, skip)
                if _all(p, [(x, -1) for x in range(4)]) and not _all(p, [(x, -1) for x in range(4, 8)]):
                    for x in range(4, 8):
                        p[x, -1] = p[3, -1]
                put(planes[0], 16, xO, yO, _pred4x4(modes[b], p), rl[addr], 4)
        elif kind == I8x8:
            locs = [(-1, y) for y in range(-1, 8)] + [(x, -1) for x in range(16)]
            for b in range(4):
                xO, yO = 8 * (b % 2), 8 * (b // 2)
                p = neighbours(planes[0], 16, xO, yO, locs)
                if _all(p, [(x, -1) for x in range(8)]) and not _all(p, [(x, -1) for x in range(8, 16)]):
                    for x in range(8, 16):
                        p[x, -1] = p[7, -1]
                put(planes[0], 16, xO, yO, _pred8x8(modes[b], _filter8x8(p)), rl[addr], 8)
        elif kind == I16x16:
            locs = [(-1, y) for y in range(-1, 16)] + [(x, -1) for x in range(16)]
            p = neighbours(planes[0], 16, 0, 0, locs)
            put(planes[0], 16, 0, 0, _pred16x16(i16mode, p), rl[addr], 16)
        else:
            raise SpecModelError("macroblock %d: kind %d" % (addr, kind))
        locs = [(-1, y) for y in range(-1, 8)] + [(x, -1) for x in range(8)]
        for pl in (0, 1):
            p = neighbours(planes[1 + pl], 8, 0, 0, locs)
            put(planes[1 + pl], 8, 0, 0, _pred_chroma(cmode, p), rcs[pl][addr], 8)

    yuv = np.frombuffer(b"".join(b"".join(bytes(r) for r in pl) for pl in planes), np.uint8)
    return Result(yuv, trk, defect)
