"""Spec-mode records without a bitstream (TEST INFRASTRUCTURE): pictures of several slices, scaling matrices, I_PCM macroblocks
and large levels in the layout of include/minivideo_hotpath.h, for tests/test_spec_model.py and tests/test_gpu_spec_model.py.

minivideo_amd/synth.py supplies kinds, QP and levels; everything that depends on slices is drawn here: a slice id per macroblock,
the `unavail` bits as "the neighbour exists and has another id" (6.4.8), and prediction modes that are legal under THAT
availability -- Intra16x16 / chroma plane prediction and the diagonal modes of the first block need mbAddrD as well, which can lie
in another slice while A and B do not.  Levels are sized with the model's classification (tests/spec_model.py), never by guess:
  "conformant"  every macroblock CONFORMANT: levels of a macroblock that is not are halved until it is;
  "int32"       levels blown up, then halved while a macroblock is BEYOND; what remains is INT32_SAFE or CONFORMANT.
Nothing BEYOND is ever produced: that region is signed-overflow territory for a C implementation."""
import ctypes as C

import numpy as np

from minivideo_amd.hotpath import StreamParams
from minivideo_amd.synth import synth_packed
from tests import spec_model as M

SLICE_MAPS = ("one", "per_row", "per_mb", "mid_row", "band_rows", "band_mid", "random", "dispersed")
_BLK4 = [(8 * ((b // 4) % 2) + 4 * ((b % 4) % 2), 8 * ((b // 4) // 2) + 4 * ((b % 4) // 2)) for b in range(16)]


def _from_starts(n, starts):
    ids = np.zeros(n, np.int32)
    for s in sorted({int(s) for s in starts if 0 < s < n}):
        ids[s:] += 1
    return ids


def slice_map(kind, W, H, rng):
    """slice id per macroblock.  All kinds but "dispersed" are raster-contiguous runs (slices without FMO); "dispersed" gives
    the macroblock at (x, y) the id (x / 2 + y / 3) % 2 -- stripes two macroblocks wide that shift every three rows, as a slice-group
    map could: the one kind where mbAddrC can lie in another slice while mbAddrB does not.
    band_rows / band_mid: boundaries exactly at macroblock rows 4k - 1, 4k and 4k + 1 (the wide kernel forms work in bands of
    four rows), at the start of the row / in the middle of it."""
    n = W * H
    if kind == "one":
        return np.zeros(n, np.int32)
    if kind == "per_row":
        return _from_starts(n, [y * W for y in range(H)])
    if kind == "per_mb":
        return np.arange(n, dtype=np.int32)
    if kind == "mid_row":
        return _from_starts(n, [y * W + int(rng.integers(1, W)) for y in range(H)] if W > 1 else range(0, n, 2))
    if kind in ("band_rows", "band_mid"):
        rows = [r for k in range(0, H + 4, 4) for r in (k - 1, k, k + 1) if 0 < r < H] or list(range(1, H))
        if kind == "band_rows" or W == 1:
            return _from_starts(n, [r * W for r in rows])
        return _from_starts(n, [r * W + int(rng.integers(1, W)) for r in rows])
    if kind == "random":
        k = int(rng.integers(1, max(2, n // 3) + 1))
        return _from_starts(n, rng.integers(1, max(2, n), size=k))
    if kind == "dispersed":
        x, y = np.arange(n) % W, np.arange(n) // W
        return ((x // 2 + y // 3) % 2).astype(np.int32)
    raise ValueError(kind)


def neighbour_flags(ids, W, H):
    """(exists[4], other[4]) for A, B, C, D: the neighbour lies in the picture / exists and has another slice id"""
    ids = np.asarray(ids).reshape(H, W)
    x = np.arange(W)[None, :].repeat(H, 0)
    y = np.arange(H)[:, None].repeat(W, 1)
    ex, other = [], []
    for dx, dy in ((-1, 0), (0, -1), (1, -1), (-1, -1)):
        e = (x + dx >= 0) & (x + dx < W) & (y + dy >= 0)
        nid = ids[np.clip(y + dy, 0, H - 1), np.clip(x + dx, 0, W - 1)]
        ex.append(e.reshape(-1))
        other.append((e & (nid != ids)).reshape(-1))
    return ex, other


def unavail_bits(ids, W, H):
    _, other = neighbour_flags(ids, W, H)
    return (other[0] * 1 + other[1] * 2 + other[2] * 4 + other[3] * 8).astype(np.uint8)


def _choose(rng, allowed):
    score = np.where(allowed, rng.random(allowed.shape), -1.0)
    return score.argmax(-1).astype(np.uint8)


def _nxn(rng, A, B, D, size):
    """modes of the 16 / size^2 ... blocks of `size` samples, legal under availability A, B, D (bool per macroblock)"""
    blocks = _BLK4 if size == 4 else [(8 * (b % 2), 8 * (b // 2)) for b in range(4)]
    out = np.zeros(A.shape + (len(blocks),), np.uint8)
    for b, (xO, yO) in enumerate(blocks):
        left = A | (xO > 0)
        up = B | (yO > 0)
        corner = (np.ones_like(A) if yO > 0 else B) if xO > 0 else (A if yO > 0 else D)
        al = np.zeros(A.shape + (9,), bool)
        al[..., 2] = True
        for m in (0, 3, 7):          # (3 and 7 without an upper-right neighbour: p[3, -1] / p[7, -1] is substituted)
            al[..., m] = up
        for m in (1, 8):
            al[..., m] = left
        for m in (4, 5, 6):
            al[..., m] = left & up & corner
        out[..., b] = _choose(rng, al)
    return out


def set_slices(rec, W, H, ids, rng):
    """rec[N, 800] of one picture, in place: unavail bits of the slice map + prediction modes legal under it"""
    ex, other = neighbour_flags(ids, W, H)
    A, B, _, D = (e & ~o for e, o in zip(ex, other))
    kind = rec[:, 0]
    rec[:, 6] = unavail_bits(ids, W, H)
    p4, p8 = _nxn(rng, A, B, D, 4), _nxn(rng, A, B, D, 8)
    pred = np.zeros((rec.shape[0], 16), np.uint8)
    pred[kind == M.I4x4] = p4[kind == M.I4x4]
    pred[kind == M.I8x8, :4] = p8[kind == M.I8x8]
    rec[:, 12:28] = pred
    al = np.zeros(A.shape + (4,), bool)
    al[..., 2], al[..., 0], al[..., 1], al[..., 3] = True, B, A, A & B & D
    rec[:, 4] = np.where(kind == M.I16x16, _choose(rng, al), 0)
    al = np.zeros(A.shape + (4,), bool)
    al[..., 0], al[..., 1], al[..., 2], al[..., 3] = True, A, B, A & B & D
    rec[:, 3] = _choose(rng, al)


def set_pcm(rec, where, rng):
    """turn the macroblocks `where` (bool[N]) of one picture into I_PCM with random samples (layout: minivideo_hotpath.h)"""
    idx = np.nonzero(where)[0]
    for k in idx:
        un = rec[k, 6]
        rec[k] = 0
        rec[k, 0], rec[k, 6] = M.IPCM, un
        area = rec[k, 32:]
        smooth = rng.integers(0, 2)
        for j in range(8):
            if smooth:
                area[64 * j:64 * j + 48] = (rng.integers(0, 256) + np.arange(48) * rng.integers(-3, 4)) & 255
            else:
                area[64 * j:64 * j + 48] = rng.integers(0, 256, 48)


def pcm_positions(ids, W, H, share, rng):
    """random positions of about `share` of the macroblocks, plus -- so that every kind of neighbour predicts from PCM samples
    at a boundary -- the first and the last macroblock of some slices and of some rows"""
    n = W * H
    where = rng.random(n) < share
    if share > 0:
        ids = np.asarray(ids)
        first = np.nonzero(np.r_[True, ids[1:] != ids[:-1]])[0]
        last = np.nonzero(np.r_[ids[1:] != ids[:-1], True])[0]
        for group in (first, last, np.arange(H) * W, np.arange(H) * W + W - 1):
            pick = group[rng.random(group.size) < 0.3]
            where[pick] = True
    return where


def fix_nz_mask(rec):
    """nz_mask from the coefficient area (I_PCM: 0), as the front end writes it"""
    N = rec.shape[0]
    coef = np.ascontiguousarray(rec[:, 32:]).view(np.int16)
    blk = (coef.reshape(N, 24, 16) != 0).any(-1)
    luma = blk[:, :16].copy()
    g8 = luma.reshape(N, 4, 4).any(-1)
    luma = np.where((rec[:, 0] == M.I8x8)[:, None], np.repeat(g8, 4, axis=-1), luma)
    bits = np.concatenate([luma, blk[:, 16:]], axis=-1)
    mask = (bits.astype(np.uint32) << np.arange(24, dtype=np.uint32)).sum(-1).astype(np.uint32)
    mask[rec[:, 0] == M.IPCM] = 0
    rec[:, 8:12] = mask.view(np.uint8).reshape(N, 4)


def levels(rec):
    """the coefficient areas of rec[N, 800] (C-contiguous) as an int16 view [N, 384], in place"""
    assert rec.flags.c_contiguous and rec.dtype == np.uint8
    return rec.view(np.int16).reshape(-1, 400)[:, 16:]


def fit_levels(params, rec, regime, rng, luma_dc_from=36):
    """size the levels of one picture rec[N, 800] (in place) for `regime`; returns the model's classes"""
    not_pcm = rec[:, 0] != M.IPCM
    coef = levels(rec)
    if regime == "int32":
        big = rng.random(coef.shape) < 0.08
        grown = np.clip(coef.astype(np.int64) * rng.integers(200, 1200, coef.shape), -32768, 32767)
        fresh = rng.integers(-32768, 32768, coef.shape)
        val = np.where(coef != 0, grown, np.where(rng.random(coef.shape) < 0.02, fresh, 0))
        coef[not_pcm] = np.where(big, val, coef)[not_pcm].astype(np.int16)
        limit = M.INT32_SAFE
    elif regime == "conformant":
        limit = M.CONFORMANT
    else:
        raise ValueError(regime)
    for _ in range(20):
        res = M.classify(params, rec, luma_dc_from)
        cls = res.cls
        over = (cls > limit) & not_pcm & ~res.defect        # (a macroblock under the reference's defect has no regime)
        if not over.any():
            break
        c = coef[over].astype(np.int32)
        coef[over] = (np.sign(c) * (np.abs(c) >> 1)).astype(np.int16)
    else:
        raise AssertionError("levels do not settle")
    fix_nz_mask(rec)
    return cls


# ---- weight sets -------------------------------------------------------------------------------------------------------------
# Table 7-3 Default_4x4_Intra and Table 7-4 Default_8x8_Intra are given in zig-zag scan order; the matrices of
# mvhp_stream_params_t are raster, so they pass through the inverse zig-zag scan of 8.5.6 (Figure 8-8, frame scan)
_DEFAULT4_ZZ = (6, 13, 13, 20, 20, 20, 28, 28, 28, 28, 32, 32, 32, 37, 37, 42)
_DEFAULT8_ZZ = (6, 10, 10, 13, 11, 13, 16, 16, 16, 16, 18, 18, 18, 18, 18, 23, 23, 23, 23, 23, 23, 25, 25, 25, 25, 25, 25, 25,
                27, 27, 27, 27, 27, 27, 27, 27, 29, 29, 29, 29, 29, 29, 29, 31, 31, 31, 31, 31, 31, 33, 33, 33, 33, 33, 36, 36,
                36, 36, 38, 38, 38, 40, 40, 42)


def _zigzag(n):
    """raster index (i * n + j) of scan position k: anti-diagonals, alternating direction, starting to the right"""
    order = []
    for s in range(2 * n - 1):
        cells = [(i, s - i) for i in range(n) if 0 <= s - i < n]
        order += cells if s % 2 else cells[::-1]
    return [i * n + j for i, j in order]


def _raster(zz, n):
    out = np.zeros(n * n, np.uint8)
    out[_zigzag(n)] = zz
    return out


def weights(name, rng=None):
    """(w4[3, 16], w8[64]) uint8, raster"""
    if name == "flat16":
        return np.full((3, 16), 16, np.uint8), np.full(64, 16, np.uint8)
    if name == "all1":
        return np.ones((3, 16), np.uint8), np.ones(64, np.uint8)
    if name == "all255":
        return np.full((3, 16), 255, np.uint8), np.full(64, 255, np.uint8)
    if name == "random":
        return rng.integers(1, 256, (3, 16)).astype(np.uint8), rng.integers(1, 256, 64).astype(np.uint8)
    if name == "default_intra":
        return np.tile(_raster(_DEFAULT4_ZZ, 4), (3, 1)), _raster(_DEFAULT8_ZZ, 8)
    raise ValueError(name)


WEIGHT_SETS = ("flat16", "all1", "all255", "random", "default_intra")
ONE_HOT = [(lst, pos) for lst in range(3) for pos in range(16)] + [(3, pos) for pos in range(64)]     # 112 sets


def one_hot_weights(lst, pos, value):
    w4, w8 = weights("flat16")
    if lst < 3:
        w4[lst, pos] = value
    else:
        w8[pos] = value
    return w4, w8


def make_params(W, H, flags, cqp=(0, 0), w=None):
    p = StreamParams(W, H, int(cqp[0]), int(cqp[1]), int(flags))
    w4, w8 = w if w is not None else weights("flat16")
    C.memmove(C.byref(p, StreamParams.scaling4.offset), np.ascontiguousarray(w4, np.uint8).ctypes.data, 48)
    C.memmove(C.byref(p, StreamParams.scaling8.offset), np.ascontiguousarray(w8, np.uint8).ctypes.data, 64)
    return p


def spec_pictures(W, H, maps, seed, weight_set="flat16", pcm_share=0.0, regime="conformant", qp_range=(0, 51), cqp=(0, 0),
                  spec_luma_dc=True, profile="high", force_scaling=True, w=None):
    """len(maps) pictures of W x H macroblocks, picture k with slice map maps[k] (a SLICE_MAPS name or an id array):
    -> (params, rec[F, N, 800], ids[F, N], cls[F, N])"""
    rng = np.random.default_rng([seed, W, H])
    F = len(maps)
    base, rec = synth_packed(W, H, F, seed=seed, profile=profile, density="dense", qp_range=qp_range, cqp_offsets=cqp,
                             allow_qp36_i16=True)
    rec = np.ascontiguousarray(rec)
    flags = (base.flags & 1) | (2 if spec_luma_dc else 0)
    all_ids = [slice_map(m, W, H, rng) if isinstance(m, str) else np.asarray(m, np.int32) for m in maps]
    if any(ids.any() for ids in all_ids):
        flags |= M.SLICES
    if w is None:
        w = weights(weight_set, rng)
    if force_scaling or weight_set != "flat16":
        flags |= M.SCALING
    params = make_params(W, H, flags, cqp, w)
    cls = []
    for k in range(F):
        set_slices(rec[k], W, H, all_ids[k], rng)
        set_pcm(rec[k], pcm_positions(all_ids[k], W, H, pcm_share, rng), rng)
        cls.append(fit_levels(params, rec[k], regime, rng, M.dc_from(params)))
    return params, rec, np.stack(all_ids), np.stack(cls)


def one_hot_pictures(lst, pos, seed=0):
    """one 3 x 2 picture for the one-hot weight set (lst, pos): levels ONLY at the coefficient the changed weight scales and at
    its transposed position (two different values), in every block of every plane, so that a transposed weight matrix, a weight
    applied to another plane or list, and a raster / zig-zag mix-up all change samples.  QP'Y 24 .. 40: scaling is exact there."""
    W, H = 3, 2
    rng = np.random.default_rng([seed, lst, pos])
    base, rec = synth_packed(W, H, 1, seed=1000 + lst * 64 + pos, profile="high", density="dense", qp_range=(24, 40),
                             allow_qp36_i16=True, kinds=(0.34, 0.5) if lst != 3 else (0.0, 1.0))
    rec = np.ascontiguousarray(rec[0])
    n = 8 if lst == 3 else 4
    i, j = divmod(pos, n)
    coef = levels(rec)
    coef[:] = 0
    for mb in range(W * H):
        a, b = (int(v) for v in rng.choice([-7, -5, -4, -3, 3, 4, 5, 6, 7], 2, replace=False))
        if rec[mb, 0] == M.I8x8:
            i8, j8 = (i, j) if lst == 3 else (2 * i, 2 * j + 1)
            for blk in range(4):
                coef[mb, 64 * blk + 8 * i8 + j8] = a
                coef[mb, 64 * blk + 8 * j8 + i8] = b
        else:
            for blk in range(16):
                coef[mb, 16 * blk + 4 * (i % 4) + j % 4] = a
                coef[mb, 16 * blk + 4 * (j % 4) + i % 4] = b
        for pl in (0, 1):
            for blk in range(4):
                coef[mb, 256 + 64 * pl + 16 * blk + 4 * (i % 4) + j % 4] = a + pl
                coef[mb, 256 + 64 * pl + 16 * blk + 4 * (j % 4) + i % 4] = b - pl
    value = int(rng.choice([1, 5, 9, 23, 40, 77, 160, 255]))
    params = make_params(W, H, (base.flags & 1) | 2 | M.SCALING, (0, 0), one_hot_weights(lst, pos, value))
    set_slices(rec, W, H, np.zeros(W * H, np.int32), rng)
    cls = fit_levels(params, rec, "conformant", rng)
    return params, rec, cls


def extreme_pictures(W, H, qp, seed, weight_set="all255", maps=("one",)):
    """pictures in which every macroblock carries ONE level, at a random coefficient of a random plane, as large as the model still
    classes INT32_SAFE at QP'Y `qp` under `weight_set` (found by bisection on the level with the model's classification; a
    macroblock whose coefficient stays INT32_SAFE at 32767 keeps 32767): -> (params, rec[F, N, 800], cls[F, N])"""
    rng = np.random.default_rng([seed, qp])
    params, rec, ids, _ = spec_pictures(W, H, list(maps), seed=seed, weight_set=weight_set, qp_range=(qp, qp), cqp=(0, 0))
    out = []
    for k in range(rec.shape[0]):
        r = rec[k]
        coef = levels(r)
        coef[:] = 0
        n = r.shape[0]
        live = np.nonzero(r[:, 0] != M.IPCM)[0]
        slot = np.where(rng.random(n) < 0.6, rng.integers(0, 256, n), rng.integers(256, 384, n))
        sign = np.where(rng.random(n) < 0.5, -1, 1)
        lo, hi = np.zeros(n, np.int64), np.full(n, 32767, np.int64)
        while (lo < hi).any():
            mid = (lo + hi + 1) >> 1
            coef[live, slot[live]] = (sign * mid)[live].astype(np.int16)
            ok = M.classify(params, r).cls <= M.INT32_SAFE
            lo, hi = np.where(ok, mid, lo), np.where(ok, hi, mid - 1)
        coef[live, slot[live]] = (sign * lo)[live].astype(np.int16)
        fix_nz_mask(r)
        out.append(M.classify(params, r).cls)
    return params, rec, np.stack(out)
