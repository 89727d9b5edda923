"""The directed corpus (TEST INFRASTRUCTURE): record batches in the layout of include/minivideo_hotpath.h that are CONSTRUCTED, not
drawn, so that every cell of tests/recon_census.py's universe occurs.  Only the values of the levels and I_PCM samples are random.

Three families, each for the shapes SHAPES (1 x 1 ... 9 x 9: columns x % 4 = 0 .. 3 and the column after a whole strip, rows on both
sides of a four-row seam) or for WAVE_SHAPE:
  positional  60 pictures per shape in four batches of 15.  Macroblock (x, y) of picture k takes variant (k + 7 x + 13 y) % 60 of
              18 Intra4x4 (block b: mode (b + r) % 9, coded (b + c) % 2), 18 Intra8x8 and 24 Intra16x16 (mode x luma none / DC / AC x
              QP'Y 36 or not) variants -- a position of which a picture has ONE (a corner) still meets all 60 -- and chroma variant
              (k + 5 x + 3 y) % 12 (mode x none / DC / AC).  A mode the position cannot have becomes DC.  QP'Y walks 0 .. 51; the
              chroma offsets belong to the shape and include (-12, 12) and (12, -12).
  zero        parity only: the same walk with NOTHING made legal, two batches per shape (Intra4x4 + Intra16x16, Intra8x8 + Intra16x16):
              the "predict 0" path of test_unavailable_neighbour_modes_predict_zero, at every block and missing-neighbour pattern.
  wave        5 x 9 pictures, batches of 17 (two groups of eight and a last group of one; four groups of four and one) and of 15 (eight
              + seven; three fours + three), one per pair of chroma offsets.  Every (group, macroblock position) is given a TARGET: a
              wave condition with none / all / exactly picture i of the group satisfying it, or a combination of two ballots.  The
              targets are laid out for groups of eight; a group of four sees "one at i" as "one at i % 4" beside a group with none.
Settings: "parity" (flags 0 / MAY_HAVE_8X8, the QP'Y 36 defect present), "spec" (MVHP_PARAM_SPEC_LUMA_DC, the same records without the
zero family) and "spec_pcm" (the spec corpus plus wave batches whose targets are I_PCM counts).

Levels are sized by QP'Y so that every macroblock is CONFORMANT by tests/spec_model.classify (asserted, nothing is halved: a halved
level could un-code a block and silently change the cell); nz_mask comes from spec_synth.fix_nz_mask."""
import functools
from collections import namedtuple

import numpy as np

from minivideo_amd.hotpath import StreamParams
from tests import recon_census as RC
from tests import spec_model as M
from tests import spec_synth as S

I4, I8, I16, PCM = RC.I4, RC.I8, RC.I16, RC.PCM
SHAPES = ((1, 1), (1, 9), (9, 1), (2, 5), (5, 9), (9, 9))
OFFSETS = {(1, 1): (0, 0), (1, 9): (-12, 12), (9, 1): (12, -12), (2, 5): (3, -5), (5, 9): (-12, 12), (9, 9): (12, -12)}
WAVE_SHAPE = (5, 9)
WAVE_OFFSETS = ((-12, 12), (12, -12), (-12, -12), (12, 12))
WAVE_COUNTS = (17, 15)
SETTINGS = RC.MODES
# form -> (pictures one wavefront keeps in lock step, taken from the form's source: `frame_raw = blockIdx.x * 8 + o` in recon_oct.hip,
# `* 4 + q` in recon_quad.hip and recon_pipe.hip; 1: a macroblock pair, recon_kernels.hip / recon_pipe1.hip; the rows per band the
# banded forms are built for, as tests/test_gpu_extents.py BUILT has them, 0 = no bands)
FORMS = {"rows": (1, (0,)), "quad": (4, (0,)), "oct": (8, (0,)), "wide": (1, (4,)), "quad_wide": (4, (4, 8)), "pipe": (4, (1, 2, 4)),
         "pipe1": (1, (1, 2, 4))}
BANDED = ("wide", "quad_wide", "pipe", "pipe1")
Batch = namedtuple("Batch", "name family params rec")     # rec[n, W * H, 800]


def _params(W, H, cqp, setting, rec):
    flags = (1 if (rec[..., 0] == I8).any() else 0) | (0 if setting == "parity" else M.SPEC_LUMA_DC)
    return StreamParams(W, H, int(cqp[0]), int(cqp[1]), flags)


# ---- one macroblock ------------------------------------------------------------------------------------------------------------
def _levels(rng, qp, slots):
    """levels for the coefficient slots `slots`: a few, smaller as QP'Y grows (8.5.12.1 shifts left by qP / 6 - 4)"""
    top = 6 if qp < 20 else 3 if qp < 36 else 1
    mag = rng.integers(1, top + 1, len(slots))
    return (mag * rng.choice((-1, 1), len(slots))).astype(np.int16)


def make_mb(rng, kind, qp, modes=(2,) * 16, i16mode=2, cmode=0, luma=(), chroma=0):
    """one record.  luma: Intra4x4 / Intra8x8 the coded blocks; Intra16x16 0 none / 1 DC only / 2 DC + AC.  chroma: 0 / 1 DC / 2 AC"""
    r = np.zeros(800, np.uint8)
    c = np.zeros(384, np.int16)
    few = 3 if qp < 40 else 1
    cbp = 0
    if kind == I4:
        for b in luma:
            s = 16 * b + rng.choice(16, few, replace=False)
            c[s] = _levels(rng, qp, s)
            cbp |= 1 << (b // 4)
        r[12:28] = modes
    elif kind == I8:
        for b in luma:
            s = 64 * b + rng.choice(64, few, replace=False)
            c[s] = _levels(rng, qp, s)
            cbp |= 1 << b
        r[12:16] = modes[:4]
    elif kind == I16:
        if luma >= 1:
            s = 16 * rng.choice(16, few, replace=False)
            c[s] = _levels(rng, qp, s)
        if luma == 2:
            for b in rng.choice(16, 5, replace=False):
                s = 16 * b + 1 + rng.choice(15, 1)
                c[s] = _levels(rng, qp, s)
            cbp = 15
        r[4] = i16mode
    if chroma:
        for pl in ((0, 1) if rng.integers(0, 3) == 0 else (int(rng.integers(0, 2)),)):
            s = 256 + 64 * pl + 16 * rng.choice(4, 2, replace=False)
            c[s] = _levels(rng, qp, s)
            if chroma == 2:
                s = 256 + 64 * pl + 16 * rng.choice(4, 2, replace=False) + 1 + rng.choice(15, 2, replace=False)
                c[s] = _levels(rng, qp, s)
    r[0], r[1], r[2], r[3] = kind, qp, cbp | (chroma << 4), cmode
    r[32:] = c.view(np.uint8)
    return r


def _finish(W, H, cqp, setting, rec, name, family, pcm=None):
    rec = np.ascontiguousarray(rec)
    if pcm is not None:
        for k in range(rec.shape[0]):
            S.set_pcm(rec[k], pcm[k], np.random.default_rng([77, k, W, H]))
    for k in range(rec.shape[0]):
        S.fix_nz_mask(rec[k])
    p = _params(W, H, cqp, setting, rec)
    res = M.classify(p, rec.reshape(-1, 800), M.dc_from(p))
    bad = (res.cls != M.CONFORMANT) & ~res.defect & (rec.reshape(-1, 800)[:, 0] != PCM)
    assert not bad.any(), "%s: %d macroblocks are not conformant" % (name, int(bad.sum()))
    return Batch(name, family, p, rec)


def _legal_modes(size, x, y, modes):
    return [m if RC._legal(RC.NEEDS[m], RC.block_avail(size, b, x > 0, y > 0)) else 2 for b, m in enumerate(modes)]


# ---- positional and zero families -------------------------------------------------------------------------------------------
def _walk_qp(k, x, y):
    return (5 * k + 3 * x + 11 * y + 17 * (k // 13)) % 52


def _variant_mb(rng, v, cv, qp, x, y, legal):
    A, B = x > 0, y > 0
    cmode, chroma = cv % 4, cv // 4
    if legal and not RC._legal(RC.NEEDSC[cmode], (A, B)):
        cmode = 0
    if v < 36:
        size, kind, nb = (4, I4, 16) if v < 18 else (8, I8, 4)
        r, c = (v % 18) % 9, (v % 18) // 9
        modes = [(b + r) % 9 for b in range(nb)]
        if legal:
            modes = _legal_modes(size, x, y, modes)
        return make_mb(rng, kind, qp, modes + [0] * (16 - nb), cmode=cmode, luma=[b for b in range(nb) if (b + c) % 2], chroma=chroma)
    i = v - 36
    mode, lum, q36 = i % 4, (i // 4) % 3, i // 12
    if legal and not RC._legal(RC.NEEDS16[mode], (A, B)):
        mode = 2
    qp = 36 if q36 else (qp if qp != 36 else 37)
    return make_mb(rng, I16, qp, i16mode=mode, cmode=cmode, luma=lum, chroma=chroma)


@functools.lru_cache(maxsize=None)
def _positional_records(W, H):
    rng = np.random.default_rng([1, W, H])
    rec = np.zeros((60, W * H, 800), np.uint8)
    for k in range(60):
        for n in range(W * H):
            x, y = n % W, n // W
            rec[k, n] = _variant_mb(rng, (k + 7 * x + 13 * y) % 60, (k + 5 * x + 3 * y) % 12, _walk_qp(k, x, y), x, y, True)
    return rec


@functools.lru_cache(maxsize=None)
def _zero_records(W, H):
    """22 pictures: Intra4x4 walks 0 .. 8, Intra8x8 walks 0 .. 8, Intra16x16 modes 0 .. 3; chroma modes walk with the picture"""
    rng = np.random.default_rng([2, W, H])
    rec = np.zeros((22, W * H, 800), np.uint8)
    for k in range(22):
        for n in range(W * H):
            x, y = n % W, n // W
            s = k + x + y
            v = s % 9 if k < 9 else 18 + s % 9 if k < 18 else 36 + 4 * (s % 3) + (k - 18 + x + y) % 4
            rec[k, n] = _variant_mb(rng, v, 4 * (s % 3) + (k + x + 2 * y) % 4, 20 + (7 * s) % 21, x, y, False)
    return rec


# ---- wave family ---------------------------------------------------------------------------------------------------------------
def _qp_where(offs, want):
    """a QP'Y at which (luma, Cb, Cr below qP 24) = want for Intra4x4, the one closest to a threshold; None: no such QP'Y"""
    best = None
    for qp in range(52):
        got = (qp < 24,) + tuple(RC.QPC[min(max(qp + o, 0), 51)] < 24 for o in offs)
        if got == tuple(want):
            d = min([abs(qp - 23.5)] + [abs(RC.QPC[min(max(qp + o, 0), 51)] - 23.5) for o in offs])
            if best is None or d < best[0]:
                best = (d, qp)
    return None if best is None else best[1]


def _qp_plane(offs, pl, slow):
    """the QP'Y nearest the threshold at which plane pl's QPc is below 24 (slow) / not"""
    qps = [qp for qp in range(52) if (RC.QPC[min(max(qp + offs[pl], 0), 51)] < 24) == slow]
    return max(qps) if slow else min(qps)


def targets(L, offs, setting):
    """the targets of one group of L pictures: ("cond", name, pattern) with pattern "none" / "all" / index; ("anylc", l, c);
    ("slow3", l, cb, cr) where the offsets allow it.  The combination targets come first: every group of a batch gets them."""
    out = [("slow3",) + t for t in np.ndindex(2, 2, 2) if _qp_where(offs, t) is not None]
    out += [("anylc", a, c) for a in (0, 1) for c in (0, 1)]
    names = list(RC.WAVE_CONDS) + (["quirk_only"] if setting == "parity" else [])
    if setting == "spec_pcm":
        names = ["ipcm"]
    rest = [("cond", n, p) for n in names for p in ["none", "all"] + list(range(L))]
    return out, rest


def _realize(rng, t, L, x, y, offs):
    """the L records of one group at macroblock (x, y) for target t"""
    A, B = x > 0, y > 0
    every4, every8 = list(range(16)), list(range(4))
    nondc = 0 if B else 1 if A else None      # a legal Intra4x4 / Intra8x8 mode that is not DC: vertical, else horizontal

    def coded(qp, **kw):
        kw.setdefault("luma", every4[::2] + [15])
        kw.setdefault("chroma", 2)
        return make_mb(rng, kw.pop("kind", I4), qp, **kw)

    # the combination targets put what they need into BOTH halves of a group of eight, so that groups of four meet them too
    def halves(a, b):
        return {i for i in (a, 4 + b) if i < L} if L > 1 else {0}

    if t[0] == "slow3":
        fast = _qp_where(offs, (0, 0, 0))
        some = halves(int(rng.integers(0, 4)), int(rng.integers(0, 3)))
        return [coded(_qp_where(offs, t[1:]) if (i in some or fast is None) else fast) for i in range(L)]
    if t[0] == "anylc":
        lum = halves(0, 0) if t[1] else set()
        chr_ = halves(1, 1) if t[2] else set()
        return [make_mb(rng, I4, 26 + i, luma=every4[1::3] if i in lum else (), chroma=2 if i in chr_ else 0) for i in range(L)]
    name, pat = t[1], t[2]
    sat = set() if pat == "none" else set(range(L)) if pat == "all" else {pat}
    out = []
    for i in range(L):
        s = i in sat
        if name == "need_l":
            mb = make_mb(rng, I4, 28, luma=every4[i % 3::3] if s else (), chroma=0 if s else 2 * (i % 2))
        elif name == "need_c":
            mb = make_mb(rng, I4, 29, luma=() if s or i % 2 else every4[::5], chroma=(1 + i % 2) if s else 0)
        elif name == "luma_slow":
            mb = coded(23 if s else 24)
        elif name in ("cb_slow", "cr_slow"):
            mb = coded(_qp_plane(offs, name == "cr_slow", s))
        elif name == "chroma_plane":
            mb = coded(27, cmode=3 if s and A and B else i % 3 if A and B else 0)
        elif name == "i16_plane":
            mb = coded(31, kind=I16, i16mode=3 if s and A and B else 2, luma=i % 3)
        elif name == "i4_dc":
            mb = coded(25, modes=(2,) * 16) if s else coded(25, modes=(nondc,) * 16) if nondc is not None else \
                coded(25, kind=I16, luma=1)
        elif name == "i8_dc":
            mb = coded(33, kind=I8, modes=(2,) * 16, luma=every8[i % 2::2]) if s else \
                coded(33, kind=I8, modes=(nondc,) * 16, luma=every8) if nondc is not None else coded(33)
        elif name == "quirk_only":
            mb = make_mb(rng, I16, 36 if s else 37, luma=0, chroma=2 * (i % 2))
        elif name == "ipcm":
            mb = coded(30 + i)          # (the I_PCM macroblocks are put over these afterwards)
        else:
            raise ValueError(name)
        out.append(mb)
    return out


@functools.lru_cache(maxsize=None)
def _wave_plan(setting):
    """{(n, oi, group): (start, count)}: the share of the condition targets of its length that the group takes.  The groups of one
    length divide the targets among themselves without overlap, so that every batch holds targets no other batch has."""
    groups = {}
    for oi, offs in enumerate(WAVE_OFFSETS if setting != "spec_pcm" else WAVE_OFFSETS[:1]):
        for n in WAVE_COUNTS:
            for gi, f0 in enumerate(range(0, n, 8)):
                groups.setdefault(min(8, n - f0), []).append((n, oi, gi))
    plan = {}
    for L, keys in groups.items():
        total = len(targets(L, WAVE_OFFSETS[0], setting)[1])
        share = -(-total // len(keys))
        for i, key in enumerate(keys):
            plan[key] = (i * share, min(share, max(0, total - i * share)))
    return plan


@functools.lru_cache(maxsize=None)
def _wave_records(n, oi, setting):
    """(rec[n, N, 800], pcm[n, N] or None).  The groups are those of eight pictures."""
    W, H = WAVE_SHAPE
    N = W * H
    offs = WAVE_OFFSETS[oi]
    rng = np.random.default_rng([3, n, oi, SETTINGS.index(setting)])
    rec = np.zeros((n, N, 800), np.uint8)
    pcm = np.zeros((n, N), bool)
    for gi, f0 in enumerate(range(0, n, 8)):
        L = min(8, n - f0)
        first, rest = targets(L, offs, setting)
        start, count = _wave_plan(setting)[n, oi, gi]
        assert len(first) + count <= N
        todo = first + rest[start:start + count]
        todo += [first[i % len(first)] for i in range(N - len(todo))]      # the positions left over repeat the combinations
        # the plane targets need both neighbours: they take positions with x > 0 and y > 0 first
        inner = [p for p in range(N) if p % W and p // W]
        edge = [p for p in range(N) if not (p % W and p // W)]
        want_inner = [t for t in todo if t[0] == "cond" and t[1] in ("chroma_plane", "i16_plane")]
        others = [t for t in todo if not (t[0] == "cond" and t[1] in ("chroma_plane", "i16_plane"))]
        assert len(want_inner) <= len(inner)
        places = inner[:len(want_inner)] + edge + inner[len(want_inner):]
        for p, t in zip(places, want_inner + others):
            for i, mb in enumerate(_realize(rng, t, L, p % W, p // W, offs)):
                rec[f0 + i, p] = mb
            if t[0] == "cond" and t[1] == "ipcm":
                sat = range(0) if t[2] == "none" else range(L) if t[2] == "all" else (t[2],)
                for i in sat:
                    pcm[f0 + i, p] = True
    return rec, (pcm if setting == "spec_pcm" else None)


# ---- the corpus ---------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def corpus(setting):
    """the batches of one setting, in a fixed order"""
    assert setting in SETTINGS
    out = []
    base = "spec" if setting == "spec_pcm" else setting
    for (W, H) in SHAPES:
        rec = _positional_records(W, H)
        for j in range(4):
            out.append(_finish(W, H, OFFSETS[(W, H)], base, rec[15 * j:15 * j + 15], "positional %dx%d #%d" % (W, H, j), "positional"))
        if setting == "parity":
            z = _zero_records(W, H)
            for j, pick in enumerate((list(range(0, 9)) + [18, 19], list(range(9, 18)) + [20, 21])):
                out.append(_finish(W, H, OFFSETS[(W, H)], base, z[pick], "zero %dx%d #%d" % (W, H, j), "zero"))
    W, H = WAVE_SHAPE
    for oi, offs in enumerate(WAVE_OFFSETS):
        for n in WAVE_COUNTS:
            rec, _ = _wave_records(n, oi, base)
            out.append(_finish(W, H, offs, base, rec.copy(), "wave %s n=%d" % (offs, n), "wave"))
    if setting == "spec_pcm":
        for n in WAVE_COUNTS:
            rec, pcm = _wave_records(n, 0, "spec_pcm")
            out.append(_finish(W, H, WAVE_OFFSETS[0], "spec", rec.copy(), "wave pcm n=%d" % n, "wave_pcm", pcm=pcm))
    return tuple(out)


def shapes_of(setting):
    return sorted({(int(b.params.width_mbs), int(b.params.height_mbs)) for b in corpus(setting)})
