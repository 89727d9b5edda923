"""Census of reconstruction inputs (TEST INFRASTRUCTURE, pure NumPy, no device): WHICH code paths of the reconstruction kernels a
set of packed records (include/minivideo_hotpath.h) enters, as a set of named cells, and the universe of legal cells by rule.
A byte-for-byte comparison proves nothing about a path no input enters; tests/test_recon_census.py asserts that the directed corpus
(tests/recon_directed.py) reaches every cell of the universe, tools/census_report.py says what the older corpora reach.

Two kinds of cells (DESIGN.md section 5 "Content census" has the branch table they come from).

MACROBLOCK cells carry the position class of the macroblock, read from the kernels:
  column  only (W = 1) | first | last | strip_first (x % 4 = 0, x > 0) | strip_last (x % 4 = 3, x < W - 1) | inner
  row     first | band_first (y > 0 and y % rows_per_band = 0; rows_per_band 0 = a form without bands) | other
  ("i4",  col, row, block 0-15, mode 0-8, coded)         ("i8", col, row, block 0-3, mode 0-8, coded)
  ("i16", col, row, mode 0-3, luma 0 none / 1 DC only / 2 AC, QP'Y = 36)      ("chroma", col, row, mode 0-3, 0 none / 1 DC only / 2 AC)
  parity mode only, a mode whose neighbours are missing (the reference predicts 0):
  ("zero", "i4" | "i8", (left, above, corner missing), mode)      ("zero", "i16" | "chroma", (left, above missing), mode)
and, without a position:  ("qp", kind, QP'Y)   ("qpc", plane, QPc)   ("qpi_clip", plane, 0 | 51)  (qPI clipped under offset -12 / +12).

WAVE cells belong to a GROUP of pictures that one wavefront keeps in lock step at one macroblock position (eight: recon_oct.hip;
four: recon_quad.hip, recon_pipe.hip), and say how many pictures of the group satisfy the condition of a wave-uniform branch:
  ("wave", condition, "none" | "one" | "all", length class, index of the one picture | None)
  ("wave2", "any_l_any_c", (some picture has a luma level, some a chroma level), length class)
  ("wave2", "slow", (some picture dequantises luma / Cb / Cr below qP 24), length class)
length class: "full", or ("short", n) for the last group of a batch.  The one-picture forms (recon_kernels.hip, recon_pipe1.hip) run
the residuals of TWO macroblocks of a row in one wavefront (recon_rows_device.h residual_pair): group = 1 means those pairs,
  ("pair", "need" | "slow", "none" | "one" | "all", "full" | ("short", 1), index | None).

A cell leaves universe() only because a rule stated there makes it impossible, never because a builder could not reach it."""
import itertools

import numpy as np

I4, I8, I16, PCM = 0, 1, 2, 3
KIND = ("i4", "i8", "i16", "pcm")
SPEC_LUMA_DC = 2
MODES = ("parity", "spec", "spec_pcm")
BLK4 = [(8 * ((b // 4) % 2) + 4 * ((b % 4) % 2), 8 * ((b // 4) // 2) + 4 * ((b % 4) // 2)) for b in range(16)]
BLK8 = [(8 * (b % 2), 8 * (b // 2)) for b in range(4)]
QPC = list(range(30)) + [29, 30, 31, 32, 32, 33, 34, 34, 35, 35, 36, 36, 37, 37, 37, 38, 38, 38, 39, 39, 39, 39]   # Table 8-15
# what a mode reads: (left, above, corner) -- 8.3.1.2 / 8.3.2.2; modes 3 and 7 substitute a missing above-right
NEEDS = {0: (0, 1, 0), 1: (1, 0, 0), 2: (0, 0, 0), 3: (0, 1, 0), 4: (1, 1, 1), 5: (1, 1, 1), 6: (1, 1, 1), 7: (0, 1, 0), 8: (1, 0, 0)}
NEEDS16 = {0: (0, 1), 1: (1, 0), 2: (0, 0), 3: (1, 1)}          # Intra16x16PredMode: V, H, DC, Plane (left, above)
NEEDSC = {0: (0, 0), 1: (1, 0), 2: (0, 1), 3: (1, 1)}           # intra_chroma_pred_mode: DC, H, V, Plane
WAVE_CONDS = ("need_l", "need_c", "luma_slow", "cb_slow", "cr_slow", "chroma_plane", "i16_plane", "i4_dc", "i8_dc")


# ---- position classes -------------------------------------------------------------------------------------------------------
def col_class(x, W):
    if W == 1:
        return "only"
    if x == 0:
        return "first"
    if x == W - 1:
        return "last"
    return {0: "strip_first", 3: "strip_last"}.get(x % 4, "inner")


def row_class(y, rows_per_band):
    if y == 0:
        return "first"
    return "band_first" if rows_per_band and y % rows_per_band == 0 else "other"


def neighbours_of(col, row):
    """(mbAddrA, mbAddrB available) of a position class (one slice: geometry alone, 6.4.8)"""
    return col not in ("only", "first"), row != "first"


def block_avail(size, b, A, B):
    """(left, above, corner) available for block b of `size` samples (tests/spec_synth.py::_nxn states the same rule)"""
    xO, yO = (BLK4 if size == 4 else BLK8)[b]
    left, up = A or xO > 0, B or yO > 0
    corner = (yO > 0 or B) if xO > 0 else (A if yO > 0 else (A and B))
    return left, up, corner


def _legal(needs, avail):
    return all(a or not n for n, a in zip(needs, avail))


def _missing(avail):
    return tuple(0 if a else 1 for a in avail)


def length_class(n, group):
    return "full" if n == group else ("short", n)


# ---- the census ---------------------------------------------------------------------------------------------------------------
def _fields(params, records):
    rec = np.ascontiguousarray(records, np.uint8)
    F, N = rec.shape[0], rec.shape[1]
    coef = np.ascontiguousarray(rec[..., 32:]).view(np.int16).reshape(F, N, 384)
    nz = np.ascontiguousarray(rec[..., 8:12]).view(np.uint32).reshape(F, N)
    kind, qp = rec[..., 0].astype(int), np.minimum(rec[..., 1].astype(int), 51)
    offs = (int(params.chroma_qp_index_offset), int(params.second_chroma_qp_index_offset))
    qpc = [np.array(QPC)[np.clip(qp + o, 0, 51)] for o in offs]
    return rec, F, N, coef, nz, kind, qp, offs, qpc


def raw_cells(params, records):
    """the macroblock cells of records[F, N, 800] before the position classes: {(x, y): set of cells without (col, row)}, and the
    cells that have no position.  Raises ValueError for a spec-mode picture with a mode whose neighbours are missing."""
    W, H = int(params.width_mbs), int(params.height_mbs)
    parity = not params.flags & SPEC_LUMA_DC
    rec, F, N, coef, nz, kind, qp, offs, qpc = _fields(params, records)
    assert N == W * H
    blk4 = (coef[..., :256].reshape(F, N, 16, 16) != 0).any(-1)
    blk8 = (coef[..., :256].reshape(F, N, 4, 64) != 0).any(-1)
    lum16 = np.where(blk4.any(-1), np.where((coef[..., :256].reshape(F, N, 16, 16)[..., 1:] != 0).any((-1, -2)), 2, 1), 0)
    ch = coef[..., 256:].reshape(F, N, 8, 16)
    chc = np.where((ch[..., 1:] != 0).any((-1, -2)), 2, np.where((ch[..., 0] != 0).any(-1), 1, 0))
    pos, free = {}, set()
    for n in range(N):
        x, y = n % W, n // W
        A, B = x > 0, y > 0
        out = pos.setdefault((x, y), set())

        def put(cell, needs, avail, zero):
            if _legal(needs, avail):
                out.add(cell)
            elif parity:
                out.add(zero)
            else:
                raise ValueError("macroblock (%d, %d): %r reads a neighbour that is not available" % (x, y, cell))

        a4 = [block_avail(4, b, A, B) for b in range(16)]
        a8 = [block_avail(8, b, A, B) for b in range(4)]
        for f in range(F):
            k = kind[f, n]
            r = rec[f, n]
            if k == I4:
                for b in range(16):
                    m = int(r[12 + b])
                    put(("i4", b, m, bool(blk4[f, n, b])), NEEDS[m], a4[b], ("zero", "i4", _missing(a4[b]), m))
            elif k == I8:
                for b in range(4):
                    m = int(r[12 + b])
                    put(("i8", b, m, bool(blk8[f, n, b])), NEEDS[m], a8[b], ("zero", "i8", _missing(a8[b]), m))
            elif k == I16:
                m = int(r[4])
                put(("i16", m, int(lum16[f, n]), bool(qp[f, n] == 36)), NEEDS16[m], (A, B), ("zero", "i16", _missing((A, B)), m))
            elif k != PCM:
                raise ValueError("macroblock kind %d" % k)
            free.add(("qp", KIND[k], int(qp[f, n])))
            if k != PCM:
                m = int(r[3])
                put(("chroma", m, int(chc[f, n])), NEEDSC[m], (A, B), ("zero", "chroma", _missing((A, B)), m))
                for pl in (0, 1):
                    free.add(("qpc", pl, int(qpc[pl][f, n])))
                    if offs[pl] == -12 and qp[f, n] + offs[pl] < 0:
                        free.add(("qpi_clip", pl, 0))
                    if offs[pl] == 12 and qp[f, n] + offs[pl] > 51:
                        free.add(("qpi_clip", pl, 51))
    return pos, free


def classed(pos, W, rows_per_band):
    """raw_cells' positional part under the position classes of (W, rows_per_band)"""
    out = set()
    for (x, y), cells in pos.items():
        c, r = col_class(x, W), row_class(y, rows_per_band)
        for t in cells:
            out.add(t if t[0] == "zero" else (t[0], c, r) + t[1:])
    return out


def conditions(params, records):
    """per picture and macroblock (i4_dc / i8_dc: and block), the conditions the wave-uniform branches ballot on"""
    W = int(params.width_mbs)
    parity = not params.flags & SPEC_LUMA_DC
    rec, F, N, coef, nz, kind, qp, offs, qpc = _fields(params, records)
    x, y = np.arange(N) % W, np.arange(N) // W
    inner = ((x > 0) & (y > 0))[None, :]
    quirk = (kind == I16) & (qp == 36) & parity
    modes = rec[..., 12:28].astype(int)
    c = {"need_l": ((nz & 0xffff) != 0) | quirk,
         "need_c": (nz & 0xff0000) != 0,
         "luma_slow": (kind != I8) & (qp < 24),
         "cb_slow": qpc[0] < 24,
         "cr_slow": qpc[1] < 24,
         "chroma_plane": (rec[..., 3] == 3) & inner & (kind != PCM),
         "i16_plane": (kind == I16) & (rec[..., 4] == 3) & inner,
         "i4_dc": (kind == I4)[..., None] & (modes == 2),
         "i8_dc": (kind == I8)[..., None] & (modes[..., :4] == 2),
         "ipcm": kind == PCM,
         "quirk_only": quirk & ((nz & 0xffff) == 0),
         "luma_nz": (nz & 0xffff) != 0}
    return c, parity


def _count_cells(tag, name, cond, lc, out):
    """cond[L, ...]: pictures (or macroblocks) of one group x positions"""
    L = cond.shape[0]
    cnt = cond.sum(0).reshape(-1)
    first = cond.argmax(0).reshape(-1)
    if (cnt == 0).any():
        out.add((tag, name, "none", lc, None))
    if (cnt == L).any():
        out.add((tag, name, "all", lc, None))
    for i in np.unique(first[cnt == 1]):
        out.add((tag, name, "one", lc, int(i)))


def wave_cells(params, records, group):
    c, parity = conditions(params, records)
    F = records.shape[0]
    W = int(params.width_mbs)
    out = set()
    if group == 1:
        # residual_pair's all_ge24 looks at QP'Y of both macroblocks whatever their kind, and at both QPc
        slow = (np.minimum(records[..., 1].astype(int), 51) < 24) | c["cb_slow"] | c["cr_slow"]
        need = c["need_l"] | c["need_c"]
        for name, v in (("need", need), ("slow", slow)):
            v = v.reshape(F, -1, W)
            for x0 in range(0, W, 2):
                pair = np.moveaxis(v[:, :, x0:x0 + 2], 2, 0)
                _count_cells("pair", name, pair, length_class(pair.shape[0], 2), out)
        return out
    names = WAVE_CONDS + (("quirk_only",) if parity else ()) + ("ipcm",)
    for f0 in range(0, F, group):
        sl = slice(f0, min(F, f0 + group))
        lc = length_class(sl.stop - f0, group)
        for name in names:
            v = c[name][sl]
            if name == "quirk_only":     # counted where nothing else keeps the luma stage alive
                v = v[:, ~c["luma_nz"][sl].any(0)]
            if name == "ipcm" and not c["ipcm"].any():
                continue
            if v.size:
                _count_cells("wave", name, v, lc, out)
        al, ac = c["need_l"][sl].any(0), c["need_c"][sl].any(0)
        for t in set(zip(al.tolist(), ac.tolist())):
            out.add(("wave2", "any_l_any_c", t, lc))
        s3 = [c[k][sl].any(0).tolist() for k in ("luma_slow", "cb_slow", "cr_slow")]
        for t in set(zip(*s3)):
            out.add(("wave2", "slow", t, lc))
    return out


def census(params, records, group, rows_per_band):
    """the cells records[n, W * H, 800] reach on a form that keeps `group` pictures in lock step (1: the one-picture forms) and works
    in bands of `rows_per_band` macroblock rows (0: no bands)"""
    records = np.asarray(records)
    pos, free = raw_cells(params, records)
    return classed(pos, int(params.width_mbs), rows_per_band) | free | wave_cells(params, records, group)


# ---- the universe -----------------------------------------------------------------------------------------------------------
def positional_universe(mode, W, H, rows_per_band, excluded=None):
    """the macroblock cells with a position class (and, parity: the "zero" cells) that pictures of W x H can reach.
    excluded: dict that receives, per rule, how many cells the rule removes."""
    assert mode in MODES
    ex = excluded if excluded is not None else {}

    def drop(rule, n=1):
        ex[rule] = ex.get(rule, 0) + n

    cols = sorted({col_class(x, W) for x in range(W)})
    rows = sorted({row_class(y, rows_per_band) for y in range(H)})
    every_col = ("only", "first", "last", "strip_first", "strip_last", "inner")
    every_row = ("first", "band_first", "other")
    per_class = 16 * 9 * 2 + 4 * 9 * 2 + 4 * 3 * 2 + 4 * 3
    drop("geometry: the shape has no such column or row class", (len(every_col) * len(every_row) - len(cols) * len(rows)) * per_class)
    out = set()
    for c, r in itertools.product(cols, rows):
        A, B = neighbours_of(c, r)
        for size, name, nb in ((4, "i4", 16), (8, "i8", 4)):
            for b in range(nb):
                av = block_avail(size, b, A, B)
                for m in range(9):
                    if _legal(NEEDS[m], av):
                        out.update((name, c, r, b, m, coded) for coded in (False, True))
                    else:
                        drop("6.4.8 / 8.3.1.2: %s mode needs a neighbour the position does not have" % name, 2)
                        if mode == "parity":
                            out.add(("zero", name, _missing(av), m))
        for m in range(4):
            if _legal(NEEDS16[m], (A, B)):
                out.update(("i16", c, r, m, lum, q) for lum in range(3) for q in (False, True))
            else:
                drop("8.3.3: Intra16x16 mode needs a neighbour the position does not have", 6)
                if mode == "parity":
                    out.add(("zero", "i16", _missing((A, B)), m))
            if _legal(NEEDSC[m], (A, B)):
                out.update(("chroma", c, r, m, cl) for cl in range(3))
            else:
                drop("8.3.4: chroma mode needs a neighbour the position does not have", 3)
                if mode == "parity":
                    out.add(("zero", "chroma", _missing((A, B)), m))
    return out


def free_universe(mode, group):
    """the cells without a position: QP, QPc, and the wave cells of a form of `group` pictures"""
    assert mode in MODES and group in (1, 4, 8)
    out = {("qp", k, q) for k in ("i4", "i8", "i16") for q in range(52)}
    # QPc: Table 8-15 maps qPI 0 .. 51 onto 0 .. 39 (onto), each plane with its own offset; the two clips of 8.5.8 under the extreme offsets
    out |= {("qpc", pl, v) for pl in (0, 1) for v in sorted(set(QPC))}
    out |= {("qpi_clip", pl, e) for pl in (0, 1) for e in (0, 51)}
    if mode == "spec_pcm":
        out.add(("qp", "pcm", 0))          # 7.4.5: QP'Y of an I_PCM macroblock is 0
    if group == 1:
        for name in ("need", "slow"):
            out |= {("pair", name, "none", "full", None), ("pair", name, "all", "full", None), ("pair", name, "one", "full", 0),
                    ("pair", name, "one", "full", 1), ("pair", name, "none", ("short", 1), None),
                    ("pair", name, "all", ("short", 1), None), ("pair", name, "one", ("short", 1), 0)}
        return out
    names = WAVE_CONDS + (("quirk_only",) if mode == "parity" else ()) + (("ipcm",) if mode == "spec_pcm" else ())
    for L in (group, group - 1, 1):
        lc = length_class(L, group)
        for name in names:
            out |= {("wave", name, "none", lc, None), ("wave", name, "all", lc, None)}
            out |= {("wave", name, "one", lc, i) for i in range(L)}
        out |= {("wave2", "any_l_any_c", t, lc) for t in itertools.product((False, True), repeat=2)}
        # chroma offsets of -12 .. 12 move either plane to either side of qP 24 whatever luma does: all eight
        out |= {("wave2", "slow", t, lc) for t in itertools.product((False, True), repeat=3)}
    return out


def universe(mode, W, H, group, rows_per_band, excluded=None):
    """every legal cell for pictures of W x H macroblocks in `mode` ("parity": flags 0 / MAY_HAVE_8X8 with the QP 36 defect and the
    reference's "predict 0"; "spec": MVHP_PARAM_SPEC_LUMA_DC; "spec_pcm": the same with I_PCM) on a form of `group` pictures per
    wavefront and `rows_per_band` rows per band.  The cells without a position do not depend on the shape: a corpus answers for
    them as a whole, each shape for its own positional cells."""
    return positional_universe(mode, W, H, rows_per_band, excluded) | free_universe(mode, group)


if __name__ == "__main__":
    for mode in MODES[:2]:
        for (W, H) in ((1, 1), (2, 1), (9, 9)):
            ex = {}
            u = positional_universe(mode, W, H, 4, ex)
            print("%s %dx%d rows_per_band 4: %d positional cells" % (mode, W, H, len(u)))
            for rule, n in sorted(ex.items()):
                print("    %7d  %s" % (n, rule))
