"""Black bars restated in NumPy and Python integers (DESIGN.md 3 "Black bars"): the reference of every bars test.  It shares no
code with the library.

A sample is bright when Y > level.  Row y of a rectangle cw x ch is content when at least need(cw) of its samples are bright,
column x when at least need(ch) of its samples are; need(L) = max(1, L >> 5).  A record is the box from the first to the last
content row / column in CODED coordinates, plus how many rows and columns are content; no content row or no content column: the
box is empty (all four zero), the counts are still reported."""
import numpy as np

DTYPE = np.dtype([("x", "<u4"), ("y", "<u4"), ("w", "<u4"), ("h", "<u4"), ("rows", "<u4"), ("cols", "<u4"), ("reserved", "<u4", (2,))])
LEVEL = 24
PROBES = 8


def need(length):
    return max(1, int(length) >> 5)


def luma_plane(picture, wmb, hmb):
    """the luma plane (a view) of one coded picture given as its 384 W H bytes"""
    W, H = 16 * wmb, 16 * hmb
    return np.asarray(picture).reshape(-1)[:W * H].reshape(H, W)


def record(Y, rect, level=LEVEL):
    """(x, y, w, h, rows, cols) of the luma plane Y over rect = (cx, cy, cw, ch)"""
    cx, cy, cw, ch = rect
    bright = np.asarray(Y)[cy:cy + ch, cx:cx + cw] > level
    rows = np.flatnonzero(bright.sum(axis=1) >= need(cw))
    cols = np.flatnonzero(bright.sum(axis=0) >= need(ch))
    if len(rows) == 0 or len(cols) == 0:
        return 0, 0, 0, 0, len(rows), len(cols)
    return (cx + int(cols[0]), cy + int(rows[0]), int(cols[-1] - cols[0]) + 1, int(rows[-1] - rows[0]) + 1, len(rows), len(cols))


def record_loops(Y, rect, level=LEVEL):
    """the same by a plain double loop (what record() is checked against)"""
    cx, cy, cw, ch = rect
    row_n, col_n = [0] * ch, [0] * cw
    for y in range(ch):
        for x in range(cw):
            if int(Y[cy + y][cx + x]) > level:
                row_n[y] += 1
                col_n[x] += 1
    rows = [y for y in range(ch) if row_n[y] >= need(cw)]
    cols = [x for x in range(cw) if col_n[x] >= need(ch)]
    if not rows or not cols:
        return 0, 0, 0, 0, len(rows), len(cols)
    return cx + cols[0], cy + rows[0], cols[-1] - cols[0] + 1, rows[-1] - rows[0] + 1, len(rows), len(cols)


def records(yuv, n, wmb, hmb, rect, level=LEVEL):
    """the n 32-byte records (DTYPE) of n coded pictures"""
    yuv = np.asarray(yuv).reshape(n, -1)
    out = np.zeros(n, dtype=DTYPE)
    for k in range(n):
        out[k]["x"], out[k]["y"], out[k]["w"], out[k]["h"], out[k]["rows"], out[k]["cols"] = record(luma_plane(yuv[k], wmb, hmb), rect, level)
    return out


def union(boxes):
    """(number of non-empty boxes, (x, y, w, h) of the smallest box that holds them all -- all zero when there is none)"""
    full = [b for b in boxes if b[2] > 0 and b[3] > 0]
    if not full:
        return 0, (0, 0, 0, 0)
    x0, y0 = min(b[0] for b in full), min(b[1] for b in full)
    x1, y1 = max(b[0] + b[2] for b in full), max(b[1] + b[3] for b in full)
    return len(full), (x0, y0, x1 - x0, y1 - y0)


def trim_rect(crop, u):
    """the trim rule: crop = (cx, cy, cw, ch), all even; u = (x, y, w, h) or None -> (accepted 0 / 1, the rectangle to use)"""
    cx, cy, cw, ch = crop
    if u is None or u[2] <= 0 or u[3] <= 0:
        return 0, tuple(crop)
    x0, x1 = max(cx, u[0]), min(cx + cw, u[0] + u[2])
    y0, y1 = max(cy, u[1]), min(cy + ch, u[1] + u[3])
    if x1 <= x0 or y1 <= y0:
        return 0, tuple(crop)
    x0, y0 = x0 - x0 % 2, y0 - y0 % 2          # left and top down to even
    x1, y1 = x1 + x1 % 2, y1 + y1 % 2          # right and bottom up to even
    if x1 - x0 < (cw + 1) // 2 or y1 - y0 < (ch + 1) // 2:
        return 0, tuple(crop)
    return 1, (x0, y0, x1 - x0, y1 - y0)


def probes(order, count=PROBES):
    """the pictures minivideo_decode probes: order[floor(k size / P)], k = 0 .. P - 1, P = min(count, size)"""
    size = len(order)
    P = min(count, size)
    return [order[k * size // P] for k in range(P)]
