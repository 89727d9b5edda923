"""NumPy / Python-int restatement of the plane histograms and the representative-picture choice (DESIGN.md 3 "Representative
pictures"; plane_hist.hip, csrc/host/represent_policy.h): the record of a picture's rectangle (np.bincount per plane), the
picture-score sums of a record, and the choice among a slot's candidates in Python integers."""
import numpy as np

HIST_DTYPE = np.dtype([("y", "<u4", (256,)), ("cb", "<u4", (256,)), ("cr", "<u4", (256,)), ("samples", "<u4"),
                       ("chroma_samples", "<u4"), ("reserved", "<u4", (6,))])


def planes(yuv, wmb, hmb):
    """(Y, Cb, Cr) of one coded picture: (16 hmb, 16 wmb), and twice (8 hmb, 8 wmb)"""
    W, H = 16 * wmb, 16 * hmb
    flat = np.asarray(yuv).reshape(-1)
    y = flat[:W * H].reshape(H, W)
    cb = flat[W * H:W * H + W * H // 4].reshape(H // 2, W // 2)
    cr = flat[W * H + W * H // 4:W * H * 3 // 2].reshape(H // 2, W // 2)
    return y, cb, cr


def record_of_planes(y, cb, cr, rect):
    """the 3104 bytes of mvhp_plane_hist_t: y over rect = (cx, cy, cw, ch), cb and cr over the rectangle halved"""
    cx, cy, cw, ch = rect
    rec = np.zeros(1, HIST_DTYPE)
    rec["y"][0] = np.bincount(np.asarray(y)[cy:cy + ch, cx:cx + cw].reshape(-1), minlength=256)
    rec["cb"][0] = np.bincount(np.asarray(cb)[cy // 2:(cy + ch) // 2, cx // 2:(cx + cw) // 2].reshape(-1), minlength=256)
    rec["cr"][0] = np.bincount(np.asarray(cr)[cy // 2:(cy + ch) // 2, cx // 2:(cx + cw) // 2].reshape(-1), minlength=256)
    rec["samples"], rec["chroma_samples"] = cw * ch, (cw // 2) * (ch // 2)
    return rec


def record(yuv, wmb, hmb, rect):
    return record_of_planes(*planes(yuv, wmb, hmb), rect)


def records(yuv, n, wmb, hmb, rect):
    """n coded pictures (flat uint8) -> n records over rect"""
    fb = wmb * hmb * 384
    flat = np.asarray(yuv).reshape(-1)
    return np.concatenate([record(flat[k * fb:(k + 1) * fb], wmb, hmb, rect) for k in range(n)])


def stats(rec):
    """(sum, sum of squares, samples) of the luma samples a record counted, Python integers"""
    y = [int(c) for c in np.asarray(rec["y"]).reshape(256)]
    return sum(v * c for v, c in enumerate(y)), sum(v * v * c for v, c in enumerate(y)), sum(y)


def bins(rec):
    """the 768 counts of a record, Python integers"""
    return [c for p in ("y", "cb", "cr") for c in np.asarray(rec[p]).reshape(256).tolist()]


def distances(hists):
    """hists: lists of counts, all candidates -> D_i = sum_b (k h_i[b] - M[b])^2, Python integers (object arrays: NumPy only
    loops, every operation is Python's own integer arithmetic)"""
    k = len(hists)
    H = np.array(hists, dtype=object).reshape(k, -1)
    M = H.sum(axis=0)
    return [int(d) for d in ((k * H - M) ** 2).sum(axis=1)]


def choose(recs, eligible=None):
    """recs: HIST_DTYPE records -> the index of the eligible candidate nearest the candidates' mean histogram, the earliest on a
    tie; candidates are the eligible entries whose sizes equal those of the first eligible one; -1 for none"""
    n = len(recs)
    el = [True] * n if eligible is None else [bool(e) for e in eligible]
    live = [i for i in range(n) if el[i]]
    if not live:
        return -1
    size = (int(recs[live[0]]["samples"]), int(recs[live[0]]["chroma_samples"]))
    cand = [i for i in live if (int(recs[i]["samples"]), int(recs[i]["chroma_samples"])) == size]
    d = distances([bins(recs[i]) for i in cand])
    return cand[d.index(min(d))]
