"""NumPy / Python-int restatement of the picture scores and the blank-picture policy (DESIGN.md 3 "Picture scores";
luma_stats.hip, csrc/host/blank_policy.h): the record of a picture's rectangle, the score, the choice among a slot's candidates,
the alternates of a slot, and the whole two-pass policy of minivideo_decode as a function of the pictures' scores."""
import numpy as np

STATS_DTYPE = np.dtype([("sum", "<u8"), ("sumsq", "<u8"), ("samples", "<u4"), ("reserved", "<u4", (3,))])
SCORE_MAX = 260100          # half the samples 0, half 255: 16 * 127.5 ** 2


def luma_plane(yuv, wmb, hmb):
    """the luma plane (16 hmb, 16 wmb) of one coded picture"""
    W, H = 16 * wmb, 16 * hmb
    return np.asarray(yuv).reshape(-1)[:W * H].reshape(H, W)


def stats(luma, cx, cy, cw, ch):
    """(sum, sum of squares, samples) of the rectangle of a 2-D uint8 plane, Python integers (uint64 sums underneath)"""
    r = np.asarray(luma)[cy:cy + ch, cx:cx + cw].astype(np.uint64)
    assert r.shape == (ch, cw)
    return int(r.sum(dtype=np.uint64)), int((r * r).sum(dtype=np.uint64)), cw * ch


def record(luma, cx, cy, cw, ch):
    """the 32 bytes of mvhp_luma_stats_t for that rectangle"""
    s, q, n = stats(luma, cx, cy, cw, ch)
    rec = np.zeros(1, STATS_DTYPE)
    rec["sum"], rec["sumsq"], rec["samples"] = s, q, n
    return rec


def records(yuv, n, wmb, hmb, rect):
    """n coded pictures (flat uint8) -> n records over rect = (cx, cy, cw, ch)"""
    fb = wmb * hmb * 384
    flat = np.asarray(yuv).reshape(-1)
    return np.concatenate([record(luma_plane(flat[k * fb:(k + 1) * fb], wmb, hmb), *rect) for k in range(n)])


def score(s, q, n):
    """floor(16 (N Q - S^2) / N^2), Python integers"""
    s, q, n = int(s), int(q), int(n)
    if n == 0:
        return 0
    return max(0, 16 * (n * q - s * s)) // (n * n)


def picture_score(yuv, wmb, hmb, rect=None):
    rect = rect or (0, 0, 16 * wmb, 16 * hmb)
    return score(*stats(luma_plane(yuv, wmb, hmb), *rect))


def choose(scores, min_score):
    """index of the first score >= min_score, else of the largest (the earliest on a tie); -1 for none"""
    if not scores:
        return -1
    for i, v in enumerate(scores):
        if v >= min_score:
            return i
    return scores.index(max(scores))


def alternates(slots, n_idr, a):
    """slots: the IDR index of every slot's picture, in slot order -> per slot, the IDR indices strictly between it and the
    next slot's picture (the end of the stream for the last slot), in stream order, at most a"""
    out = []
    for k, idr in enumerate(slots):
        end = slots[k + 1] if k + 1 < len(slots) else n_idr
        out.append(list(range(idr + 1, min(end, n_idr)))[:a])
    return out


def policy(slots, scores, min_score, a):
    """slots: the IDR of every slot after pass 1; scores: the score of every IDR of the stream -> (the IDR every slot's file
    holds in the end, the IDRs pass 2 decodes, in order)"""
    final, second = [], []
    for k, alts in enumerate(alternates(slots, len(scores), a)):
        cand = [slots[k]]
        if scores[slots[k]] < min_score:
            cand += alts
            second += alts
        final.append(cand[choose([scores[i] for i in cand], min_score)])
    return final, second
