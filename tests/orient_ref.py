"""NumPy restatement of the orientation pass (DESIGN.md 3 "Orientation"; orient.hip): every plane of a picture turned by quarter
turns, clockwise, and the colour conversion of the turned planes (tests/resample_ref.py: the reference's integer formula,
2x2-nearest chroma).  For a source plane S of w x h and its output O:
    1 turn:  O[y][x] = S[h-1-x][y]       2 turns: O[y][x] = S[h-1-y][w-1-x]       3 turns: O[y][x] = S[x][w-1-y]
which are np.rot90 with k = -1, 2 and 1.  Checked against a plain per-sample loop in tests/test_orient.py."""
import numpy as np

from tests import resample_ref as R

ROT90_K = {0: 0, 1: -1, 2: 2, 3: 1}


def turned_size(w, h, turns):
    """size of a w x h picture after `turns` quarter turns"""
    return (h, w) if turns & 1 else (w, h)


def turn_plane(plane, turns):
    """one plane (2-D) turned clockwise by `turns` quarter turns"""
    return np.ascontiguousarray(np.rot90(plane, ROT90_K[turns & 3]))


def turn(planes, w, h, turns):
    """dense pictures (n x w*h*3/2 bytes, planar Y | Cb | Cr of w x h) -> the turned pictures, the same layout at the turned size"""
    planes = np.ascontiguousarray(planes, np.uint8).reshape(-1, w * h * 3 // 2)
    n, q = planes.shape[0], (w // 2) * (h // 2)
    out = np.empty_like(planes)
    for f in range(n):
        out[f, :w * h] = turn_plane(planes[f, :w * h].reshape(h, w), turns).reshape(-1)
        out[f, w * h:w * h + q] = turn_plane(planes[f, w * h:w * h + q].reshape(h // 2, w // 2), turns).reshape(-1)
        out[f, w * h + q:] = turn_plane(planes[f, w * h + q:].reshape(h // 2, w // 2), turns).reshape(-1)
    return out


def to_rgb(turned, w, h, turns):
    """RGB of turned pictures (what turn(planes, w, h, turns) returned)"""
    tw, th = turned_size(w, h, turns)
    return R.to_rgb(turned, tw, th)


def crop(yuv, width_mbs, height_mbs, rect):
    """coded pictures -> the dense pictures of rect = (cx, cy, cw, ch): what the coded source form reads"""
    cx, cy, cw, ch = rect
    Wp, Hp = 16 * width_mbs, 16 * height_mbs
    yuv = np.ascontiguousarray(yuv, np.uint8).reshape(-1, Wp * Hp * 3 // 2)
    n = yuv.shape[0]
    Y = yuv[:, :Wp * Hp].reshape(n, Hp, Wp)[:, cy:cy + ch, cx:cx + cw]
    C = yuv[:, Wp * Hp:].reshape(n, 2, Hp // 2, Wp // 2)[:, :, cy // 2:(cy + ch) // 2, cx // 2:(cx + cw) // 2]
    return np.concatenate([Y.reshape(n, -1), C.reshape(n, -1)], axis=1)


# ---- a plain per-sample loop: what the forms above are checked against ----
def turn_plane_loop(plane, turns):
    h, w = plane.shape
    ow, oh = turned_size(w, h, turns)
    out = np.zeros((oh, ow), plane.dtype)
    for y in range(oh):
        for x in range(ow):
            if turns == 0:
                out[y, x] = plane[y, x]
            elif turns == 1:
                out[y, x] = plane[h - 1 - x, y]
            elif turns == 2:
                out[y, x] = plane[h - 1 - y, w - 1 - x]
            else:
                out[y, x] = plane[x, w - 1 - y]
    return out
