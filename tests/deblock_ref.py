"""NumPy reference of the H.264 in-loop deblocking filter (clause 8.7), written from the standard's text for what the front end
produces: frame macroblocks (no MBAFF, no fields), 4:2:0, 8-bit, every macroblock intra -- bS = 4 on macroblock edges, bS = 3
on internal edges, luma internal edges 4 and 12 skipped for transform_size_8x8_flag, chroma edges 0 and 4 always.

There is no other H.264 decoder available to the suite to pin it against, and the reference decoder the project is pinned to never
deblocks: this module, the hand-derived known answers of tests/test_deblock.py and the HIP kernel (deblock.hip, with the
per-edge arithmetic of deblock_edge.h) are three restatements of clause 8.7 that must agree byte for byte.

Vectorised over pictures and over the lines of an edge, and over macroblocks as well: the macroblocks with the same
x + 2y are filtered together.  That is the standard's raster order in another guise -- MB(x, y) touches only samples that
MB(x - 1, y), MB(x + 1, y - 1), MB(x, y - 1) and MB(x - 1, y + 1) also touch, and those four come before it (x + 2y smaller)
or after it (larger) in both orders; two macroblocks of one step never touch the same sample.

Entry point: deblock(yuv, packed, params) -> filtered yuv (same shape), with yuv = n pictures of planar Y | Cb | Cr of the
coded size, packed = their packed records (the 32-byte headers are read: mb_kind, qp_y, flags bits 1-2 =
disable_deblocking_filter_idc, unavail, dbk_offsets) and params an mvhp_stream_params_t (size, chroma QP offsets)."""
import numpy as np

# Table 8-16 (indexA / indexB 0..51)
ALPHA = np.array([0] * 16 + [4, 4, 5, 6, 7, 8, 9, 10, 12, 13, 15, 17, 20, 22, 25, 28, 32, 36, 40, 45, 50, 56, 63, 71, 80, 90,
                             101, 113, 127, 144, 162, 182, 203, 226, 255, 255], np.int32)
BETA = np.array([0] * 16 + [2, 2, 2, 3, 3, 3, 3, 4, 4, 4, 6, 6, 7, 7, 8, 8, 9, 9, 10, 10, 11, 11, 12, 12, 13, 13, 14, 14, 15, 15,
                            16, 16, 17, 17, 18, 18], np.int32)
# Table 8-17, column bS = 3
TC0_BS3 = np.array([0] * 17 + [1] * 10 + [2] * 4 + [3] * 3 + [4] * 3 + [5, 6, 6, 7, 8, 9, 10, 11, 13, 14, 16, 18, 20, 23, 25],
                   np.int32)
# Table 8-15: QPc as a function of qPI
QPC = np.array(list(range(30)) + [29, 30, 31, 32, 32, 33, 34, 34, 35, 35, 36, 36, 37, 37, 37, 38, 38, 38, 39, 39, 39, 39],
               np.int32)
assert len(ALPHA) == len(BETA) == len(TC0_BS3) == len(QPC) == 52

KIND_I8X8, KIND_IPCM = 1, 3
UNAVAIL_A, UNAVAIL_B = 1, 2


def qpc(qpy, offset):
    return QPC[np.clip(np.asarray(qpy) + offset, 0, 51)]


def edge_params(qpav, alpha_div2, beta_div2):
    """(alpha, beta, tC0 for bS 3) of an edge: indexA = Clip3(0, 51, qPav + FilterOffsetA), FilterOffsetA = 2 * div2."""
    ia = np.clip(np.asarray(qpav) + 2 * np.asarray(alpha_div2), 0, 51)
    ib = np.clip(np.asarray(qpav) + 2 * np.asarray(beta_div2), 0, 51)
    return ALPHA[ia], BETA[ib], TC0_BS3[ia]


def filter_lines(v, alpha, beta, tc0, bs4, chroma, enable=True):
    """v[..., 8] = p3 p2 p1 p0 q0 q1 q2 q3 (any integer dtype); alpha / beta / tc0 / bs4 / enable broadcast against v[..., 0].
    Returns the filtered lines as int32 (8.7.2.3 for bS < 4, 8.7.2.4 for bS = 4)."""
    v = np.asarray(v).astype(np.int32)
    p3, p2, p1, p0, q0, q1, q2, q3 = (v[..., i] for i in range(8))
    alpha, beta, tc0 = (np.broadcast_to(np.asarray(t, np.int32), p0.shape) for t in (alpha, beta, tc0))
    bs4 = np.broadcast_to(np.asarray(bs4, bool), p0.shape)
    go = np.broadcast_to(np.asarray(enable, bool), p0.shape) & (np.abs(p0 - q0) < alpha) & (np.abs(p1 - p0) < beta) & \
        (np.abs(q1 - q0) < beta)
    ap, aq = np.abs(p2 - p0), np.abs(q2 - q0)
    out = v.copy()
    # bS = 4
    if chroma:
        strong_p = strong_q = np.zeros_like(go)
    else:
        small = np.abs(p0 - q0) < ((alpha >> 2) + 2)
        strong_p, strong_q = (ap < beta) & small, (aq < beta) & small
    s4 = go & bs4
    P0 = np.where(strong_p, (p2 + 2 * p1 + 2 * p0 + 2 * q0 + q1 + 4) >> 3, (2 * p1 + p0 + q1 + 2) >> 2)
    Q0 = np.where(strong_q, (p1 + 2 * p0 + 2 * q0 + 2 * q1 + q2 + 4) >> 3, (2 * q1 + q0 + p1 + 2) >> 2)
    P1 = np.where(strong_p, (p2 + p1 + p0 + q0 + 2) >> 2, p1)
    Q1 = np.where(strong_q, (p0 + q0 + q1 + q2 + 2) >> 2, q1)
    P2 = np.where(strong_p, (2 * p3 + 3 * p2 + p1 + p0 + q0 + 4) >> 3, p2)
    Q2 = np.where(strong_q, (2 * q3 + 3 * q2 + q1 + q0 + p0 + 4) >> 3, q2)
    # bS < 4 (here 3)
    s3 = go & ~bs4
    tc = tc0 + 1 if chroma else tc0 + (ap < beta) + (aq < beta)
    delta = np.clip((((q0 - p0) << 2) + (p1 - q1) + 4) >> 3, -tc, tc)
    N_P0, N_Q0 = np.clip(p0 + delta, 0, 255), np.clip(q0 - delta, 0, 255)
    if chroma:
        N_P1, N_Q1 = p1, q1
    else:
        N_P1 = np.where(ap < beta, p1 + np.clip((p2 + ((p0 + q0 + 1) >> 1) - (p1 << 1)) >> 1, -tc0, tc0), p1)
        N_Q1 = np.where(aq < beta, q1 + np.clip((q2 + ((p0 + q0 + 1) >> 1) - (q1 << 1)) >> 1, -tc0, tc0), q1)
    out[..., 3] = np.where(s4, P0, np.where(s3, N_P0, p0))
    out[..., 4] = np.where(s4, Q0, np.where(s3, N_Q0, q0))
    out[..., 2] = np.where(s4, P1, np.where(s3, N_P1, p1))
    out[..., 5] = np.where(s4, Q1, np.where(s3, N_Q1, q1))
    out[..., 1] = np.where(s4, P2, p2)
    out[..., 6] = np.where(s4, Q2, q2)
    return out


def header_fields(packed, n, mbs):
    """per picture and macroblock: (filter QP'Y, idc, alpha_div2, beta_div2, transform 8x8, unavail)"""
    h = np.asarray(packed, np.uint8).reshape(n, mbs, -1)[:, :, :32].astype(np.int32)
    kind, qp = h[..., 0], h[..., 1]
    qp = np.where(kind == KIND_IPCM, 0, qp)          # 8.7.2.2: qPp of an I_PCM macroblock is 0
    idc = (h[..., 5] >> 1) & 3
    off = h[..., 7]
    a2 = ((off & 15) ^ 8) - 8
    b2 = (((off >> 4) & 15) ^ 8) - 8
    return qp, idc, a2, b2, kind == KIND_I8X8, h[..., 6]


def _filter_plane(P, W, H, mbsz, qp, idc, a2, b2, t8, un, chroma):
    """P: [n, 4 + H*mbsz, 4 + W*mbsz] int32, padded by 4 on top / left; filtered in place.  qp etc.: [n, H, W]."""
    n = P.shape[0]
    on = idc != 1
    xs_all, ys_all = np.meshgrid(np.arange(W), np.arange(H))
    t_of = xs_all + 2 * ys_all
    nedge = mbsz // 4                                   # luma: edges 0, 4, 8, 12; chroma: 0, 4
    w = 4 + mbsz
    r16, c20 = np.arange(mbsz), np.arange(w)
    for t in range(int(t_of.max()) + 1):
        ys, xs = np.nonzero(t_of == t)
        if ys.size == 0:
            continue
        q = qp[:, ys, xs]
        qleft = qp[:, ys, np.maximum(xs - 1, 0)]
        qtop = qp[:, np.maximum(ys - 1, 0), xs]
        o = on[:, ys, xs]
        A2, B2 = a2[:, ys, xs], b2[:, ys, xs]
        i2 = idc[:, ys, xs] == 2
        left = o & (xs > 0)[None] & ~(i2 & ((un[:, ys, xs] & UNAVAIL_A) != 0))
        top = o & (ys > 0)[None] & ~(i2 & ((un[:, ys, xs] & UNAVAIL_B) != 0))
        inner = o & ~t8[:, ys, xs] if not chroma else o
        for direction in (0, 1):                          # vertical edges (along rows), then horizontal edges
            rows = 4 + ys[:, None] * mbsz + r16[None, :]   # [M, mbsz] lines
            cols = ys[:, None] * 0 + xs[:, None] * mbsz + c20[None, :]   # [M, w] window incl. 4 samples before the edge
            if direction == 0:
                idx = (rows[:, :, None], cols[:, None, :])            # [M, mbsz lines, w]
            else:
                rr = ys[:, None] * mbsz + c20[None, :]                # rows of the window (incl. 4 above)
                cc = 4 + xs[:, None] * mbsz + r16[None, :]            # the lines are columns
                idx = (rr[:, None, :], cc[:, :, None])                # [M, mbsz lines, w]
            L = P[:, idx[0], idx[1]]                                  # [n, M, lines, w]
            mbedge = left if direction == 0 else top
            nb = qleft if direction == 0 else qtop
            for k in range(nedge):
                if k == 0:
                    qpav, en, bs4 = (nb + q + 1) >> 1, mbedge, True
                else:
                    qpav, bs4 = q, False
                    en = o if (chroma or k == 2) else inner
                al, be, tc = edge_params(qpav, A2, B2)
                seg = L[..., 4 * k:4 * k + 8]
                L[..., 4 * k:4 * k + 8] = filter_lines(seg, al[..., None], be[..., None], tc[..., None], bs4, chroma,
                                                       en[..., None])
            P[:, idx[0], idx[1]] = L


def deblock(yuv, packed, params):
    W, H = int(params.width_mbs), int(params.height_mbs)
    mbs = W * H
    flat = np.asarray(yuv, np.uint8)
    n = flat.size // (mbs * 384)
    f = flat.reshape(n, mbs * 384)
    qp, idc, a2, b2, t8, un = (a.reshape(n, H, W) for a in header_fields(packed, n, mbs))
    out = f.copy()
    planes = ((0, 16, 16 * W, 16 * H, None), (mbs * 256, 8, 8 * W, 8 * H, int(params.chroma_qp_index_offset)),
              (mbs * 320, 8, 8 * W, 8 * H, int(params.second_chroma_qp_index_offset)))
    for base, mbsz, pw, ph, coff in planes:
        P = np.zeros((n, ph + 4, pw + 4), np.int32)
        P[:, 4:, 4:] = f[:, base:base + pw * ph].reshape(n, ph, pw)
        q = qp if coff is None else qpc(qp, coff)
        _filter_plane(P, W, H, mbsz, q, idc, a2, b2, t8, un, coff is not None)
        out[:, base:base + pw * ph] = P[:, 4:, 4:].reshape(n, -1).astype(np.uint8)
    return out.reshape(flat.shape)
