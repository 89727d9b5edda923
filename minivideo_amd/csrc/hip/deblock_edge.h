// deblock_edge.h -- the per-edge arithmetic of the H.264 deblocking filter (clause 8.7.2), shared by the deblock kernel
// (deblock.hip) and a host-compiled CPU test (tests/test_deblock.py compiles this header with g++ and fuzzes it against the
// NumPy reference tests/deblock_ref.py).  8-bit samples, frame macroblocks, intra only: bS is 4 (macroblock edge) or 3
// (internal edge).  No HIP types: everything is plain int arithmetic.
#pragma once
#include <stdint.h>

#if defined(__HIPCC__) || defined(__HIP__)
#define MVDB_HD __host__ __device__ __forceinline__
#else
#define MVDB_HD inline
#endif

namespace mvdb {

// Table 8-16: alpha' and beta' by indexA / indexB (0..51)
#define MVDB_ALPHA_TABLE                                                                                                  \
    {0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 4, 4, 5, 6, 7, 8, 9, 10, 12, 13, 15, 17, 20, 22, 25, 28, 32, 36, 40, 45, \
     50, 56, 63, 71, 80, 90, 101, 113, 127, 144, 162, 182, 203, 226, 255, 255}
#define MVDB_BETA_TABLE                                                                                                  \
    {0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 2, 2, 2, 3, 3, 3, 3, 4, 4, 4, 6, 6, 7, 7, 8, 8, 9, 9, 10, 10, 11, 11, \
     12, 12, 13, 13, 14, 14, 15, 15, 16, 16, 17, 17, 18, 18}
// Table 8-17: tC0 for bS = 3 (the only bS < 4 an intra picture has)
#define MVDB_TC0_BS3_TABLE                                                                                               \
    {0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 1, 1, 1, 1, 1, 1, 1, 1, 1, 1, 2, 2, 2, 2, 3, 3, 3, 4, 4, 4, 5, 6, 6, \
     7, 8, 9, 10, 11, 13, 14, 16, 18, 20, 23, 25}
// Table 8-15: QPc by qPI for qPI >= 30 (below 30, QPc = qPI)
#define MVDB_QPC_TABLE {29, 30, 31, 32, 32, 33, 34, 34, 35, 35, 36, 36, 37, 37, 37, 38, 38, 38, 39, 39, 39, 39}

MVDB_HD int clip3(int lo, int hi, int v) { return v < lo ? lo : (v > hi ? hi : v); }
MVDB_HD int iabs(int v) { return v < 0 ? -v : v; }

// Filter parameters of one edge: alpha, beta and tC0 (bS = 3) looked up by the caller from indexA / indexB.
struct EdgeParams {
    int alpha, beta, tc0;
    int bs4;     // 1: bS = 4 (macroblock edge), 0: bS = 3 (internal edge)
};

// One line across an edge: v[0..3] = p3 p2 p1 p0, v[4..7] = q0 q1 q2 q3 (8.7.2.3 / 8.7.2.4).  Luma modifies up to p2 / q2,
// chroma (chroma = 1) only p0 / q0 and reads only p1..q1.
MVDB_HD void filter_line(int *v, const EdgeParams &e, bool chroma)
{
    const int p3 = v[0], p2 = v[1], p1 = v[2], p0 = v[3], q0 = v[4], q1 = v[5], q2 = v[6], q3 = v[7];
    if (!(iabs(p0 - q0) < e.alpha && iabs(p1 - p0) < e.beta && iabs(q1 - q0) < e.beta)) return;   // filterSamplesFlag (8-468)
    const int ap = iabs(p2 - p0), aq = iabs(q2 - q0);
    if (e.bs4) {   // 8.7.2.4
        if (!chroma && ap < e.beta && iabs(p0 - q0) < ((e.alpha >> 2) + 2)) {
            v[3] = (p2 + 2 * p1 + 2 * p0 + 2 * q0 + q1 + 4) >> 3;
            v[2] = (p2 + p1 + p0 + q0 + 2) >> 2;
            v[1] = (2 * p3 + 3 * p2 + p1 + p0 + q0 + 4) >> 3;
        } else {
            v[3] = (2 * p1 + p0 + q1 + 2) >> 2;
        }
        if (!chroma && aq < e.beta && iabs(p0 - q0) < ((e.alpha >> 2) + 2)) {
            v[4] = (p1 + 2 * p0 + 2 * q0 + 2 * q1 + q2 + 4) >> 3;
            v[5] = (p0 + q0 + q1 + q2 + 2) >> 2;
            v[6] = (2 * q3 + 3 * q2 + q1 + q0 + p0 + 4) >> 3;
        } else {
            v[4] = (2 * q1 + q0 + p1 + 2) >> 2;
        }
    } else {       // 8.7.2.3
        const int tc = chroma ? e.tc0 + 1 : e.tc0 + (ap < e.beta ? 1 : 0) + (aq < e.beta ? 1 : 0);
        const int delta = clip3(-tc, tc, (((q0 - p0) << 2) + (p1 - q1) + 4) >> 3);
        v[3] = clip3(0, 255, p0 + delta);
        v[4] = clip3(0, 255, q0 - delta);
        if (!chroma) {
            if (ap < e.beta) v[2] = p1 + clip3(-e.tc0, e.tc0, (p2 + ((p0 + q0 + 1) >> 1) - (p1 << 1)) >> 1);
            if (aq < e.beta) v[5] = q1 + clip3(-e.tc0, e.tc0, (q2 + ((p0 + q0 + 1) >> 1) - (q1 << 1)) >> 1);
        }
    }
}

// QP'Y used by the filter for a macroblock: 0 for I_PCM (8.7.2.2), its QP'Y otherwise.
MVDB_HD int filter_qp(int kind, int qp_y) { return kind == 3 ? 0 : qp_y; }

MVDB_HD int qpc_of(int qpy, int offset, const uint8_t *qpc_table)
{
    const int qpi = clip3(0, 51, qpy + offset);
    return qpi < 30 ? qpi : qpc_table[qpi - 30];
}

// alpha / beta / tC0 of an edge from qPav and the filter offsets (in units of 2, 8.7.2.2: FilterOffsetA = offset_div2 << 1)
MVDB_HD EdgeParams edge_params(int qpav, int alpha_div2, int beta_div2, int bs4, const uint8_t *alpha_t, const uint8_t *beta_t,
                               const uint8_t *tc0_t)
{
    const int ia = clip3(0, 51, qpav + alpha_div2 * 2), ib = clip3(0, 51, qpav + beta_div2 * 2);
    EdgeParams e;
    e.alpha = alpha_t[ia];
    e.beta = beta_t[ib];
    e.tc0 = tc0_t[ia];
    e.bs4 = bs4;
    return e;
}

} // namespace mvdb
