// resample_taps.h -- the tap arithmetic of the output-geometry filter (DESIGN.md 3 "Output geometry"), shared by the resample
// kernel (resample.hip), the host size rule and a host-compiled CPU test (tests/test_thumbnail.py compiles this header with g++
// and checks it against the NumPy restatement tests/resample_ref.py).  No HIP types: plain integer arithmetic.
//
// One axis, source length S (the cropped length), output length D <= S.  Output sample j covers [j S, (j + 1) S) in units where
// source sample i occupies [i D, (i + 1) D).  C(i) = clamp(i D - j S, 0, S) is the overlap accumulated before source sample i,
// F(c) = floor((c 2^14 + floor(S / 2)) / S), and the tap of source sample i is F(C(i + 1)) - F(C(i)): never negative, one
// weight at a time, and the taps of an output sample sum to exactly 2^14.
#pragma once
#include <stdint.h>

#if defined(__HIPCC__) || defined(__HIP__)
#define MVRS_HD __host__ __device__ __forceinline__
#else
#define MVRS_HD inline
#endif

namespace mvrs {

constexpr int kOne = 1 << 14;   // the weights of an output sample sum to this

// first covered source sample i0 and the number of covered samples of output sample j (S, D <= 16384: products fit 32 bits)
MVRS_HD void span(int S, int D, int j, int &i0, int &n)
{
    i0 = (int)(((uint32_t)j * (uint32_t)S) / (uint32_t)D);
    const int i1 = (int)(((uint32_t)(j + 1) * (uint32_t)S + (uint32_t)D - 1u) / (uint32_t)D);
    n = i1 - i0;
}

// F(C(i)) for output sample j: the cumulative weight before source sample i
MVRS_HD int cum(int S, int D, int j, int i)
{
    int c = i * D - j * S;
    c = c < 0 ? 0 : (c > S ? S : c);
    return (int)(((uint32_t)c * (uint32_t)kOne + (uint32_t)(S >> 1)) / (uint32_t)S);
}

// the tap of source sample i for output sample j
MVRS_HD int weight(int S, int D, int j, int i) { return cum(S, D, j, i + 1) - cum(S, D, j, i); }

// the vertical pass (first): sum of w_y * sample (<= 255 * 2^14) -> a 16-bit intermediate with 8 fractional bits
MVRS_HD uint32_t round_v(uint32_t acc) { return (acc + 32u) >> 6; }
// the horizontal pass: sum of w_x * intermediate (<= 65280 * 2^14 < 2^31) -> the output sample (<= 255)
MVRS_HD uint32_t round_h(uint32_t acc) { return (acc + (1u << 21)) >> 22; }

// The size rule: cw x ch (even) fitted into bw x bh (each >= 2): aspect kept, even sides, never enlarged.  0 = bad arguments.
MVRS_HD int fit(uint32_t cw, uint32_t ch, uint32_t bw, uint32_t bh, uint32_t &ow, uint32_t &oh)
{
    if (cw < 2 || ch < 2 || bw < 2 || bh < 2) return 0;
    if (cw <= bw && ch <= bh) {
        ow = cw;
        oh = ch;
        return 1;
    }
    const uint64_t W = cw, H = ch;
    if (W * bh >= H * bw) {   // width-limited
        ow = bw & ~1u;
        uint64_t h = 2 * ((H * ow + W) / (2 * W));
        if (h < 2) h = 2;
        if (h > (bh & ~1u)) h = bh & ~1u;
        oh = (uint32_t)h;
    } else {                  // height-limited
        oh = bh & ~1u;
        uint64_t w = 2 * ((W * oh + H) / (2 * H));
        if (w < 2) w = 2;
        if (w > (bw & ~1u)) w = bw & ~1u;
        ow = (uint32_t)w;
    }
    return 1;
}

// The aspect rule: cw x ch (even) whose samples are a : b as wide as high (0 in either: 1 : 1) -> the size with square samples.
// One axis shrinks, nothing is enlarged, sides stay even and at least 2.  64-bit: ch * b + a < 2^33 for sides and terms below 2^16
// (and for any 32-bit values).  0 = bad arguments.
MVRS_HD int aspect(uint32_t cw, uint32_t ch, uint32_t a, uint32_t b, uint32_t &ow, uint32_t &oh)
{
    if (cw < 2 || ch < 2) return 0;
    ow = cw;
    oh = ch;
    if (a == 0 || b == 0 || a == b) return 1;
    const uint64_t A = a, B = b;
    if (a > b) {   // wide samples: the height shrinks
        const uint64_t h = 2 * (((uint64_t)ch * B + A) / (2 * A));
        oh = h < 2 ? 2u : (uint32_t)h;
    } else {       // tall samples: the width shrinks
        const uint64_t w = 2 * (((uint64_t)cw * A + B) / (2 * B));
        ow = w < 2 ? 2u : (uint32_t)w;
    }
    return 1;
}

} // namespace mvrs
