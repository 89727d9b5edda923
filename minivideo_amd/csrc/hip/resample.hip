// resample.hip -- the output-geometry pass (opt-in: mvhp_resample_dev) over reconstructed (and, when asked, deblocked) coded
// planes, gfx950.  DESIGN.md 3 "Output geometry" defines the filter; the tap arithmetic is resample_taps.h, also compiled by
// the CPU test.
//
// Mapping: one workgroup of 256 threads per (picture, band of `band` chroma output rows = 2 band luma output rows).  For each
// output row of each plane:
//   vertical pass   lanes own aligned CH-byte column strips of the cropped source rows (CH = 16 for luma: one dwordx4 per tap
//                   row; 8 for chroma, whose rows are only 8-byte aligned); the tap weights are the same for the whole row,
//                   so the loads of a strip stream in coalesced and the weights stay wave-uniform.  The 16-bit intermediate
//                   row goes to LDS.
//   horizontal pass lanes own output samples and read their taps from LDS; the band's output rows are staged in LDS.
// Then the band leaves as whole runs of bytes: the planes (contiguous per plane: dword stores between a byte head and tail) and
// RGB from the staged rows (the packed colour helpers of recon_batch_device.h, 2x2-nearest chroma, four samples per lane).
// Stateless: nothing crosses workgroups, no waits -- safe under stream capture.  D = S (crop only) is the same pass: one tap
// of 2^14 in each direction reproduces every sample exactly; an axis with D = S skips its horizontal tap arithmetic.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "recon_batch_device.h"
#include "recon_kernels.h"
#include "resample_taps.h"

namespace mvhp {

namespace {

constexpr int kThreads = 256;

struct PlaneView {
    const uint8_t *base;   // the coded plane of this picture
    int pitch;             // bytes per coded row
    int x0, y0, sw, sh;    // the cropped rectangle in this plane
    int dw, dh;            // output size of this plane
};

template <int CH> struct Strip;
template <> struct Strip<16> {
    uint32_t w[4];
    __device__ __forceinline__ void load(const uint8_t *p)
    {
        const uint4 v = *reinterpret_cast<const uint4 *>(p);
        w[0] = v.x; w[1] = v.y; w[2] = v.z; w[3] = v.w;
    }
};
template <> struct Strip<8> {
    uint32_t w[2];
    __device__ __forceinline__ void load(const uint8_t *p)
    {
        const uint2 v = *reinterpret_cast<const uint2 *>(p);
        w[0] = v.x; w[1] = v.y;
    }
};

template <int CH>
__device__ __forceinline__ void mac(uint32_t (&acc)[CH], const Strip<CH> &s, uint32_t wt)
{
#pragma unroll
    for (int b = 0; b < CH; b++) acc[b] += wt * ((s.w[b >> 2] >> (8 * (b & 3))) & 255u);
}

// vertical taps of output row j of plane P -> t[0 .. P.sw) (16-bit, 8 fractional bits)
template <int CH>
__device__ void vertical(const PlaneView &P, int j, uint16_t *t)
{
    int i0, n;
    mvrs::span(P.sh, P.dh, j, i0, n);
    const int mis = P.x0 & (CH - 1);                     // the row starts are CH-aligned: every tap row has the same offset
    const int nch = (mis + P.sw + CH - 1) / CH;
    const uint8_t *base = P.base + (size_t)(P.y0 + i0) * P.pitch + (P.x0 - mis);
    for (int c = threadIdx.x; c < nch; c += kThreads) {
        uint32_t acc[CH];
#pragma unroll
        for (int b = 0; b < CH; b++) acc[b] = 0;
        const uint8_t *p = base + c * CH;
        int k = 0;
        for (; k + 4 <= n; k += 4) {   // four tap rows in flight
            Strip<CH> s[4];
#pragma unroll
            for (int q = 0; q < 4; q++) s[q].load(p + (size_t)(k + q) * P.pitch);
#pragma unroll
            for (int q = 0; q < 4; q++) mac<CH>(acc, s[q], (uint32_t)mvrs::weight(P.sh, P.dh, j, i0 + k + q));
        }
        for (; k < n; k++) {
            Strip<CH> s;
            s.load(p + (size_t)k * P.pitch);
            mac<CH>(acc, s, (uint32_t)mvrs::weight(P.sh, P.dh, j, i0 + k));
        }
#pragma unroll
        for (int b = 0; b < CH; b++) {
            const int col = c * CH - mis + b;
            if (col >= 0 && col < P.sw) t[col] = (uint16_t)mvrs::round_v(acc[b]);
        }
    }
}

// horizontal taps of the intermediate row t -> one output row (bytes, LDS)
__device__ void horizontal(const PlaneView &P, const uint16_t *t, uint8_t *out)
{
    if (P.dw == P.sw) {   // one tap of 2^14: (t 2^14 + 2^21) >> 22 = (t + 128) >> 8
        for (int x = threadIdx.x; x < P.dw; x += kThreads) out[x] = (uint8_t)((t[x] + 128u) >> 8);
        return;
    }
    for (int x = threadIdx.x; x < P.dw; x += kThreads) {
        int i0, n;
        mvrs::span(P.sw, P.dw, x, i0, n);
        uint32_t acc = 0;
        int f0 = mvrs::cum(P.sw, P.dw, x, i0);
        for (int k = 0; k < n; k++) {
            const int f1 = mvrs::cum(P.sw, P.dw, x, i0 + k + 1);
            acc += (uint32_t)(f1 - f0) * t[i0 + k];
            f0 = f1;
        }
        out[x] = (uint8_t)mvrs::round_h(acc);
    }
}

// `len` staged bytes -> global memory: a byte head up to the first 4-byte boundary, dwords, a byte tail
__device__ void copy_out(uint8_t *dst, const uint8_t *s, int len)
{
    const int head = min(len, (int)((4u - ((uint32_t)(uintptr_t)dst & 3u)) & 3u));
    const int body = (len - head) >> 2;
    for (int k = threadIdx.x; k < body; k += kThreads) {
        const int o = head + 4 * k;
        *reinterpret_cast<uint32_t *>(dst + o) = (uint32_t)s[o] | ((uint32_t)s[o + 1] << 8) | ((uint32_t)s[o + 2] << 16) |
                                                 ((uint32_t)s[o + 3] << 24);
    }
    for (int o = head + 4 * body + (int)threadIdx.x; o < len; o += kThreads) dst[o] = s[o];
    if ((int)threadIdx.x < head) dst[threadIdx.x] = s[threadIdx.x];
}

__global__ __launch_bounds__(256) void resample_kernel(ResampleArgs a)
{
    extern __shared__ __attribute__((aligned(16))) uint8_t lds[];
    const int pic = blockIdx.y;
    const int Wp = a.width_mbs * 16, Hp = a.height_mbs * 16;
    const int ow = a.ow, oh = a.oh, cow = ow >> 1, coh = oh >> 1;
    const int r0 = blockIdx.x * a.band;                 // first chroma output row of the band
    const int nr = min(a.band, coh - r0);
    if (nr <= 0) return;
    const uint8_t *src = a.src + (size_t)pic * ((size_t)Wp * Hp * 3 / 2);
    uint16_t *t = reinterpret_cast<uint16_t *>(lds);
    uint8_t *sy = lds + (((size_t)a.cw * 2 + 15) & ~(size_t)15);   // 2 band rows of ow
    uint8_t *scb = sy + (size_t)2 * a.band * ow;                     // band rows of ow / 2
    uint8_t *scr = scb + (size_t)a.band * cow;

    const PlaneView L{src, Wp, a.cx, a.cy, a.cw, a.ch, ow, oh};
    for (int r = 0; r < 2 * nr; r++) {
        vertical<16>(L, 2 * r0 + r, t);
        __syncthreads();
        horizontal(L, t, sy + r * ow);
        __syncthreads();
    }
    for (int pl = 0; pl < 2; pl++) {
        const PlaneView C{src + (size_t)Wp * Hp + (size_t)pl * (Wp >> 1) * (Hp >> 1), Wp >> 1, a.cx >> 1, a.cy >> 1,
                          a.cw >> 1, a.ch >> 1, cow, coh};
        uint8_t *st = pl ? scr : scb;
        for (int r = 0; r < nr; r++) {
            vertical<8>(C, r0 + r, t);
            __syncthreads();
            horizontal(C, t, st + r * cow);
            __syncthreads();
        }
    }
    if (a.yuv) {
        uint8_t *o = a.yuv + (size_t)pic * ((size_t)ow * oh * 3 / 2);
        copy_out(o + (size_t)2 * r0 * ow, sy, 2 * nr * ow);
        copy_out(o + (size_t)ow * oh + (size_t)r0 * cow, scb, nr * cow);
        copy_out(o + (size_t)ow * oh + (size_t)cow * coh + (size_t)r0 * cow, scr, nr * cow);
    }
    if (a.rgb) {
        // four samples per lane (the last group of a row whose width is 2 mod 4 has two); a group starts at an even byte
        uint8_t *o = a.rgb + (size_t)pic * ((size_t)ow * oh * 3);
        const int groups = (ow + 3) >> 2;
        for (int k = threadIdx.x; k < 2 * nr * groups; k += kThreads) {
            const int r = k / groups, g = k - r * groups, x = 4 * g;
            const bool four = x + 4 <= ow;
            const uint8_t *ly = sy + r * ow + x;
            const uint8_t *cb = scb + (r >> 1) * cow + 2 * g, *cr = scr + (r >> 1) * cow + 2 * g;
            const uint32_t yw = (uint32_t)ly[0] | ((uint32_t)ly[1] << 8) | (four ? ((uint32_t)ly[2] << 16) | ((uint32_t)ly[3] << 24) : 0u);
            const u16x2 cbv = {(unsigned short)cb[0], (unsigned short)(four ? cb[1] : 0)};
            const u16x2 crv = {(unsigned short)cr[0], (unsigned short)(four ? cr[1] : 0)};
            int d0, d1, d2;
            rgb4(yw, cbv, crv, d0, d1, d2);
            uint8_t *dst = o + ((size_t)(2 * r0 + r) * ow + x) * 3;
            const uint32_t w0 = (uint32_t)d0, w1 = (uint32_t)d1, w2 = (uint32_t)d2;
            if (((uintptr_t)dst & 3) == 0) {
                *reinterpret_cast<uint32_t *>(dst) = w0;
                if (four) {
                    *reinterpret_cast<uint32_t *>(dst + 4) = w1;
                    *reinterpret_cast<uint32_t *>(dst + 8) = w2;
                } else {
                    *reinterpret_cast<uint16_t *>(dst + 4) = (uint16_t)w1;
                }
            } else {   // 2 mod 4
                *reinterpret_cast<uint16_t *>(dst) = (uint16_t)w0;
                *reinterpret_cast<uint32_t *>(dst + 2) = (w0 >> 16) | (w1 << 16);
                if (four) {
                    *reinterpret_cast<uint32_t *>(dst + 6) = (w1 >> 16) | (w2 << 16);
                    *reinterpret_cast<uint16_t *>(dst + 10) = (uint16_t)(w2 >> 16);
                }
            }
        }
    }
}

} // namespace

size_t resample_lds_bytes(int cw, int ow, int band)
{
    return (((size_t)cw * 2 + 15) & ~(size_t)15) + (size_t)3 * band * ow;
}

hipError_t launch_resample(const ResampleArgs &a, hipStream_t stream)
{
    const size_t lds = resample_lds_bytes(a.cw, a.ow, a.band);
    hipError_t e = hipFuncSetAttribute((const void *)resample_kernel, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds);
    if (e != hipSuccess) return e;
    const int bands = (a.oh / 2 + a.band - 1) / a.band;
    for (int first = 0; first < a.n_frames; first += 65535) {   // (grid y is at most 65535)
        ResampleArgs b = a;
        const int n = min(65535, a.n_frames - first);
        const size_t coded = (size_t)a.width_mbs * a.height_mbs * 384;
        b.src = a.src + (size_t)first * coded;
        b.yuv = a.yuv ? a.yuv + (size_t)first * ((size_t)a.ow * a.oh * 3 / 2) : nullptr;
        b.rgb = a.rgb ? a.rgb + (size_t)first * ((size_t)a.ow * a.oh * 3) : nullptr;
        b.n_frames = n;
        hipLaunchKernelGGL(resample_kernel, dim3((unsigned)bands, (unsigned)n), dim3(kThreads), lds, stream, b);
        e = hipGetLastError();
        if (e != hipSuccess) return e;
    }
    return hipSuccess;
}

} // namespace mvhp
