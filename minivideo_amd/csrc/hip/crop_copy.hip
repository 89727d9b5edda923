// crop_copy.hip -- crop only (out_w == crop_w, out_h == crop_h) as a copy: coded planes -> the cropped planes and / or the RGB of
// the cropped picture, global memory to global memory, gfx950.  The general pass (resample.hip) gives the same bytes for such a
// geometry (one tap of 2^14 per axis is an exact copy) through its LDS row buffers; this kernel has no LDS, no tap arithmetic
// and no limit on the width.
//
// Mapping: one workgroup of 256 threads per (picture, band of `band` chroma rows = 2 band luma rows).  An output plane is
// one contiguous run of bytes (its pitch is its width), so a row starts at any byte: the row is cut at the 16-byte boundaries
// of the DESTINATION.  A lane owns one such block of one row -- consecutive lanes consecutive blocks, a wave writes one
// contiguous run -- and stores it with one aligned dwordx4; its source bytes are loaded as aligned dwords (a source row is 16-
// or 8-byte aligned, the crop offset is not) and shifted into place in registers (v_alignbyte).  The blocks a row only
// partly covers, its head and its tail, are written byte by byte by the lanes that own them: once per row.
// RGB: a lane owns the 16 samples whose 48 bytes of RGB start on a 16-byte boundary (an even sample, because rows of RGB
// start on even bytes), converts them with the packed helpers of recon_batch_device.h -- chroma 2x2-nearest relative to the
// CROPPED picture -- and stores three aligned dwordx4; head and tail samples go out in pairs.
// Stateless: nothing crosses workgroups, no waits, no inline assembly -- safe under stream capture.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "recon_batch_device.h"
#include "recon_kernels.h"

namespace mvhp {

namespace {

constexpr int kThreads = 256;

// dword-aligned loads of two / four dwords (the address is a multiple of 4, not of 8 / 16)
struct __attribute__((packed, aligned(4))) Dwords4 { uint32_t w[4]; };
struct __attribute__((packed, aligned(4))) Dwords2 { uint32_t w[2]; };

// the 16 bytes at p (any alignment), from the aligned dwords that hold them: every dword read contains a byte of [p, p + 16)
__device__ __forceinline__ uint4 load16(const uint8_t *p)
{
    const uint32_t sh = (uint32_t)(uintptr_t)p & 3u;
    const uint8_t *q = p - sh;
    const Dwords4 a = *reinterpret_cast<const Dwords4 *>(q);
    uint32_t w4 = 0;
    if (sh) w4 = *reinterpret_cast<const uint32_t *>(q + 16);
    return uint4{__builtin_amdgcn_alignbyte(a.w[1], a.w[0], sh), __builtin_amdgcn_alignbyte(a.w[2], a.w[1], sh),
                 __builtin_amdgcn_alignbyte(a.w[3], a.w[2], sh), __builtin_amdgcn_alignbyte(w4, a.w[3], sh)};
}

// ... the 8 bytes at p
__device__ __forceinline__ uint2 load8(const uint8_t *p)
{
    const uint32_t sh = (uint32_t)(uintptr_t)p & 3u;
    const uint8_t *q = p - sh;
    const Dwords2 a = *reinterpret_cast<const Dwords2 *>(q);
    uint32_t w2 = 0;
    if (sh) w2 = *reinterpret_cast<const uint32_t *>(q + 8);
    return uint2{__builtin_amdgcn_alignbyte(a.w[1], a.w[0], sh), __builtin_amdgcn_alignbyte(w2, a.w[1], sh)};
}

// How the workgroup's lanes map onto (row, block) of rows that hold up to `slots` blocks: lanes [0, tx_n) of a group walk the
// blocks, ny groups take rows side by side.  One division per lane and plane, none per block.
struct LaneMap {
    int tx, ty, tx_n, ny;
    __device__ explicit LaneMap(int slots)
    {
        tx_n = min(slots, kThreads);
        ny = kThreads / tx_n;
        ty = (int)threadIdx.x / tx_n;
        tx = (int)threadIdx.x - ty * tx_n;
        if (ty >= ny) ty = -1;   // (the lanes behind the last whole group idle)
    }
};

// rows [0, nrows) of `len` bytes: source row r at s + r * spitch, destination row r at d + r * len
__device__ void copy_rows(uint8_t *d, const uint8_t *s, int spitch, int len, int nrows)
{
    const int slots = ((len + 15) >> 4) + 1;   // blocks a row can touch: ((d & 15) + len + 15) / 16 at most
    const LaneMap m(slots);
    if (m.ty < 0) return;
    for (int r = m.ty; r < nrows; r += m.ny) {
        uint8_t *dr = d + (size_t)r * len;
        const uint8_t *sr = s + (size_t)r * spitch;
        const int a = (int)((uintptr_t)dr & 15);
        for (int j = m.tx; j < slots; j += m.tx_n) {
            const int b0 = 16 * j - a;   // offset, in the row, of the block's first byte
            if (b0 >= len) break;
            if (b0 >= 0 && b0 + 16 <= len) {
                *reinterpret_cast<uint4 *>(dr + b0) = load16(sr + b0);
            } else {   // head or tail of the row
                const int e = min(b0 + 16, len);
                for (int b = max(b0, 0); b < e; b++) dr[b] = sr[b];
            }
        }
    }
}

// rows [0, nrows) of `w` samples -> RGB: luma row r at y + r * ypitch, chroma row r >> 1 at cb / cr + (r >> 1) * cpitch (the
// first row is an even row of the cropped picture), RGB row r at d + r * 3 w
__device__ void rgb_rows(uint8_t *d, const uint8_t *y, int ypitch, const uint8_t *cb, const uint8_t *cr, int cpitch, int w,
                         int nrows)
{
    const int slots = ((w + 15) >> 4) + 1;
    const LaneMap m(slots);
    if (m.ty < 0) return;
    for (int r = m.ty; r < nrows; r += m.ny) {
        uint8_t *dr = d + (size_t)r * w * 3;
        const uint8_t *yr = y + (size_t)r * ypitch;
        const uint8_t *cbr = cb + (size_t)(r >> 1) * cpitch, *crr = cr + (size_t)(r >> 1) * cpitch;
        // the first sample whose RGB starts a 16-byte block: 3 ph = -dr (mod 16), 3 * 11 = 1 (mod 16); dr is even, so is ph
        const int ph = (int)((0u - (uint32_t)(uintptr_t)dr) * 11u & 15u);
        for (int j = m.tx; j < slots; j += m.tx_n) {
            const int x0 = ph - 16 + 16 * j;   // block j: samples [x0, x0 + 16)
            if (x0 >= w) break;
            if (x0 >= 0 && x0 + 16 <= w) {
                v4i o0, o1, o2;
                rgb16(load16(yr + x0), load8(cbr + (x0 >> 1)), load8(crr + (x0 >> 1)), o0, o1, o2);
                v4i *o = reinterpret_cast<v4i *>(dr + (size_t)x0 * 3);
                o[0] = o0; o[1] = o1; o[2] = o2;
            } else {   // head or tail: pairs of samples (one chroma sample each), six bytes at an even address
                const int e = min(x0 + 16, w);
                for (int x = max(x0, 0); x < e; x += 2) {
                    const uint32_t yw = (uint32_t)yr[x] | ((uint32_t)yr[x + 1] << 8);
                    const u16x2 cbv = {(unsigned short)cbr[x >> 1], (unsigned short)0};
                    const u16x2 crv = {(unsigned short)crr[x >> 1], (unsigned short)0};
                    int d0, d1, d2;
                    rgb4(yw, cbv, crv, d0, d1, d2);   // d0 = R0 G0 B0 R1, d1 = G1 B1 . .
                    uint16_t *o = reinterpret_cast<uint16_t *>(dr + (size_t)x * 3);
                    o[0] = (uint16_t)d0; o[1] = (uint16_t)((uint32_t)d0 >> 16); o[2] = (uint16_t)d1;
                }
            }
        }
    }
}

__global__ __launch_bounds__(256) void crop_copy_kernel(ResampleArgs a)
{
    const int pic = blockIdx.y;
    const int Wp = a.width_mbs * 16, Hp = a.height_mbs * 16;
    const int cw = a.cw, ch = a.ch, ccw = cw >> 1, cch = ch >> 1;
    const int r0 = blockIdx.x * a.band;   // first chroma row of the band
    const int nr = min(a.band, cch - r0);
    if (nr <= 0) return;
    const uint8_t *src = a.src + (size_t)pic * ((size_t)Wp * Hp * 3 / 2);
    const uint8_t *sy = src + (size_t)(a.cy + 2 * r0) * Wp + a.cx;
    const uint8_t *scb = src + (size_t)Wp * Hp + (size_t)((a.cy >> 1) + r0) * (Wp >> 1) + (a.cx >> 1);
    const uint8_t *scr = scb + (size_t)(Wp >> 1) * (Hp >> 1);
    if (a.yuv) {
        uint8_t *o = a.yuv + (size_t)pic * ((size_t)cw * ch * 3 / 2);
        copy_rows(o + (size_t)2 * r0 * cw, sy, Wp, cw, 2 * nr);
        copy_rows(o + (size_t)cw * ch + (size_t)r0 * ccw, scb, Wp >> 1, ccw, nr);
        copy_rows(o + (size_t)cw * ch + (size_t)ccw * cch + (size_t)r0 * ccw, scr, Wp >> 1, ccw, nr);
    }
    if (a.rgb) {
        uint8_t *o = a.rgb + (size_t)pic * ((size_t)cw * ch * 3);
        rgb_rows(o + (size_t)2 * r0 * cw * 3, sy, Wp, scb, scr, Wp >> 1, cw, 2 * nr);
    }
}

} // namespace

// a.ow == a.cw and a.oh == a.ch; a.band = chroma rows per workgroup
hipError_t launch_crop_copy(const ResampleArgs &a, hipStream_t stream)
{
    const int bands = (a.ch / 2 + a.band - 1) / a.band;
    for (int first = 0; first < a.n_frames; first += 65535) {   // (grid y is at most 65535)
        ResampleArgs b = a;
        const int n = min(65535, a.n_frames - first);
        const size_t coded = (size_t)a.width_mbs * a.height_mbs * 384;
        b.src = a.src + (size_t)first * coded;
        b.yuv = a.yuv ? a.yuv + (size_t)first * ((size_t)a.cw * a.ch * 3 / 2) : nullptr;
        b.rgb = a.rgb ? a.rgb + (size_t)first * ((size_t)a.cw * a.ch * 3) : nullptr;
        b.n_frames = n;
        hipLaunchKernelGGL(crop_copy_kernel, dim3((unsigned)bands, (unsigned)n), dim3(kThreads), 0, stream, b);
        const hipError_t e = hipGetLastError();
        if (e != hipSuccess) return e;
    }
    return hipSuccess;
}

} // namespace mvhp
