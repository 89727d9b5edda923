// color_convert.hip -- RGB from dense planar 4:2:0 pictures by the matrix, range and chroma siting the stream names, gfx950
// (include/minivideo_hotpath.h "Colour conversion"; tests/color_ref.py restates the arithmetic).  Integers only:
//     y' = 16 cy (Y - yoff) + 2^17,   cb = Cb16 - 2048,   cr = Cr16 - 2048   (chroma in sixteenths of a sample)
//     R = clamp8((y' + crv cr) >> 18)   G = clamp8((y' - gcb cb - gcr cr) >> 18)   B = clamp8((y' + cbu cb) >> 18)
// |y'| < 7.4e7 and every chroma term < 7.1e7: int32 throughout.
//
// A workgroup owns a band of chroma rows of one picture, that is twice as many luma and RGB rows.  The write side is the one of
// the other output kernels (orient.hip, crop_copy.hip): an RGB row is cut at the 16-byte boundaries of the DESTINATION, a lane
// owns 16 samples whose 48 bytes start at such a boundary and stores them with three aligned dwordx4; the samples a row has in
// front of its first boundary and behind its last go out as pairs, six bytes at an even address.  Luma comes with one 16-byte
// load per lane (aligned dwords shifted into place).
// Chroma is staged ONCE per band into LDS with 16-byte loads and stores: every chroma row serves two luma rows (four with the
// blend), and a lane's eight chroma samples lie at any byte phase, which LDS reads absorb better than memory does (measured on
// the NEAREST form, 2048 x 1080p: 6.40 ms with its chroma straight from memory, 6.00 ms staged).
//   MVHP_CHROMA_NEAREST: the band's own chroma rows; a lane reads eight samples per plane (three dwords, shifted into place).
//   MVHP_CHROMA_LEFT / _CENTER: a luma row blends two chroma rows, so rows r0 - 1 .. r0 + band are staged, clamped at the plane's
//     top and bottom, column -1 and column cw filled with the edge samples: the blend behind the barrier has no edge cases.  A
//     lane reads the ten samples of its block from two rows (four dwords each, shifted into place), blends vertically (weights
//     1 3 / 3 1, values <= 1020) and then horizontally.
// The band shrinks where a row is long: the staged rows of two planes stay below 60 KB.
// Stateless: nothing crosses workgroups, no waits, no inline assembly -- safe under stream capture and across streams.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "minivideo_hotpath.h"
#include "recon_kernels.h"

namespace mvhp {

namespace {

constexpr int kThreads = 256;
constexpr int kLead = 16;            // bytes in front of column 0 of a staged row (column -1 is byte 15)
constexpr int kLdsBudget = 60000;    // of the 64 KB a workgroup may ask for

struct __attribute__((packed, aligned(4))) Dwords4 { uint32_t w[4]; };
typedef uint32_t u32x4 __attribute__((ext_vector_type(4)));

// the 16 bytes at p (any alignment), from the aligned dwords that hold them; `end` = the dword-aligned end of what may be read:
// the last bytes of the last picture come one by one (orient.hip has the same reader)
__device__ __forceinline__ uint4 load16(const uint8_t *p, const uint8_t *end)
{
    const uint32_t sh = (uint32_t)(uintptr_t)p & 3u;
    const uint8_t *q = p - sh;
    if (q + (sh ? 20 : 16) > end) {
        uint32_t w[4] = {0, 0, 0, 0};
        for (int i = 0; i < 16; i++) w[i >> 2] |= (uint32_t)p[i] << (8 * (i & 3));
        return uint4{w[0], w[1], w[2], w[3]};
    }
    const Dwords4 a = *reinterpret_cast<const Dwords4 *>(q);
    uint32_t w4 = 0;
    if (sh) w4 = *reinterpret_cast<const uint32_t *>(q + 16);
    return uint4{__builtin_amdgcn_alignbyte(a.w[1], a.w[0], sh), __builtin_amdgcn_alignbyte(a.w[2], a.w[1], sh),
                 __builtin_amdgcn_alignbyte(a.w[3], a.w[2], sh), __builtin_amdgcn_alignbyte(w4, a.w[3], sh)};
}

// the 8 bytes at byte address p of LDS (any alignment; a staged row has room behind its samples)
__device__ __forceinline__ uint2 lds8(const uint8_t *p)
{
    const uint32_t sh = (uint32_t)(uintptr_t)p & 3u;
    const uint32_t *q = reinterpret_cast<const uint32_t *>(p - sh);
    const uint32_t w0 = q[0], w1 = q[1], w2 = q[2];
    return uint2{__builtin_amdgcn_alignbyte(w1, w0, sh), __builtin_amdgcn_alignbyte(w2, w1, sh)};
}

__device__ __forceinline__ uint32_t byte_of(uint32_t w, int i) { return (w >> (8 * i)) & 255u; }
// clamp8(v >> 18): the clamp comes FIRST, on the unshifted value, and the shift is a logical one of a non-negative number -- the
// same result as clamping the shifted value.  (Written the other way round, shift then clamp, two channels of a dword are matched
// to gfx950's pack-with-saturation shift, whose result this compiler then ORs into a dword as if the upper half-word were zero;
// on the device it is not, and stray bits land in bytes 2 and 3 of the dword.)
__device__ __forceinline__ uint32_t shift_clamp8(int v) { return (uint32_t)min(max(v, 0), (256 << 18) - 1) >> 18; }

// one sample: luma Y and chroma in sixteenths -> R | G << 8 | B << 16
__device__ __forceinline__ uint32_t pixel(const ColorConvertArgs &a, uint32_t Y, int cb16, int cr16)
{
    const int yp = a.ymul * ((int)Y - a.yoff) + (1 << 17);
    const int cb = cb16 - 2048, cr = cr16 - 2048;
    const uint32_t r = shift_clamp8(yp + a.crv * cr);
    const uint32_t g = shift_clamp8(yp - a.gcb * cb - a.gcr * cr);
    const uint32_t b = shift_clamp8(yp + a.cbu * cb);
    return r | (g << 8) | (b << 16);
}

// the horizontal blend of the even and the odd sample of chroma column i of v[] (v[0] = the column in front of the block's first)
template <int SITING>
__device__ __forceinline__ void blend_h(const int *v, int i, int &even, int &odd)
{
    if (SITING == MVHP_CHROMA_LEFT) {
        even = 4 * v[i];
        odd = 2 * v[i] + 2 * v[i + 1];
    } else {
        even = v[i - 1] + 3 * v[i];
        odd = 3 * v[i] + v[i + 1];
    }
}

// the ten samples from byte address `p` of LDS on (any alignment), blended: out[i] = wa * rowa[i] + wb * rowb[i]
__device__ __forceinline__ void blend_v10(const uint8_t *pa, const uint8_t *pb, int wa, int wb, int *out)
{
    const uint32_t sh = (uint32_t)(uintptr_t)pa & 3u;   // (rows are a multiple of 16 bytes apart: pb has the same phase)
    const uint32_t *qa = reinterpret_cast<const uint32_t *>(pa - sh), *qb = reinterpret_cast<const uint32_t *>(pb - sh);
    const uint32_t a0 = qa[0], a1 = qa[1], a2 = qa[2], a3 = qa[3], b0 = qb[0], b1 = qb[1], b2 = qb[2], b3 = qb[3];
    const uint32_t ra[3] = {__builtin_amdgcn_alignbyte(a1, a0, sh), __builtin_amdgcn_alignbyte(a2, a1, sh), __builtin_amdgcn_alignbyte(a3, a2, sh)};
    const uint32_t rb[3] = {__builtin_amdgcn_alignbyte(b1, b0, sh), __builtin_amdgcn_alignbyte(b2, b1, sh), __builtin_amdgcn_alignbyte(b3, b2, sh)};
#pragma unroll
    for (int i = 0; i < 10; i++) out[i] = wa * (int)byte_of(ra[i >> 2], i & 3) + wb * (int)byte_of(rb[i >> 2], i & 3);
}

// 16 samples -> 48 bytes at o (16-byte aligned)
__device__ __forceinline__ void store48(uint8_t *o, const uint32_t *px)
{
    uint32_t w[12];
#pragma unroll
    for (int g = 0; g < 4; g++) {   // four samples = three dwords
        const uint32_t p0 = px[4 * g], p1 = px[4 * g + 1], p2 = px[4 * g + 2], p3 = px[4 * g + 3];
        w[3 * g] = p0 | (p1 << 24);
        w[3 * g + 1] = (p1 >> 8) | (p2 << 16);
        w[3 * g + 2] = (p2 >> 16) | (p3 << 8);
    }
    // (native vectors: each line stays one aligned dwordx4 store; as structs of four members the twelve dwords of the NEAREST
    //  form were regrouped into stores of 16, 12, 12 and 8 bytes: 6.00 ms for 2048 x 1080p instead of 4.77 ms)
    u32x4 *d = reinterpret_cast<u32x4 *>(o);
    d[0] = u32x4{w[0], w[1], w[2], w[3]};
    d[1] = u32x4{w[4], w[5], w[6], w[7]};
    d[2] = u32x4{w[8], w[9], w[10], w[11]};
}

// two samples -> six bytes at o (even address)
__device__ __forceinline__ void store6(uint8_t *o, uint32_t p0, uint32_t p1)
{
    uint16_t *d = reinterpret_cast<uint16_t *>(o);
    d[0] = (uint16_t)p0;
    d[1] = (uint16_t)((p0 >> 16) | (p1 << 8));
    d[2] = (uint16_t)(p1 >> 8);
}

// How the workgroup's lanes map onto (row, block) of rows that hold up to `slots` blocks (crop_copy.hip)
struct LaneMap {
    int tx, ty, tx_n, ny;
    __device__ explicit LaneMap(int slots)
    {
        tx_n = min(slots, kThreads);
        ny = kThreads / tx_n;
        ty = (int)threadIdx.x / tx_n;
        tx = (int)threadIdx.x - ty * tx_n;
        if (ty >= ny) ty = -1;
    }
};

template <int SITING>
__global__ __launch_bounds__(256) void color_kernel(ColorConvertArgs a)
{
    extern __shared__ __attribute__((aligned(16))) uint8_t lds[];
    const int pic = blockIdx.y;
    const int w = a.w, h = a.h, cw = w >> 1, ch = h >> 1;
    const int r0 = blockIdx.x * a.band;   // first chroma row of the band
    const int nr = min(a.band, ch - r0);
    if (nr <= 0) return;
    const uint8_t *src = a.yuv + (size_t)pic * ((size_t)w * h * 3 / 2);
    const uint8_t *scb = src + (size_t)w * h, *scr = scb + (size_t)cw * ch;
    uint8_t *dst = a.rgb + (size_t)pic * ((size_t)w * h * 3);
    const int P = ((cw + 15) & ~15) + 2 * kLead;   // staged row: 16 bytes, the samples, at least 16 bytes a block read may run over
    constexpr int HALO = SITING == MVHP_CHROMA_NEAREST ? 0 : 1;   // chroma rows staged above and below the band's own
    const int plane = (a.band + 2 * HALO) * P;     // of the second plane in LDS

    {   // chroma rows r0 - HALO .. r0 + nr - 1 + HALO, clamped, into LDS rows 0 .. nr - 1 + 2 HALO
        const int rows = nr + 2 * HALO;
        const int nch = (cw + 15) >> 4;
        const int units = 2 * rows * nch;
        for (int u = threadIdx.x; u < units; u += kThreads) {
            const int pl = u / (rows * nch), v = u - pl * rows * nch;
            const int lr = v / nch, i = v - lr * nch;
            const int jr = min(max(r0 - HALO + lr, 0), ch - 1);
            const uint8_t *s = (pl ? scr : scb) + (size_t)jr * cw;
            uint8_t *d = lds + pl * plane + lr * P + kLead;
            if (16 * i + 16 <= cw) {
                *reinterpret_cast<uint4 *>(d + 16 * i) = load16(s + 16 * i, a.yuv_end);
            } else {
                for (int k = 16 * i; k < cw; k++) d[k] = s[k];
            }
            if (i == 0) d[-1] = s[0];
            if (i == nch - 1) d[cw] = s[cw - 1];
        }
        __syncthreads();
    }

    const int slots = ((w + 15) >> 4) + 1;
    const LaneMap m(slots);
    if (m.ty < 0) return;
    for (int r = m.ty; r < 2 * nr; r += m.ny) {
        const int y = 2 * r0 + r, j = y >> 1;
        const uint8_t *sy = src + (size_t)y * w;
        uint8_t *dr = dst + (size_t)y * w * 3;
        // NEAREST: the staged row j.  LEFT / CENTER: two staged rows and their weights (y even: j - 1, j with 1, 3; y odd: j,
        // j + 1 with 3, 1).  The LDS row of chroma row jr is jr - r0 + HALO
        const int la = HALO == 0 ? j - r0 : (y & 1) ? j - r0 + 1 : j - r0, wa = (y & 1) ? 3 : 1, wb = 4 - wa;
        const uint8_t *lcb = lds + la * P + kLead, *lcr = lcb + plane;
        // the first sample whose RGB starts a 16-byte block: 3 ph = -dr (mod 16), 3 * 11 = 1 (mod 16); dr is even, so is ph
        const int ph = (int)((0u - (uint32_t)(uintptr_t)dr) * 11u & 15u);
        for (int jb = m.tx; jb < slots; jb += m.tx_n) {
            const int x0 = ph - 16 + 16 * jb;
            if (x0 >= w) break;
            if (x0 >= 0 && x0 + 16 <= w) {
                const int k0 = x0 >> 1;
                const uint4 yv = load16(sy + x0, a.yuv_end);
                const uint32_t yw[4] = {yv.x, yv.y, yv.z, yv.w};
                uint32_t px[16];
                if (SITING == MVHP_CHROMA_NEAREST) {
                    const uint2 cbv = lds8(lcb + k0), crv = lds8(lcr + k0);
                    const uint32_t cbw[2] = {cbv.x, cbv.y}, crw[2] = {crv.x, crv.y};
#pragma unroll
                    for (int q = 0; q < 8; q++) {
                        const int cb16 = 16 * (int)byte_of(cbw[q >> 2], q & 3), cr16 = 16 * (int)byte_of(crw[q >> 2], q & 3);
                        px[2 * q] = pixel(a, byte_of(yw[q >> 1], (2 * q) & 3), cb16, cr16);
                        px[2 * q + 1] = pixel(a, byte_of(yw[q >> 1], (2 * q + 1) & 3), cb16, cr16);
                    }
                } else {
                    int vb[10], vr[10];   // columns k0 - 1 .. k0 + 8, blended vertically
                    blend_v10(lcb + k0 - 1, lcb + P + k0 - 1, wa, wb, vb);
                    blend_v10(lcr + k0 - 1, lcr + P + k0 - 1, wa, wb, vr);
#pragma unroll
                    for (int q = 0; q < 8; q++) {
                        int be, bo, re, ro;
                        blend_h<SITING>(vb, q + 1, be, bo);
                        blend_h<SITING>(vr, q + 1, re, ro);
                        px[2 * q] = pixel(a, byte_of(yw[q >> 1], (2 * q) & 3), be, re);
                        px[2 * q + 1] = pixel(a, byte_of(yw[q >> 1], (2 * q + 1) & 3), bo, ro);
                    }
                }
                store48(dr + (size_t)x0 * 3, px);
            } else {   // head or tail: pairs of samples, six bytes at an even address
                const int e = min(x0 + 16, w);
                for (int x = max(x0, 0); x < e; x += 2) {
                    const int k = x >> 1;
                    int be, bo, re, ro;
                    if (SITING == MVHP_CHROMA_NEAREST) {
                        be = bo = 16 * (int)lcb[k];
                        re = ro = 16 * (int)lcr[k];
                    } else {
                        int vb[3], vr[3];   // columns k - 1, k, k + 1 (the staged rows hold the edge samples at -1 and cw)
                        for (int i = 0; i < 3; i++) {
                            vb[i] = wa * (int)lcb[k - 1 + i] + wb * (int)lcb[P + k - 1 + i];
                            vr[i] = wa * (int)lcr[k - 1 + i] + wb * (int)lcr[P + k - 1 + i];
                        }
                        blend_h<SITING>(vb, 1, be, bo);
                        blend_h<SITING>(vr, 1, re, ro);
                    }
                    store6(dr + (size_t)x * 3, pixel(a, sy[x], be, re), pixel(a, sy[x + 1], bo, ro));
                }
            }
        }
    }
}

} // namespace

hipError_t launch_color_convert(const ColorConvertArgs &a0, hipStream_t stream)
{
    ColorConvertArgs a = a0;
    const int cw = a.w >> 1, ch = a.h >> 1;
    const int P = ((cw + 15) & ~15) + 2 * kLead;
    if (a.band < 1) a.band = 1;
    const int halo2 = a.siting == MVHP_CHROMA_NEAREST ? 0 : 2;
    while (a.band > 1 && (size_t)(a.band + halo2) * P * 2 > (size_t)kLdsBudget) a.band /= 2;
    const size_t lds = (size_t)(a.band + halo2) * P * 2;   // (16 384 wide, blended: 3 rows of 8224 bytes, two planes = 49 344)
    const unsigned gx = (unsigned)((ch + a.band - 1) / a.band);
    const size_t yuv_pic = (size_t)a.w * a.h * 3 / 2, rgb_pic = (size_t)a.w * a.h * 3;
    for (int first = 0; first < a.n; first += 65535) {   // (grid y is at most 65535)
        ColorConvertArgs b = a;
        b.n = min(65535, a.n - first);
        b.yuv = a.yuv + (size_t)first * yuv_pic;
        b.rgb = a.rgb + (size_t)first * rgb_pic;
        const dim3 grid(gx, (unsigned)b.n), block(kThreads);
        if (a.siting == MVHP_CHROMA_NEAREST) hipLaunchKernelGGL(color_kernel<MVHP_CHROMA_NEAREST>, grid, block, lds, stream, b);
        else if (a.siting == MVHP_CHROMA_LEFT) hipLaunchKernelGGL(color_kernel<MVHP_CHROMA_LEFT>, grid, block, lds, stream, b);
        else hipLaunchKernelGGL(color_kernel<MVHP_CHROMA_CENTER>, grid, block, lds, stream, b);
        const hipError_t e = hipGetLastError();
        if (e != hipSuccess) return e;
    }
    return hipSuccess;
}

} // namespace mvhp
