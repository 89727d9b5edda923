// orient.hip -- display orientation: pictures turned by quarter turns (clockwise) into planes and / or the RGB of the turned
// planes, gfx950.  The source is either the crop rectangle of coded pictures or dense pictures as the resample pass leaves
// them; both are "a rectangle of w x h with a pitch", so one set of kernels serves both.
//
// For a source plane S of w x h and its output O (each plane with its own size):
//     1 turn:  O[y][x] = S[h-1-x][y]       2 turns: O[y][x] = S[h-1-y][w-1-x]       3 turns: O[y][x] = S[x][w-1-y]
// RGB is made from the turned planes (2x2-nearest chroma).  All sides are even, so a 2x2 chroma cell of the source is a 2x2 cell
// of the output: RGB of the turned planes equals the turned RGB of the source.
//
// The write side is the one of crop_copy.hip for every turn: an output row (or a tile's segment of one) is cut at the 16-byte
// boundaries of the DESTINATION, a lane owns one such block and stores it with one aligned dwordx4; the blocks a segment only
// partly covers go out as aligned dwords where a whole dword lies inside the segment and as bytes for the at most three at
// either end.  What differs per turn is where a lane finds the 16 output bytes of its block (the "plane readers" below):
//   0 turns: in the source row, as crop_copy.hip loads them (aligned dwords shifted into place);
//   2 turns: in the source row read backwards -- 16 bytes loaded the same way and reversed in registers, no LDS;
//   1 and 3 turns: in LDS.  A workgroup owns one luma tile of 128 x 128 OUTPUT samples with its two chroma tiles of 64 x 64.  A
//     lane loads 16 bytes of each of four consecutive source rows (16-byte accesses along the SOURCE rows), transposes the four
//     4x4 byte blocks in registers (v_perm) and stores sixteen dwords, each four neighbours of one OUTPUT row.  Lanes are laid out
//     four blocks along a source row (64 contiguous bytes) by eight row groups per half-wave, and the LDS pitch is an odd number
//     of dwords (37 luma, 21 chroma): the stores of a half-wave then meet at most two to a bank, which a dword store absorbs.
//     Behind one barrier the tile leaves as contiguous runs per output row, read from LDS with 16-byte accesses.
// Stateless: nothing crosses workgroups, no waits, no inline assembly -- safe under stream capture and across streams.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "recon_batch_device.h"
#include "recon_kernels.h"

namespace mvhp {

namespace {

constexpr int kThreads = 256;
constexpr int kTile = 128;                    // luma samples per side of an output tile
constexpr int kPitchY = kTile + 20;           // 37 dwords: the tile, 16 bytes a block read may run over, odd dword count
constexpr int kPitchC = kTile / 2 + 20;       // 21 dwords
constexpr int kLdsY = kTile * kPitchY;
constexpr int kLdsC = (kTile / 2) * kPitchC;
constexpr int kLdsBytes = kLdsY + 2 * kLdsC + 32;

struct __attribute__((packed, aligned(4))) Dwords4 { uint32_t w[4]; };
struct __attribute__((packed, aligned(4))) Dwords2 { uint32_t w[2]; };

// the 16 bytes at p (any alignment), from the aligned dwords that hold them; `end` = the dword-aligned end of what may be read
// (a dense source ends where its last picture ends, which need not be a dword boundary): the last bytes come one by one
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

__device__ __forceinline__ uint2 load8(const uint8_t *p, const uint8_t *end)
{
    const uint32_t sh = (uint32_t)(uintptr_t)p & 3u;
    const uint8_t *q = p - sh;
    if (q + (sh ? 12 : 8) > end) {
        uint32_t w[2] = {0, 0};
        for (int i = 0; i < 8; i++) w[i >> 2] |= (uint32_t)p[i] << (8 * (i & 3));
        return uint2{w[0], w[1]};
    }
    const Dwords2 a = *reinterpret_cast<const Dwords2 *>(q);
    uint32_t w2 = 0;
    if (sh) w2 = *reinterpret_cast<const uint32_t *>(q + 8);
    return uint2{__builtin_amdgcn_alignbyte(a.w[1], a.w[0], sh), __builtin_amdgcn_alignbyte(w2, a.w[1], sh)};
}

// ---- plane readers: the bytes of OUTPUT rows [0, nrows) of one plane, wherever they are ----

struct FwdPlane {   // 0 turns: output (r, x) = p[r * pitch + x]
    const uint8_t *p, *end;
    int pitch;
    __device__ uint4 v16(int r, int x) const { return load16(p + (size_t)r * pitch + x, end); }
    __device__ uint2 v8(int r, int x) const { return load8(p + (size_t)r * pitch + x, end); }
    __device__ uint32_t v1(int r, int x) const { return p[(size_t)r * pitch + x]; }
};

struct RevPlane {   // 2 turns: output (r, x) = p[-(r * pitch + x)], p = the source sample of output (0, 0)
    const uint8_t *p, *end;
    int pitch;
    __device__ uint4 v16(int r, int x) const
    {
        const uint4 v = load16(p - (size_t)r * pitch - x - 15, end);
        return uint4{__builtin_bswap32(v.w), __builtin_bswap32(v.z), __builtin_bswap32(v.y), __builtin_bswap32(v.x)};
    }
    __device__ uint2 v8(int r, int x) const
    {
        const uint2 v = load8(p - (size_t)r * pitch - x - 7, end);
        return uint2{__builtin_bswap32(v.y), __builtin_bswap32(v.x)};
    }
    __device__ uint32_t v1(int r, int x) const { return *(p - (size_t)r * pitch - x); }
};

struct LdsPlane {   // 1 and 3 turns: the staged tile (the pitch leaves room for a block read to run over)
    const uint8_t *p;
    int pitch;
    __device__ uint4 v16(int r, int x) const
    {
        const uint8_t *a = p + r * pitch + x;
        const uint32_t sh = (uint32_t)(uintptr_t)a & 3u;
        const uint32_t *q = reinterpret_cast<const uint32_t *>(a - sh);
        const uint32_t w0 = q[0], w1 = q[1], w2 = q[2], w3 = q[3], w4 = q[4];
        return uint4{__builtin_amdgcn_alignbyte(w1, w0, sh), __builtin_amdgcn_alignbyte(w2, w1, sh),
                     __builtin_amdgcn_alignbyte(w3, w2, sh), __builtin_amdgcn_alignbyte(w4, w3, sh)};
    }
    __device__ uint2 v8(int r, int x) const
    {
        const uint8_t *a = p + r * pitch + x;
        const uint32_t sh = (uint32_t)(uintptr_t)a & 3u;
        const uint32_t *q = reinterpret_cast<const uint32_t *>(a - sh);
        const uint32_t w0 = q[0], w1 = q[1], w2 = q[2];
        return uint2{__builtin_amdgcn_alignbyte(w1, w0, sh), __builtin_amdgcn_alignbyte(w2, w1, sh)};
    }
    __device__ uint32_t v1(int r, int x) const { return p[r * pitch + x]; }
};

// How the workgroup's lanes map onto (row, block) of segments that hold up to `slots` blocks (crop_copy.hip)
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

// rows [0, nrows) of `len` bytes from `src` to d + r * dpitch
template <class P>
__device__ void put_rows(uint8_t *d, size_t dpitch, int len, int nrows, const P &src)
{
    const int slots = ((len + 15) >> 4) + 1;
    const LaneMap m(slots);
    if (m.ty < 0) return;
    for (int r = m.ty; r < nrows; r += m.ny) {
        uint8_t *dr = d + (size_t)r * dpitch;
        const int a = (int)((uintptr_t)dr & 15);
        for (int j = m.tx; j < slots; j += m.tx_n) {
            const int b0 = 16 * j - a;
            if (b0 >= len) break;
            if (b0 >= 0 && b0 + 16 <= len) {
                *reinterpret_cast<uint4 *>(dr + b0) = src.v16(r, b0);
            } else {   // head or tail of the segment: whole dwords where there are any, bytes for the rest
                for (int q = 0; q < 4; q++) {
                    const int s = b0 + 4 * q;
                    if (s >= 0 && s + 4 <= len) {
                        *reinterpret_cast<uint32_t *>(dr + s) =
                            src.v1(r, s) | (src.v1(r, s + 1) << 8) | (src.v1(r, s + 2) << 16) | (src.v1(r, s + 3) << 24);
                    } else {
                        const int e = min(s + 4, len);
                        for (int b = max(s, 0); b < e; b++) dr[b] = (uint8_t)src.v1(r, b);
                    }
                }
            }
        }
    }
}

// rows [0, nrows) of `w` samples -> RGB at d + r * dpitch; the first row is an even row and the first sample an even sample of
// the output picture, so chroma is row r >> 1, sample x >> 1 of cb / cr
template <class P>
__device__ void put_rgb(uint8_t *d, size_t dpitch, int w, int nrows, const P &y, const P &cb, const P &cr)
{
    const int slots = ((w + 15) >> 4) + 1;
    const LaneMap m(slots);
    if (m.ty < 0) return;
    for (int r = m.ty; r < nrows; r += m.ny) {
        uint8_t *dr = d + (size_t)r * dpitch;
        // the first sample whose RGB starts a 16-byte block: 3 ph = -dr (mod 16), 3 * 11 = 1 (mod 16); dr is even, so is ph
        const int ph = (int)((0u - (uint32_t)(uintptr_t)dr) * 11u & 15u);
        for (int j = m.tx; j < slots; j += m.tx_n) {
            const int x0 = ph - 16 + 16 * j;
            if (x0 >= w) break;
            if (x0 >= 0 && x0 + 16 <= w) {
                v4i o0, o1, o2;
                rgb16(y.v16(r, x0), cb.v8(r >> 1, x0 >> 1), cr.v8(r >> 1, x0 >> 1), o0, o1, o2);
                v4i *o = reinterpret_cast<v4i *>(dr + (size_t)x0 * 3);
                o[0] = o0; o[1] = o1; o[2] = o2;
            } else {   // head or tail: pairs of samples (one chroma sample each), six bytes at an even address
                const int e = min(x0 + 16, w);
                for (int x = max(x0, 0); x < e; x += 2) {
                    const uint32_t yw = y.v1(r, x) | (y.v1(r, x + 1) << 8);
                    const u16x2 cbv = {(unsigned short)cb.v1(r >> 1, x >> 1), (unsigned short)0};
                    const u16x2 crv = {(unsigned short)cr.v1(r >> 1, x >> 1), (unsigned short)0};
                    int d0, d1, d2;
                    rgb4(yw, cbv, crv, d0, d1, d2);
                    uint16_t *o = reinterpret_cast<uint16_t *>(dr + (size_t)x * 3);
                    o[0] = (uint16_t)d0; o[1] = (uint16_t)((uint32_t)d0 >> 16); o[2] = (uint16_t)d1;
                }
            }
        }
    }
}

struct Planes {   // where the rectangle of one source picture lies
    const uint8_t *y, *cb, *cr;
};
__device__ __forceinline__ Planes planes_of(const OrientArgs &a, int pic)
{
    const uint8_t *s = a.src + (size_t)pic * a.frame_bytes;
    return {s + a.y_off, s + a.cb_off, s + a.cr_off};
}

// ---- 0 and 2 turns: bands of whole rows, no LDS ----
template <class P>
__device__ void band_out(const OrientArgs &a, int pic, int r0, int nr, const P &y, const P &cb, const P &cr)
{
    const int w = a.w, h = a.h, cw = w >> 1, ch = h >> 1;
    if (a.yuv) {
        uint8_t *o = a.yuv + (size_t)pic * ((size_t)w * h * 3 / 2);
        put_rows(o + (size_t)2 * r0 * w, (size_t)w, w, 2 * nr, y);
        put_rows(o + (size_t)w * h + (size_t)r0 * cw, (size_t)cw, cw, nr, cb);
        put_rows(o + (size_t)w * h + (size_t)cw * ch + (size_t)r0 * cw, (size_t)cw, cw, nr, cr);
    }
    if (a.rgb) {
        uint8_t *o = a.rgb + (size_t)pic * ((size_t)w * h * 3);
        put_rgb(o + (size_t)2 * r0 * w * 3, (size_t)w * 3, w, 2 * nr, y, cb, cr);
    }
}

__global__ __launch_bounds__(256) void orient_rows_kernel(OrientArgs a)
{
    const int pic = blockIdx.y;
    const int cw = a.w >> 1, ch = a.h >> 1;
    const int r0 = blockIdx.x * a.band;   // first chroma row of the band, in the OUTPUT
    const int nr = min(a.band, ch - r0);
    if (nr <= 0) return;
    const Planes s = planes_of(a, pic);
    const int cp = a.pitch >> 1;
    if (a.turns == 0) {
        const FwdPlane y{s.y + (size_t)2 * r0 * a.pitch, a.src_end, a.pitch};
        const FwdPlane cb{s.cb + (size_t)r0 * cp, a.src_end, cp}, cr{s.cr + (size_t)r0 * cp, a.src_end, cp};
        band_out(a, pic, r0, nr, y, cb, cr);
    } else {   // output (R, x) = source (h - 1 - R, w - 1 - x)
        const RevPlane y{s.y + (size_t)(a.h - 1 - 2 * r0) * a.pitch + (a.w - 1), a.src_end, a.pitch};
        const RevPlane cb{s.cb + (size_t)(ch - 1 - r0) * cp + (cw - 1), a.src_end, cp};
        const RevPlane cr{s.cr + (size_t)(ch - 1 - r0) * cp + (cw - 1), a.src_end, cp};
        band_out(a, pic, r0, nr, y, cb, cr);
    }
}

// ---- 1 and 3 turns: tiles through LDS ----

// 4x4 bytes: rows a b c d (one dword each) -> columns t[0..3], t[j] = a_j | b_j << 8 | c_j << 16 | d_j << 24
__device__ __forceinline__ void transpose4(uint32_t a, uint32_t b, uint32_t c, uint32_t d, uint32_t t[4])
{
    const uint32_t ab_lo = __builtin_amdgcn_perm(b, a, 0x05010400u), ab_hi = __builtin_amdgcn_perm(b, a, 0x07030602u);
    const uint32_t cd_lo = __builtin_amdgcn_perm(d, c, 0x05010400u), cd_hi = __builtin_amdgcn_perm(d, c, 0x07030602u);
    t[0] = __builtin_amdgcn_perm(cd_lo, ab_lo, 0x05040100u);
    t[1] = __builtin_amdgcn_perm(cd_lo, ab_lo, 0x07060302u);
    t[2] = __builtin_amdgcn_perm(cd_hi, ab_hi, 0x05040100u);
    t[3] = __builtin_amdgcn_perm(cd_hi, ab_hi, 0x07060302u);
}

// The source rectangle s (sw x sh, sw <= tile, sh <= tile of the plane) turned into `lds`.  With SHp = sh rounded up to 4 and
// SWp = sw rounded up to 16, source (ly, lx) lands at
//     1 turn:  row lx,            byte SHp - 1 - ly     (the tile's output starts at byte SHp - sh of row 0)
//     3 turns: row SWp - 1 - lx,  byte ly               (the tile's output starts at byte 0 of row SWp - sw)
// so every store is an aligned dword inside the tile, whatever sw and sh; samples beyond the rectangle are zeros that nothing reads.
__device__ void stage(uint8_t *lds, int lpitch, const uint8_t *s, int pitch, int sw, int sh, int turns, const uint8_t *end)
{
    const int nbx = (sw + 15) >> 4, nry = (sh + 3) >> 2;
    const int units = 4 * nry * ((nbx + 3) >> 2);
    const int SHp = nry * 4, SWp = nbx * 16;
    for (int u = threadIdx.x; u < units; u += kThreads) {
        const int t = u >> 2, g = t / nry;
        const int ry = t - g * nry, bx = g * 4 + (u & 3);
        if (bx >= nbx) continue;
        const int x = 16 * bx, y = 4 * ry;
        uint4 r[4];
        for (int k = 0; k < 4; k++) {
            r[k] = uint4{0, 0, 0, 0};
            if (y + k >= sh) continue;
            const uint8_t *p = s + (size_t)(y + k) * pitch + x;
            if (x + 16 <= sw) {
                r[k] = load16(p, end);
            } else {
                uint32_t w[4] = {0, 0, 0, 0};
                for (int i = 0; i < sw - x; i++) w[i >> 2] |= (uint32_t)p[i] << (8 * (i & 3));
                r[k] = uint4{w[0], w[1], w[2], w[3]};
            }
        }
        const bool one = turns == 1;
        const uint4 a = one ? r[3] : r[0], b = one ? r[2] : r[1], c = one ? r[1] : r[2], d = one ? r[0] : r[3];
        uint8_t *o = one ? lds + x * lpitch + (SHp - 4 - y) : lds + (SWp - 1 - x) * lpitch + y;
        const int step = one ? lpitch : -lpitch;
        const uint32_t aw[4] = {a.x, a.y, a.z, a.w}, bw[4] = {b.x, b.y, b.z, b.w}, cw[4] = {c.x, c.y, c.z, c.w},
                       dw[4] = {d.x, d.y, d.z, d.w};
#pragma unroll
        for (int k = 0; k < 4; k++) {
            uint32_t tr[4];
            transpose4(aw[k], bw[k], cw[k], dw[k], tr);
#pragma unroll
            for (int j = 0; j < 4; j++) *reinterpret_cast<uint32_t *>(o + (4 * k + j) * step) = tr[j];
        }
    }
}

__global__ __launch_bounds__(256) void orient_tiles_kernel(OrientArgs a)
{
    __shared__ __attribute__((aligned(16))) uint8_t lds[kLdsBytes];
    uint8_t *ly = lds, *lcb = lds + kLdsY, *lcr = lds + kLdsY + kLdsC;
    const int pic = blockIdx.y;
    const int w = a.w, h = a.h;
    const int OW = h, OH = w;   // the output picture
    const int tiles_x = (OW + kTile - 1) / kTile;
    const int ty = (int)blockIdx.x / tiles_x, tx = (int)blockIdx.x - ty * tiles_x;
    const int ox0 = tx * kTile, oy0 = ty * kTile;
    const int otw = min(kTile, OW - ox0), oth = min(kTile, OH - oy0);
    // the source rectangle of the tile: sh = otw rows, sw = oth samples
    const int sx0 = a.turns == 1 ? oy0 : w - oy0 - oth;
    const int sy0 = a.turns == 1 ? h - ox0 - otw : ox0;
    const int sw = oth, sh = otw;
    const Planes s = planes_of(a, pic);
    const int cp = a.pitch >> 1;
    stage(ly, kPitchY, s.y + (size_t)sy0 * a.pitch + sx0, a.pitch, sw, sh, a.turns, a.src_end);
    stage(lcb, kPitchC, s.cb + (size_t)(sy0 >> 1) * cp + (sx0 >> 1), cp, sw >> 1, sh >> 1, a.turns, a.src_end);
    stage(lcr, kPitchC, s.cr + (size_t)(sy0 >> 1) * cp + (sx0 >> 1), cp, sw >> 1, sh >> 1, a.turns, a.src_end);
    __syncthreads();
    // where the tile's output (0, 0) lies in each staged plane
    const int csw = sw >> 1, csh = sh >> 1;
    const int yo = a.turns == 1 ? ((sh + 3) & ~3) - sh : (((sw + 15) & ~15) - sw) * kPitchY;
    const int co = a.turns == 1 ? ((csh + 3) & ~3) - csh : (((csw + 15) & ~15) - csw) * kPitchC;
    const LdsPlane py{ly + yo, kPitchY}, pcb{lcb + co, kPitchC}, pcr{lcr + co, kPitchC};
    const int cOW = OW >> 1, cOH = OH >> 1;
    if (a.yuv) {
        uint8_t *o = a.yuv + (size_t)pic * ((size_t)w * h * 3 / 2);
        put_rows(o + (size_t)oy0 * OW + ox0, (size_t)OW, otw, oth, py);
        uint8_t *oc = o + (size_t)OW * OH + (size_t)(oy0 >> 1) * cOW + (ox0 >> 1);
        put_rows(oc, (size_t)cOW, otw >> 1, oth >> 1, pcb);
        put_rows(oc + (size_t)cOW * cOH, (size_t)cOW, otw >> 1, oth >> 1, pcr);
    }
    if (a.rgb) {
        uint8_t *o = a.rgb + (size_t)pic * ((size_t)w * h * 3);
        put_rgb(o + ((size_t)oy0 * OW + ox0) * 3, (size_t)OW * 3, otw, oth, py, pcb, pcr);
    }
}

} // namespace

hipError_t launch_orient(const OrientArgs &a, hipStream_t stream)
{
    const bool tiles = (a.turns & 1) != 0;
    const unsigned gx = tiles ? (unsigned)(((a.h + kTile - 1) / kTile) * ((a.w + kTile - 1) / kTile))
                              : (unsigned)((a.h / 2 + a.band - 1) / a.band);
    for (int first = 0; first < a.n; first += 65535) {   // (grid y is at most 65535)
        OrientArgs b = a;
        b.n = min(65535, a.n - first);
        b.src = a.src + (size_t)first * a.frame_bytes;
        b.yuv = a.yuv ? a.yuv + (size_t)first * ((size_t)a.w * a.h * 3 / 2) : nullptr;
        b.rgb = a.rgb ? a.rgb + (size_t)first * ((size_t)a.w * a.h * 3) : nullptr;
        if (tiles) hipLaunchKernelGGL(orient_tiles_kernel, dim3(gx, (unsigned)b.n), dim3(kThreads), 0, stream, b);
        else hipLaunchKernelGGL(orient_rows_kernel, dim3(gx, (unsigned)b.n), dim3(kThreads), 0, stream, b);
        const hipError_t e = hipGetLastError();
        if (e != hipSuccess) return e;
    }
    return hipSuccess;
}

} // namespace mvhp
