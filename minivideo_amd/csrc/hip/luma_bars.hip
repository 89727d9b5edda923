// luma_bars.hip -- black bars (opt-in; DESIGN.md 3 "Black bars"): the box of the content rows and columns of one rectangle of
// every coded picture of a batch, gfx950.  Read-only on the planes, 32 bytes out per picture.  A sample is bright when
// Y > level; a row is content when at least max(1, cw >> 5) of its samples are bright, a column when at least max(1, ch >> 5).
//
// Two kernels.  The counting pass: one workgroup of 256 threads per (picture, band of `band` luma rows), pictures in grid.x.  A
// source row is 16-byte aligned, so the rectangle's part of a row is cut at the 16-byte boundaries of the SOURCE (blocks
// cx / 16 .. (cx + cw - 1) / 16, each a whole aligned dwordx4); the bytes of a row's first and last block outside the rectangle
// are zeroed in registers (level >= 1: a zero is never bright).  A row takes L lanes, L = the blocks of a row rounded up to
// whole waves (at most 256; wider rows are walked in chunks of 256 blocks), so 256 / L rows are in flight per step and a lane
// STAYS ON ITS COLUMN BLOCK down the band: the bright flags of four samples sit in the four bytes of a dword (two 16-bit adds
// whose carries are the comparisons), and adding the flag dwords row after row gives four column counters per add -- for up to
// 255 rows, then the lane empties them into LDS.  v_sad_u8 of a flag dword against 0 is the row's share of that lane; shares of
// two rows ride one dword through the wave reduction, and one lane adds the wave's share to the row's counter in LDS.
// A band is walked in tiles of 1024 rows.  Behind a tile the row counters go out as PLAIN stores (a workgroup owns its rows)
// and the column counters are added to the picture's 32-bit counters with device-scope atomics, consecutive lanes on
// consecutive counters, zeros skipped.  Integer sums: the counters do not depend on the band size or the order of arrival.
// The bounds pass: one workgroup per picture finds first, last and number of the content rows and columns and writes the record.
// Stateless: the launch function zeroes the column counters on the same stream first; no waits, no inline assembly -- safe
// under stream capture.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "recon_kernels.h"

namespace mvhp {

namespace {

constexpr int kThreads = 256;
constexpr int kInFlight = 4;    // rows a lane loads before it counts the first
constexpr int kTile = 1024;     // rows whose counters a workgroup keeps in LDS
constexpr int kColPitch = kThreads + 1;   // of the column counters in LDS: [sample of the block][lane], odd against bank conflicts

// the dword holding bytes [4 k, 4 k + 4) of a block, with the bytes outside [lo, hi) of the block zeroed (0 <= lo <= hi <= 16)
__device__ __forceinline__ uint32_t keep(uint32_t w, int k, int lo, int hi)
{
    const int s = min(max(lo - 4 * k, 0), 4), e = min(max(hi - 4 * k, 0), 4);
    const uint32_t m_lo = s >= 4 ? 0u : 0xffffffffu << (8 * s);
    const uint32_t m_hi = e <= 0 ? 0u : 0xffffffffu >> (8 * (4 - e));
    return w & m_lo & m_hi;
}

// 0x01 in every byte of w that is above the level; K = (255 - level) * 0x00010001: x + 255 - level carries into bit 8 exactly
// when x > level, and two bytes per dword leave room for the carry
__device__ __forceinline__ uint32_t bright(uint32_t w, uint32_t K)
{
    const uint32_t even = ((w & 0x00ff00ffu) + K) >> 8 & 0x00010001u;
    const uint32_t odd = (((w >> 8) & 0x00ff00ffu) + K) & 0x01000100u;
    return even | odd;
}

__device__ __forceinline__ uint32_t wave_sum(uint32_t v)
{
    for (int d = 32; d > 0; d >>= 1) v += __shfl_xor(v, d, 64);
    return v;
}

// a lane's four packed column counters into the chunk's counters in LDS (lane cl of the chunk)
__device__ __forceinline__ void empty_into(uint32_t *s_col, int cl, uint32_t acc[4])
{
#pragma unroll
    for (int k = 0; k < 4; k++) {
#pragma unroll
        for (int b = 0; b < 4; b++) {
            const uint32_t v = (acc[k] >> (8 * b)) & 0xffu;
            if (v) atomicAdd(&s_col[(4 * k + b) * kColPitch + cl], v);
        }
        acc[k] = 0;
    }
}

__global__ __launch_bounds__(256) void luma_bars_count_kernel(LumaBarsArgs a)
{
    __shared__ uint32_t s_col[16 * kColPitch];
    __shared__ uint32_t s_row[kTile];
    const int pic = blockIdx.x;
    const int r0 = blockIdx.y * a.band;
    const int nr = min(a.band, a.ch - r0);
    if (nr <= 0) return;
    const int b_lo = a.cx >> 4;
    const int nblk = ((a.cx + a.cw - 1) >> 4) - b_lo + 1;      // blocks of a row that hold samples of the rectangle
    const int x_end = a.cx + a.cw;
    const int L = min(((nblk + 63) >> 6) << 6, kThreads);       // lanes of a row: whole waves, so a wave works on one row
    const int G = kThreads / L;                                 // rows in flight per step (L = 192 leaves one wave idle)
    const int t = threadIdx.x;
    const int rsub = t / L, cl = t - rsub * L;
    const uint32_t K = (255u - (uint32_t)a.level) * 0x00010001u;
    const uint8_t *band0 = a.src + (size_t)pic * a.frame_bytes + (size_t)(a.cy + r0) * a.pitch + (size_t)b_lo * 16;
    uint32_t *cols = a.cols + (size_t)pic * a.cw;
    uint32_t *rows = a.rows + (size_t)pic * a.ch + r0;

    for (int tb = 0; tb < nr; tb += kTile) {
        const int tr = min(kTile, nr - tb);
        for (int c0 = 0; c0 < nblk; c0 += L) {
            for (int i = t; i < 16 * kColPitch; i += kThreads) s_col[i] = 0;
            if (c0 == 0)
                for (int i = t; i < tr; i += kThreads) s_row[i] = 0;
            __syncthreads();
            if (rsub < G) {   // (uniform in a wave)
                const int c = c0 + cl;
                const bool on = c < nblk;                      // a lane past the row's last block loads block c0 and keeps nothing
                const int x0 = (b_lo + c) * 16;                // the block's first sample, in the coded row
                const int lo = on ? max(a.cx - x0, 0) : 0, hi = on ? min(x_end - x0, 16) : 0;
                const uint8_t *col0 = band0 + (size_t)tb * a.pitch + (size_t)(on ? c : c0) * 16;
                uint32_t acc[4] = {0, 0, 0, 0};
                int held = 0;                                  // rows added to acc since it was emptied (uniform in a wave)
                for (int r = rsub; r < tr; r += kInFlight * G) {
                    if (held > 255 - kInFlight) { empty_into(s_col, cl, acc); held = 0; }
                    uint4 v[kInFlight];
                    // Four unconditional loads, back to back: a row past the tile's last one loads row r instead and counts nothing
#pragma unroll
                    for (int u = 0; u < kInFlight; u++) {
                        const int rr = r + u * G;
                        v[u] = *reinterpret_cast<const uint4 *>(col0 + (size_t)(rr < tr ? rr : r) * a.pitch);
                    }
                    uint32_t share[kInFlight];
#pragma unroll
                    for (int u = 0; u < kInFlight; u++) {
                        uint32_t w[4] = {v[u].x, v[u].y, v[u].z, v[u].w};
                        const bool live = r + u * G < tr;
                        const int l = live ? lo : 0, h = live ? hi : 0;
                        if (l != 0 || h != 16) {               // head or tail block of a row, or nothing at all
#pragma unroll
                            for (int k = 0; k < 4; k++) w[k] = keep(w[k], k, l, h);
                        }
                        uint32_t s = 0;
#pragma unroll
                        for (int k = 0; k < 4; k++) {
                            const uint32_t f = bright(w[k], K);
                            acc[k] += f;
                            s = __builtin_amdgcn_sad_u8(f, 0u, s);
                        }
                        share[u] = s;                          // at most 16
                    }
                    held += kInFlight;
                    // a wave's share of a row is at most 1024: two rows per dword
                    const uint32_t p01 = wave_sum(share[0] | share[1] << 16), p23 = wave_sum(share[2] | share[3] << 16);
                    if ((t & 63) == 0) {
                        const uint32_t sum[kInFlight] = {p01 & 0xffffu, p01 >> 16, p23 & 0xffffu, p23 >> 16};
#pragma unroll
                        for (int u = 0; u < kInFlight; u++)
                            if (r + u * G < tr && sum[u]) atomicAdd(&s_row[r + u * G], sum[u]);
                    }
                }
                empty_into(s_col, cl, acc);
            }
            __syncthreads();
            // the chunk's columns, in the order of the row: consecutive lanes add to consecutive counters
            for (int i = t; i < 16 * L; i += kThreads) {
                const int x = (b_lo + c0 + (i >> 4)) * 16 + (i & 15);
                if (x >= a.cx && x < x_end) {
                    const uint32_t v = s_col[(i & 15) * kColPitch + (i >> 4)];
                    if (v) __hip_atomic_fetch_add(&cols[x - a.cx], v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
                }
            }
            if (c0 + L >= nblk)   // the row's last chunk: the tile's row counters are whole
                for (int i = t; i < tr; i += kThreads) rows[tb + i] = s_row[i];
            __syncthreads();
        }
    }
}

__global__ __launch_bounds__(256) void luma_bars_bounds_kernel(LumaBarsArgs a)
{
    __shared__ uint32_t s[6];   // rows: first, last + 1, count; columns: the same
    const int pic = blockIdx.x, t = threadIdx.x;
    if (t < 6) s[t] = (t == 0 || t == 3) ? 0xffffffffu : 0u;
    __syncthreads();
    const uint32_t need_row = max(1u, (uint32_t)a.cw >> 5), need_col = max(1u, (uint32_t)a.ch >> 5);
    for (int axis = 0; axis < 2; axis++) {
        const uint32_t *cnt = axis ? a.cols + (size_t)pic * a.cw : a.rows + (size_t)pic * a.ch;
        const int len = axis ? a.cw : a.ch;
        const uint32_t need = axis ? need_col : need_row;
        uint32_t first = 0xffffffffu, end = 0, count = 0;
        for (int i = t; i < len; i += kThreads)
            if (cnt[i] >= need) { first = min(first, (uint32_t)i); end = (uint32_t)i + 1; count++; }
        if (count) {
            atomicMin(&s[3 * axis], first);
            atomicMax(&s[3 * axis + 1], end);
            atomicAdd(&s[3 * axis + 2], count);
        }
    }
    __syncthreads();
    if (t == 0) {
        mvhp_luma_bars_t rec;
        const bool any = s[2] != 0 && s[5] != 0;
        rec.x = any ? (uint32_t)a.cx + s[3] : 0u;
        rec.y = any ? (uint32_t)a.cy + s[0] : 0u;
        rec.w = any ? s[4] - s[3] : 0u;
        rec.h = any ? s[1] - s[0] : 0u;
        rec.rows = s[2];
        rec.cols = s[5];
        rec.reserved[0] = rec.reserved[1] = 0;
        a.bars[pic] = rec;
    }
}

} // namespace

size_t luma_bars_scratch_bytes(const LumaBarsArgs &a) { return (size_t)a.n * ((size_t)a.cw + (size_t)a.ch) * sizeof(uint32_t); }

hipError_t launch_luma_bars(const LumaBarsArgs &a, hipStream_t stream)
{
    if (a.n == 0) return hipSuccess;
    LumaBarsArgs b = a;
    b.cols = a.scratch;                               // n x cw, added to: zeroed here
    b.rows = a.scratch + (size_t)a.n * a.cw;          // n x ch, every one stored by the workgroup that owns the row
    hipError_t e = hipMemsetAsync(b.cols, 0, (size_t)a.n * a.cw * sizeof(uint32_t), stream);
    if (e != hipSuccess) return e;
    while ((b.ch + b.band - 1) / b.band > 65535) b.band *= 2;   // (grid y is at most 65535)
    const int bands = (b.ch + b.band - 1) / b.band;
    int per_launch = (1 << 23) / bands > 0 ? (1 << 23) / bands : 1;   // (a grid holds fewer than 2^32 threads)
    if (per_launch > 65535) per_launch = 65535;
    for (int first = 0; first < a.n; first += per_launch) {
        LumaBarsArgs c = b;
        c.n = a.n - first < per_launch ? a.n - first : per_launch;
        c.src = b.src + (size_t)first * b.frame_bytes;
        c.cols = b.cols + (size_t)first * b.cw;
        c.rows = b.rows + (size_t)first * b.ch;
        c.bars = b.bars + first;
        hipLaunchKernelGGL(luma_bars_count_kernel, dim3((unsigned)c.n, (unsigned)bands), dim3(kThreads), 0, stream, c);
        e = hipGetLastError();
        if (e != hipSuccess) return e;
        hipLaunchKernelGGL(luma_bars_bounds_kernel, dim3((unsigned)c.n), dim3(kThreads), 0, stream, c);
        e = hipGetLastError();
        if (e != hipSuccess) return e;
    }
    return hipSuccess;
}

} // namespace mvhp
