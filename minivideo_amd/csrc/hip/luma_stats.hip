// luma_stats.hip -- picture scores (opt-in; DESIGN.md 3 "Picture scores"): the sum and the sum of squares of the luma samples of
// one rectangle of every coded picture of a batch, gfx950.  Read-only on the planes, 32 bytes out per picture.
//
// Mapping: one workgroup of 256 threads per (picture, band of `band` luma rows); pictures in grid.x (a batch may pass 65535).
// A source row is 16-byte aligned (the pitch is 16 W, a picture 384 W H bytes), so the rectangle's part of a row is cut at the
// 16-byte boundaries of the SOURCE: blocks cx / 16 .. (cx + cw - 1) / 16 of the row, every one a whole aligned dwordx4 inside
// the row.  The band's (row, block) pairs are numbered row-major and lane t takes pairs t, t + 256, ...: consecutive lanes
// load consecutive blocks, four loads of a lane are in flight before the first is summed.  The bytes of a row's first and last
// block that lie outside the rectangle are zeroed in registers (two shifts per dword), so they add nothing to either sum.
// Sums: v_sad_u8 against 0 and v_dot4_u32_u8 of a dword with itself, four samples per instruction.  Lanes are reduced across
// the wave, the four waves through 64 bytes of LDS, and one lane adds the band's two 64-bit sums to the picture's record with
// device-scope atomics.  Integer sums: the record does not depend on the band size or on the order the bands arrive in.
// Stateless: the launch function zeroes the records on the same stream first; no waits, no inline assembly -- safe under
// stream capture.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "recon_kernels.h"

namespace mvhp {

namespace {

constexpr int kThreads = 256;
constexpr int kInFlight = 4;   // blocks a lane loads before it sums the first

// the dword holding bytes [4 k, 4 k + 4) of a block, with the bytes outside [lo, hi) of the block zeroed (0 <= lo < hi <= 16)
__device__ __forceinline__ uint32_t keep(uint32_t w, int k, int lo, int hi)
{
    const int s = min(max(lo - 4 * k, 0), 4), e = min(max(hi - 4 * k, 0), 4);
    const uint32_t m_lo = s >= 4 ? 0u : 0xffffffffu << (8 * s);
    const uint32_t m_hi = e <= 0 ? 0u : 0xffffffffu >> (8 * (4 - e));
    return w & m_lo & m_hi;
}

__device__ __forceinline__ uint64_t wave_sum(uint64_t v)
{
    for (int d = 32; d > 0; d >>= 1) v += __shfl_xor((unsigned long long)v, d, 64);
    return v;
}

__global__ __launch_bounds__(256) void luma_stats_kernel(LumaStatsArgs a)
{
    const int pic = blockIdx.x;
    const int r0 = blockIdx.y * a.band;
    const int nr = min(a.band, a.ch - r0);
    if (nr <= 0) return;
    const int b_lo = a.cx >> 4;
    const int nblk = ((a.cx + a.cw - 1) >> 4) - b_lo + 1;      // blocks of a row that hold samples of the rectangle
    const int x_end = a.cx + a.cw;
    const uint8_t *base = a.src + (size_t)pic * a.frame_bytes + (size_t)(a.cy + r0) * a.pitch + (size_t)b_lo * 16;
    const int items = nr * nblk;
    // pair i = (row i / nblk, block i % nblk); a lane's next pair is 256 further: one division per lane, none per block
    const int dq = kThreads / nblk, dm = kThreads - dq * nblk;
    int row = (int)threadIdx.x / nblk, blk = (int)threadIdx.x - row * nblk;

    uint64_t S = 0, Q = 0;
    for (int i = threadIdx.x; i < items; i += kInFlight * kThreads) {
        uint4 v[kInFlight];
        int lo[kInFlight], hi[kInFlight];
        // Four unconditional loads, back to back: a pair past the band's last one (the last round only) loads pair (0, 0)
        // instead -- items >= 1, so that block exists -- and keeps none of its bytes (lo = hi = 0).  No load sits under a branch.
#pragma unroll
        for (int u = 0; u < kInFlight; u++) {
            const bool live = i + u * kThreads < items;
            const int r = live ? row : 0, c = live ? blk : 0;
            v[u] = *reinterpret_cast<const uint4 *>(base + (size_t)r * a.pitch + (size_t)c * 16);
            const int x0 = (b_lo + c) * 16;                    // the block's first sample, in the coded row
            lo[u] = live ? max(a.cx - x0, 0) : 0;
            hi[u] = live ? min(x_end - x0, 16) : 0;
            row += dq; blk += dm;
            if (blk >= nblk) { blk -= nblk; row++; }
        }
        // 32-bit sums of one round: at most 4 blocks x 16 samples x 255^2 = 4 161 600 (and x 255 = 16 320), far below 2^32;
        // they are widened to 64 bits after every round, so no count of rows or blocks can overflow them.
        uint32_t s = 0, q = 0;
#pragma unroll
        for (int u = 0; u < kInFlight; u++) {
            uint32_t w[4] = {v[u].x, v[u].y, v[u].z, v[u].w};
            if (lo[u] != 0 || hi[u] != 16) {                   // head or tail block of a row
#pragma unroll
                for (int k = 0; k < 4; k++) w[k] = keep(w[k], k, lo[u], hi[u]);
            }
#pragma unroll
            for (int k = 0; k < 4; k++) {
                s = __builtin_amdgcn_sad_u8(w[k], 0u, s);
                q = __builtin_amdgcn_udot4(w[k], w[k], q, false);
            }
        }
        S += s;
        Q += q;
    }

    __shared__ uint64_t part[2][kThreads / 64];
    S = wave_sum(S);
    Q = wave_sum(Q);
    const int wave = threadIdx.x >> 6;
    if ((threadIdx.x & 63) == 0) { part[0][wave] = S; part[1][wave] = Q; }
    __syncthreads();
    if (threadIdx.x == 0) {
        uint64_t ts = 0, tq = 0;
        for (int k = 0; k < kThreads / 64; k++) { ts += part[0][k]; tq += part[1][k]; }
        mvhp_luma_stats_t *rec = a.stats + pic;
        __hip_atomic_fetch_add((unsigned long long *)&rec->sum, (unsigned long long)ts, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        __hip_atomic_fetch_add((unsigned long long *)&rec->sumsq, (unsigned long long)tq, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        if (blockIdx.y == 0) rec->samples = (uint32_t)a.cw * (uint32_t)a.ch;   // (the other words stay as the memset left them)
    }
}

} // namespace

hipError_t launch_luma_stats(const LumaStatsArgs &a, hipStream_t stream)
{
    if (a.n == 0) return hipSuccess;
    hipError_t e = hipMemsetAsync(a.stats, 0, (size_t)a.n * sizeof(mvhp_luma_stats_t), stream);
    if (e != hipSuccess) return e;
    LumaStatsArgs b = a;
    while ((b.ch + b.band - 1) / b.band > 65535) b.band *= 2;   // (grid y is at most 65535)
    const int bands = (b.ch + b.band - 1) / b.band;
    const int per_launch = (1 << 23) / bands > 0 ? (1 << 23) / bands : 1;   // (a grid holds fewer than 2^32 threads)
    for (int first = 0; first < a.n; first += per_launch) {
        b.n = a.n - first < per_launch ? a.n - first : per_launch;
        b.src = a.src + (size_t)first * a.frame_bytes;
        b.stats = a.stats + first;
        hipLaunchKernelGGL(luma_stats_kernel, dim3((unsigned)b.n, (unsigned)bands), dim3(kThreads), 0, stream, b);
        e = hipGetLastError();
        if (e != hipSuccess) return e;
    }
    return hipSuccess;
}

} // namespace mvhp
