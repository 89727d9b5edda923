// plane_hist.hip -- representative pictures (opt-in; DESIGN.md 3 "Representative pictures"): the histograms of the luma and the
// two chroma samples of one rectangle of every coded picture of a batch, gfx950.  Read-only on the planes, 3104 bytes out per
// picture.
//
// Mapping: one workgroup of 256 threads per (picture, band of `band` luma rows); pictures in grid.x (a batch may pass 65535).
// A band owns the chroma rows whose upper luma row lies in it, so bands of any size, odd ones too, split the chroma rows exactly.
// Luma rows are 16-byte aligned (pitch 16 W), chroma rows 8-byte aligned (pitch 8 W): the rectangle's part of a row is cut at the
// 16-byte (chroma: 8-byte) boundaries of the SOURCE, every block one aligned dwordx4 (dwordx2) inside the row, as in
// luma_stats.hip.  The band's (row, block) pairs are numbered row-major -- for chroma the rows of Cb, then those of Cr -- lane t
// takes pairs t, t + 256, ...; four loads of a lane are in flight before the first is counted, none under a branch.
// Counting: the workgroup keeps kRep = 16 copies of each of the three histograms in LDS (48 KiB: three workgroups a CU), copy
// lane & 15, word (value * 16 + copy): the 16 copies of one value lie in 16 consecutive banks, so a flat picture -- every lane
// the same value -- spreads a half-wave's 32 adds over 16 addresses in 16 banks (2 adds an address) instead of 32 on one, and on
// any content two lanes of a half-wave meet in a bank only as the pair (l, l + 16).  One ds_add_u32 per sample, no return value.
// The bytes of a row's first and last block that lie outside the rectangle are NOT counted (a zeroed byte would land in bin 0):
// such a block counts its bytes one by one under a predicate; whole blocks take the unpredicated path.
// At the end thread t sums the copies of bin t of each plane and adds what is not zero to the picture's record with a 32-bit
// device-scope atomic: consecutive lanes, consecutive words.  Integer counts: the record does not depend on the band size or on
// the order the bands arrive in.  Stateless: the launch function zeroes the records on the same stream first; no waits, no
// inline assembly -- safe under stream capture.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "recon_kernels.h"

namespace mvhp {

namespace {

constexpr int kThreads = 256;
constexpr int kInFlight = 4;            // blocks a lane loads before it counts the first
constexpr int kRep = 16;                // copies of a histogram in LDS
constexpr int kPlaneWords = 256 * kRep;

// h: the lane's copy of one plane's histogram (word `copy` of it)
__device__ __forceinline__ void bump(uint32_t *h, uint32_t v)
{
    __hip_atomic_fetch_add(h + v * kRep, 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
}

// the four samples of dword w, which holds bytes [j0, j0 + 4) of a block of which bytes [lo, hi) count
__device__ __forceinline__ void count_dword(uint32_t *h, uint32_t w, int j0, int lo, int hi, bool whole)
{
    if (whole) {
        bump(h, w & 255u);
        bump(h, (w >> 8) & 255u);
        bump(h, (w >> 16) & 255u);
        bump(h, w >> 24);
    } else {
#pragma unroll
        for (int b = 0; b < 4; b++)
            if (j0 + b >= lo && j0 + b < hi) bump(h, (w >> (8 * b)) & 255u);
    }
}

__global__ __launch_bounds__(256) void plane_hist_kernel(PlaneHistArgs a)
{
    __shared__ __attribute__((aligned(16))) uint32_t lds[3 * kPlaneWords];
    const int pic = blockIdx.x;
    const int r0 = blockIdx.y * a.band;
    const int nr = min(a.band, a.ch - r0);
    if (nr <= 0) return;
    const int t = threadIdx.x;
    {
        uint4 *z = reinterpret_cast<uint4 *>(lds);
#pragma unroll
        for (int i = 0; i < 3 * kPlaneWords / 4 / kThreads; i++) z[i * kThreads + t] = make_uint4(0u, 0u, 0u, 0u);
    }
    __syncthreads();
    uint32_t *mine = lds + (t & (kRep - 1));
    const uint8_t *frame = a.src + (size_t)pic * a.frame_bytes;

    {   // ---- luma: rows r0 .. r0 + nr of the rectangle, 16-byte blocks
        const int b_lo = a.cx >> 4;
        const int nblk = ((a.cx + a.cw - 1) >> 4) - b_lo + 1;
        const int x_end = a.cx + a.cw;
        const uint8_t *base = frame + (size_t)(a.cy + r0) * a.pitch + (size_t)b_lo * 16;
        const int items = nr * nblk;
        // pair i = (row i / nblk, block i % nblk); a lane's next pair is 256 further: one division per lane, none per block
        const int dq = kThreads / nblk, dm = kThreads - dq * nblk;
        int row = t / nblk, blk = t - row * nblk;
        for (int i = t; i < items; i += kInFlight * kThreads) {
            uint4 v[kInFlight];
            int lo[kInFlight], hi[kInFlight];
            // a pair past the band's last one (the last round only) loads pair (0, 0) instead -- items >= 1, so that block
            // exists -- and counts none of its bytes (lo = hi = 0)
#pragma unroll
            for (int u = 0; u < kInFlight; u++) {
                const bool live = i + u * kThreads < items;
                const int r = live ? row : 0, c = live ? blk : 0;
                v[u] = *reinterpret_cast<const uint4 *>(base + (size_t)r * a.pitch + (size_t)c * 16);
                const int x0 = (b_lo + c) * 16;
                lo[u] = live ? max(a.cx - x0, 0) : 0;
                hi[u] = live ? min(x_end - x0, 16) : 0;
                row += dq; blk += dm;
                if (blk >= nblk) { blk -= nblk; row++; }
            }
#pragma unroll
            for (int u = 0; u < kInFlight; u++) {
                const bool whole = lo[u] == 0 && hi[u] == 16;
                count_dword(mine, v[u].x, 0, lo[u], hi[u], whole);
                count_dword(mine, v[u].y, 4, lo[u], hi[u], whole);
                count_dword(mine, v[u].z, 8, lo[u], hi[u], whole);
                count_dword(mine, v[u].w, 12, lo[u], hi[u], whole);
            }
        }
    }

    {   // ---- chroma: the rows j of the halved rectangle with r0 <= 2 j < r0 + nr, of Cb and then of Cr, 8-byte blocks
        const int j0 = (r0 + 1) >> 1, j1 = (r0 + nr + 1) >> 1;   // (r0 + nr <= ch, ch even: j1 <= ch / 2)
        const int ncr = j1 - j0;
        const int ccx = a.cx >> 1, ccw = a.cw >> 1, cpitch = a.pitch >> 1;
        const int b_lo = ccx >> 3;
        const int nblk = ((ccx + ccw - 1) >> 3) - b_lo + 1;
        const int x_end = ccx + ccw;
        const size_t luma_bytes = (size_t)a.pitch * a.rows;
        const uint8_t *base = frame + luma_bytes + (size_t)((a.cy >> 1) + j0) * cpitch + (size_t)b_lo * 8;
        const int items = 2 * ncr * nblk;                        // 0 for a band that owns no chroma row
        const int dq = kThreads / nblk, dm = kThreads - dq * nblk;
        int row = t / nblk, blk = t - row * nblk;                // row: 0 .. ncr of Cb, ncr .. 2 ncr of Cr
        for (int i = t; i < items; i += kInFlight * kThreads) {
            uint2 v[kInFlight];
            int lo[kInFlight], hi[kInFlight], pl[kInFlight];
#pragma unroll
            for (int u = 0; u < kInFlight; u++) {
                const bool live = i + u * kThreads < items;
                const int rr = live ? row : 0, c = live ? blk : 0;
                const int plane = rr >= ncr ? 1 : 0, r = rr - plane * ncr;
                v[u] = *reinterpret_cast<const uint2 *>(base + (size_t)plane * (luma_bytes >> 2) + (size_t)r * cpitch + (size_t)c * 8);
                const int x0 = (b_lo + c) * 8;
                lo[u] = live ? max(ccx - x0, 0) : 0;
                hi[u] = live ? min(x_end - x0, 8) : 0;
                pl[u] = plane;
                row += dq; blk += dm;
                if (blk >= nblk) { blk -= nblk; row++; }
            }
#pragma unroll
            for (int u = 0; u < kInFlight; u++) {
                uint32_t *h = mine + (1 + pl[u]) * kPlaneWords;
                const bool whole = lo[u] == 0 && hi[u] == 8;
                count_dword(h, v[u].x, 0, lo[u], hi[u], whole);
                count_dword(h, v[u].y, 4, lo[u], hi[u], whole);
            }
        }
    }

    __syncthreads();
    uint32_t *rec = reinterpret_cast<uint32_t *>(a.hist + pic);   // y[256], cb[256], cr[256]: words 0 .. 767
#pragma unroll
    for (int p = 0; p < 3; p++) {
        const uint4 *q = reinterpret_cast<const uint4 *>(lds + p * kPlaneWords + t * kRep);
        uint32_t s = 0;
#pragma unroll
        for (int k = 0; k < kRep / 4; k++) { const uint4 w = q[k]; s += w.x + w.y + w.z + w.w; }
        if (s) __hip_atomic_fetch_add(rec + p * 256 + t, s, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    }
    if (blockIdx.y == 0 && t == 0) {                              // (the other words stay as the memset left them)
        a.hist[pic].samples = (uint32_t)a.cw * (uint32_t)a.ch;
        a.hist[pic].chroma_samples = (uint32_t)(a.cw >> 1) * (uint32_t)(a.ch >> 1);
    }
}

} // namespace

hipError_t launch_plane_hist(const PlaneHistArgs &a, hipStream_t stream)
{
    if (a.n == 0) return hipSuccess;
    hipError_t e = hipMemsetAsync(a.hist, 0, (size_t)a.n * sizeof(mvhp_plane_hist_t), stream);
    if (e != hipSuccess) return e;
    PlaneHistArgs b = a;
    while ((b.ch + b.band - 1) / b.band > 65535) b.band *= 2;   // (grid y is at most 65535)
    const int bands = (b.ch + b.band - 1) / b.band;
    const int per_launch = (1 << 23) / bands > 0 ? (1 << 23) / bands : 1;   // (a grid holds fewer than 2^32 threads)
    for (int first = 0; first < a.n; first += per_launch) {
        b.n = a.n - first < per_launch ? a.n - first : per_launch;
        b.src = a.src + (size_t)first * a.frame_bytes;
        b.hist = a.hist + first;
        hipLaunchKernelGGL(plane_hist_kernel, dim3((unsigned)b.n, (unsigned)bands), dim3(kThreads), 0, stream, b);
        e = hipGetLastError();
        if (e != hipSuccess) return e;
    }
    return hipSuccess;
}

} // namespace mvhp
