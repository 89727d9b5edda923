// deblock.hip -- the H.264 in-loop deblocking filter (clause 8.7) as a post-pass over reconstructed pictures, gfx950.
// Opt-in (MVHP_STREAM_DEBLOCK / MVHP_PARAM_DEBLOCK / MINIVIDEO_DEBLOCK=1); the reference never deblocks, so nothing here is
// pinned to it.  Scope: what the front end produces -- frame macroblocks, 4:2:0, 8-bit, intra only (bS 4 on macroblock edges,
// 3 inside).  Intra prediction has already used the unfiltered samples, so filtering the finished planes in macroblock raster
// order is exactly the standard's process.
//
// Mapping: one workgroup per picture, NW wavefronts; wave w filters macroblock rows w, w + NW, ...  MB(x, y) may start once
// row y - 1 has finished MB(x + 1, y - 1) (its left-edge filter is the last to touch MB(x, y - 1)): a per-wave progress
// counter in LDS, as recon_rows_kernel.  Nothing is shared between workgroups.
//
// Every output byte is written once, by the wave that finalises it, and no wave reads from global memory a byte another wave
// writes:
//   * step x of row y reads MB(x, y) from the planes (unfiltered: nobody has written it yet) and keeps, in its LDS tile, the
//     4 luma / 2 chroma columns left of it from step x - 1;
//   * the rows above the top edge (luma 12..15, chroma 6..7 of row y - 1, as row y - 1 left them) come from ONE LDS line
//     buffer per picture; the top-edge filter changes luma rows 13..15 / chroma row 7 of row y - 1, and row y writes them;
//   * after step x the columns [16x - 4, 16x + 12) (chroma [8x - 2, 8x + 6)) of row y are final except for the rows the next
//     row's top edge may change: rows 0..12 (chroma 0..6) go to the planes, rows 12..15 (chroma 6..7) to the line buffer.
//     The last column also flushes its right four (two) columns; the last row also writes its own bottom rows.
// Lanes: 0..15 hold the 16 luma lines of an edge, 16..23 the Cb lines, 24..31 the Cr lines -- rows for the vertical edges,
// columns (through the LDS tile) for the horizontal ones.  The per-edge arithmetic is deblock_edge.h.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "minivideo_hotpath.h"
#include "recon_kernels.h"
#include "recon_device.h"
#include "deblock_edge.h"

namespace mvhp {

namespace {

constexpr int TYS = 20;   // luma tile: 20 x 20, rows 0..3 = above rows 12..15, cols 0..3 = left columns 12..15
constexpr int TCS = 12;   // chroma tile: 10 rows x 12 (10 used), rows 0..1 = above rows 6..7, cols 0..1 = left columns 6..7

struct __attribute__((aligned(16))) DbBlock {
    int     progress[16];   // macroblock steps completed by wave w (monotonic over its rows)
    int     abort_flag;
    int     pad[3];
    uint8_t alpha[52], beta[52], tc0[52], qpc[22], pad2[14];
};

struct __attribute__((aligned(16))) DbWave {
    uint8_t ty[TYS * TYS];
    uint8_t tc[2][10 * TCS];
    uint8_t pad[16 - (TYS * TYS + 2 * 10 * TCS) % 16];
};

__constant__ uint8_t c_db_alpha[52] = MVDB_ALPHA_TABLE;
__constant__ uint8_t c_db_beta[52] = MVDB_BETA_TABLE;
__constant__ uint8_t c_db_tc0[52] = MVDB_TC0_BS3_TABLE;
__constant__ uint8_t c_db_qpc[22] = MVDB_QPC_TABLE;

// what the filter needs of one macroblock's header: QP for this lane's plane, disable_deblocking_filter_idc, offsets, unavail
struct DbMb {
    int qp, idc, a2, b2, t8, un;
};

__device__ __forceinline__ int sext4(uint32_t v) { return (int)((v & 15u) ^ 8u) - 8; }

__device__ __forceinline__ DbMb db_mb(const uint8_t *rec, int plane, int cqp_cb, int cqp_cr, const uint8_t *qpc)
{
    const uint2 h = *reinterpret_cast<const uint2 *>(rec);
    DbMb m;
    const int kind = h.x & 255;
    const int qpy = mvdb::filter_qp(kind, (h.x >> 8) & 255);
    m.qp = plane == 0 ? qpy : mvdb::qpc_of(qpy, plane == 1 ? cqp_cb : cqp_cr, qpc);
    m.idc = (h.y >> 9) & 3;
    const uint32_t off = h.y >> 24;
    m.a2 = sext4(off);
    m.b2 = sext4(off >> 4);
    m.t8 = kind == MVHP_KIND_I8x8;
    m.un = (h.y >> 16) & 255;
    return m;
}

// the edges of one macroblock in one direction on this lane's line v[0..19]: luma v[4..19] = the macroblock, v[0..3] = the
// neighbour; chroma v[4..11] = the macroblock, v[2..3] = the neighbour.  Edge k sits between v[4k + 3] and v[4k + 4].
__device__ __forceinline__ void db_line(int *v, bool chroma, bool mb_edge, int qp_nb, const DbMb &m, const DbBlock &B)
{
    if (mb_edge) {
        const mvdb::EdgeParams e = mvdb::edge_params((qp_nb + m.qp + 1) >> 1, m.a2, m.b2, 1, B.alpha, B.beta, B.tc0);
        mvdb::filter_line(v + 0, e, chroma);
    }
    const mvdb::EdgeParams e = mvdb::edge_params(m.qp, m.a2, m.b2, 0, B.alpha, B.beta, B.tc0);
    if (!chroma) {
        if (!m.t8) mvdb::filter_line(v + 4, e, false);
        mvdb::filter_line(v + 8, e, false);
        if (!m.t8) mvdb::filter_line(v + 12, e, false);
    } else {
        mvdb::filter_line(v + 4, e, true);
    }
}

} // namespace

template <int NW>
__global__ __launch_bounds__(NW * 64) void deblock_kernel(DeblockArgs a)
{
    extern __shared__ __attribute__((aligned(16))) uint8_t smem[];
    const int W = a.width_mbs, H = a.height_mbs;
    DbBlock &B = *reinterpret_cast<DbBlock *>(smem);
    uint8_t *lb_y = smem + sizeof(DbBlock);          // [4][W * 16]: luma rows 12..15 of the row above
    uint8_t *lb_c = lb_y + (size_t)W * 64;           // [2 planes][2][W * 8]: chroma rows 6..7
    const int wave = __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
    const int lane = threadIdx.x & 63;
    DbWave &T = *reinterpret_cast<DbWave *>(lb_c + (size_t)W * 32 + (size_t)wave * sizeof(DbWave));

    for (int i = threadIdx.x; i < 52; i += NW * 64) {
        B.alpha[i] = c_db_alpha[i];
        B.beta[i] = c_db_beta[i];
        B.tc0[i] = c_db_tc0[i];
        if (i < 22) B.qpc[i] = c_db_qpc[i];
    }
    if (threadIdx.x < 16) B.progress[threadIdx.x] = 0;
    if (threadIdx.x == 16) B.abort_flag = 0;
    __syncthreads();

    const int frame = (int)blockIdx.x;
    const size_t pitch = (size_t)W * 16, cpitch = (size_t)W * 8;
    uint8_t *fy = a.yuv + (size_t)frame * W * H * 384;
    uint8_t *fc[2] = {fy + (size_t)W * H * 256, fy + (size_t)W * H * 320};
    const uint8_t *recs = a.packed + (size_t)frame * W * H * MVHP_MB_BYTES;

    // this lane's line: luma lanes 0..15, Cb 16..23, Cr 24..31 (lanes 32..63 only help with the stores)
    const bool active = lane < 32;
    const int plane = lane < 16 ? 0 : (lane < 24 ? 1 : 2);
    const bool chroma = plane != 0;
    const int li = lane < 16 ? lane : (lane & 7);     // line index inside the macroblock
    const int cp = plane - 1;                          // chroma plane index (lanes 16..31)

    int done = 0;
    for (int row = wave; row < H; row += NW) {
        const int up_wave = (row + NW - 1) % NW;
        const int up_base = ((row - 1) / NW) * W;      // steps of up_wave before row - 1 (unused for row 0)
        const bool last_row = row == H - 1;
        int qp_left = 0;
        for (int x = 0; x < W; x++) {
            const uint8_t *rec = recs + (size_t)(row * W + x) * MVHP_MB_BYTES;
            const DbMb m = db_mb(rec, plane, a.cqp_off_cb, a.cqp_off_cr, B.qpc);
            const bool on = m.idc != 1;
            const bool left = on && x > 0 && !(m.idc == 2 && (m.un & MVHP_UNAVAIL_A));
            const bool top = on && row > 0 && !(m.idc == 2 && (m.un & MVHP_UNAVAIL_B));
            const int qp_top = row > 0 ? db_mb(rec - (size_t)W * MVHP_MB_BYTES, plane, a.cqp_off_cb, a.cqp_off_cr, B.qpc).qp : 0;

            // ---- wait for row - 1 to have finished MB(x + 1, row - 1) ----
            if (row > 0) {
                const int need = up_base + min(x + 2, W);
                int spins = 0;
                while (__hip_atomic_load(&B.progress[up_wave], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP) < need) {
                    __builtin_amdgcn_s_sleep(1);
                    if (++spins > (1 << 22) || __hip_atomic_load(&B.abort_flag, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP)) {
                        if (lane == 0) {
                            __hip_atomic_store(&B.abort_flag, 1, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
                            atomicOr(a.err, 4u);
                        }
                        return;
                    }
                }
                __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "workgroup");
            }

            // ---- vertical edges: lane = one row of the macroblock plus the columns left of it ----
            int v[20];
#pragma unroll
            for (int i = 0; i < 20; i++) v[i] = 0;
            if (active) {
                if (!chroma) {
                    const uint32_t mg = *reinterpret_cast<const uint32_t *>(&T.ty[(4 + li) * TYS + 16]);
                    const uint4 s = *reinterpret_cast<const uint4 *>(fy + (size_t)(row * 16 + li) * pitch + x * 16);
                    const uint32_t w[5] = {mg, s.x, s.y, s.z, s.w};
#pragma unroll
                    for (int i = 0; i < 20; i++) v[i] = (w[i >> 2] >> ((i & 3) * 8)) & 255;
                } else {
                    const uint8_t *tr = &T.tc[cp][(2 + li) * TCS];
                    const uint2 s = *reinterpret_cast<const uint2 *>(fc[cp] + (size_t)(row * 8 + li) * cpitch + x * 8);
                    v[2] = tr[8];
                    v[3] = tr[9];
#pragma unroll
                    for (int i = 0; i < 8; i++) v[4 + i] = (((i < 4) ? s.x : s.y) >> ((i & 3) * 8)) & 255;
                }
                if (on) db_line(v, chroma, left, qp_left, m, B);
                if (!chroma) {
#pragma unroll
                    for (int i = 0; i < 20; i++) T.ty[(4 + li) * TYS + i] = (uint8_t)v[i];
                } else {
#pragma unroll
                    for (int i = 2; i < 12; i++) T.tc[cp][(2 + li) * TCS + i - 2] = (uint8_t)v[i];
                }
            }
            WAVE_SYNC();

            // ---- horizontal edges: lane = one column of the macroblock plus the rows above it (line buffer) ----
            if (active) {
#pragma unroll
                for (int i = 0; i < 20; i++) v[i] = 0;
                if (!chroma) {
                    if (row > 0) {
#pragma unroll
                        for (int k = 0; k < 4; k++) v[k] = lb_y[(size_t)k * pitch + x * 16 + li];
                    }
#pragma unroll
                    for (int k = 0; k < 16; k++) v[4 + k] = T.ty[(4 + k) * TYS + 4 + li];
                } else {
                    if (row > 0) {
                        v[2] = lb_c[(size_t)(cp * 2 + 0) * cpitch + x * 8 + li];
                        v[3] = lb_c[(size_t)(cp * 2 + 1) * cpitch + x * 8 + li];
                    }
#pragma unroll
                    for (int k = 0; k < 8; k++) v[4 + k] = T.tc[cp][(2 + k) * TCS + 2 + li];
                }
                if (on) db_line(v, chroma, top, qp_top, m, B);
                if (!chroma) {
#pragma unroll
                    for (int k = 0; k < 20; k++) T.ty[k * TYS + 4 + li] = (uint8_t)v[k];
                } else {
#pragma unroll
                    for (int k = 2; k < 12; k++) T.tc[cp][(k - 2) * TCS + 2 + li] = (uint8_t)v[k];
                }
            }
            WAVE_SYNC();

            // ---- write-out ----
            // luma rows 13..15 of the row above (the top edge's p side): 3 rows x 4 dwords
            if (row > 0 && lane < 12) {
                const int r = 1 + (lane >> 2), d = lane & 3;
                *reinterpret_cast<uint32_t *>(fy + (size_t)(row * 16 - 4 + r) * pitch + x * 16 + d * 4) =
                    *reinterpret_cast<const uint32_t *>(&T.ty[r * TYS + 4 + d * 4]);
            }
            // chroma row 7 of the row above: 2 planes x 4 pairs
            if (row > 0 && lane >= 16 && lane < 24) {
                const int pl = (lane - 16) >> 2, d = lane & 3;
                *reinterpret_cast<uint16_t *>(fc[pl] + (size_t)(row * 8 - 1) * cpitch + x * 8 + d * 2) =
                    *reinterpret_cast<const uint16_t *>(&T.tc[pl][1 * TCS + 2 + d * 2]);
            }
            // luma of this row: 16 rows x 5 dwords (tile columns 4d .. 4d + 3 = picture columns 16x - 4 + 4d ..)
            for (int it = lane; it < 80; it += 64) {
                const int r = it / 5, d = it - r * 5;
                const bool col_ok = (d > 0 || x > 0) && (d < 4 || x == W - 1);
                if (!col_ok) continue;
                const uint32_t val = *reinterpret_cast<const uint32_t *>(&T.ty[(4 + r) * TYS + d * 4]);
                const size_t col = (size_t)x * 16 - 4 + d * 4;
                if (r <= 12 || last_row) *reinterpret_cast<uint32_t *>(fy + (size_t)(row * 16 + r) * pitch + col) = val;
                if (r >= 12 && !last_row) *reinterpret_cast<uint32_t *>(lb_y + (size_t)(r - 12) * pitch + col) = val;
            }
            // chroma of this row: 2 planes x 8 rows x 5 pairs
            for (int it = lane; it < 80; it += 64) {
                const int pl = it / 40, rem = it - pl * 40, r = rem / 5, d = rem - r * 5;
                const bool col_ok = (d > 0 || x > 0) && (d < 4 || x == W - 1);
                if (!col_ok) continue;
                const uint16_t val = *reinterpret_cast<const uint16_t *>(&T.tc[pl][(2 + r) * TCS + d * 2]);
                const size_t col = (size_t)x * 8 - 2 + d * 2;
                if (r <= 6 || last_row) *reinterpret_cast<uint16_t *>(fc[pl] + (size_t)(row * 8 + r) * cpitch + col) = val;
                if (r >= 6 && !last_row) *reinterpret_cast<uint16_t *>(lb_c + (size_t)(pl * 2 + r - 6) * cpitch + col) = val;
            }
            qp_left = m.qp;

            // ---- publish: the line-buffer writes land before the counter ----
            done++;
            __builtin_amdgcn_fence(__ATOMIC_RELEASE, "workgroup");
            if (lane == 0) __hip_atomic_store(&B.progress[wave], done, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
            WAVE_SYNC();
        }
    }
}

size_t deblock_lds_bytes(int width_mbs, int nw)
{
    return sizeof(DbBlock) + (size_t)width_mbs * 96 + (size_t)nw * sizeof(DbWave);
}

int deblock_waves(int n_frames) { return n_frames >= 512 ? 4 : 16; }

template <int NW>
static hipError_t launch_deblock_one(const DeblockArgs &a, hipStream_t stream)
{
    const size_t lds = deblock_lds_bytes(a.width_mbs, NW);
    hipError_t e = hipFuncSetAttribute((const void *)deblock_kernel<NW>, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds);
    if (e != hipSuccess) return e;
    hipLaunchKernelGGL(deblock_kernel<NW>, dim3(a.n_frames), dim3(NW * 64), lds, stream, a);
    return hipGetLastError();
}

hipError_t launch_deblock(const DeblockArgs &a, int nw, hipStream_t stream)
{
    if (a.n_frames <= 0) return hipSuccess;
    switch (nw) {
    case 4: return launch_deblock_one<4>(a, stream);
    case 16: return launch_deblock_one<16>(a, stream);
    default: return hipErrorInvalidValue;
    }
}

} // namespace mvhp
