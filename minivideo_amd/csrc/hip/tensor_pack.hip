// tensor_pack.hip -- tensor output (opt-in; DESIGN.md 3 "Tensor output"): dense RGB8 pictures -> normalised float tensors of one
// fixed shape (F32 / F16 / BF16, NCHW / NHWC, R,G,B or B,G,R), the picture centred on a padded canvas, gfx950.  A streaming
// kernel: 3 bytes in and 6 to 12 bytes out per pixel, nothing shared between workgroups or launches.
//
// Mapping: one workgroup of 256 threads per (strip of `rows` canvas rows, picture); strips in grid.x, pictures in grid.y (at most
// 65535 a launch).  The source rows of a strip are ONE run of bytes of the dense picture, and the strip's part of an output plane
// (NCHW; NHWC: of the interleaved picture) is ONE run of bytes of the tensor, so both sides are handled as runs, not row by row:
// * in: the run is cut at the 16-byte boundaries of the SOURCE ADDRESS and copied to LDS chunk by chunk, lane t chunk t, t + 256,
//   ...: one aligned dwordx4 per lane, whatever byte phase 3 * src_w leaves the rows on.  LDS keeps that phase.  Only the chunk
//   that holds the first or the last byte of the whole call's pictures can reach outside them; it is gathered byte by byte
//   under a predicate -- nothing outside [src, src_end) is read.
// * out: the run is cut at the 16-byte boundaries of the DESTINATION ADDRESS; lane t makes the 4 (F32) or 8 (F16, BF16) elements
//   of chunk t, t + 256, ... -- one division per chunk finds the first element's row, column and channel, the others follow by
//   stepping -- and stores one aligned dwordx4.  The run's first and last chunk (odd canvases with 2-byte elements and slots of
//   any length put run starts on every even byte) store their elements of the run one by one; nothing outside the run is written.
//   The samples come out of LDS as bytes (a lane's elements lie 1 or 3 bytes apart there); pad elements take the pad colour's
//   sample through the same arithmetic.
// Arithmetic: fmaf((float)c, scale[k], bias[k]), then the element type's round-to-nearest-even.  hipcc compiles kernels with f32
// and f16 subnormals kept (the kernel descriptor's denorm modes; this file asks for nothing else), so v_fma_f32 and v_cvt_f16_f32
// deliver them; bfloat16 is rounded in integers on the bit pattern.
#include <hip/hip_fp16.h>
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "minivideo_hotpath.h"
#include "recon_kernels.h"

namespace mvhp {

namespace {

constexpr int kThreads = 256;

template <int DT> __device__ __forceinline__ uint32_t element_bits(float v)
{
    if (DT == MVHP_TENSOR_F32) return __float_as_uint(v);
    if (DT == MVHP_TENSOR_F16) return (uint32_t)__half_as_ushort(__float2half_rn(v));
    const uint32_t u = __float_as_uint(v);   // (scale and bias are finite: v is never a NaN)
    return (u + 0x7fffu + ((u >> 16) & 1u)) >> 16;
}

// the elements [max(e0, 0), min(e0 + 16 / ES, run_elems)) of the chunk at q, which holds elements e0 .. e0 + 16 / ES of a run, one
// store each.  Not inlined: next to the whole-chunk store the compiler otherwise merges the two paths' first words and splits the
// dwordx4 into a dwordx3 and a dword.
template <int ES> __device__ __noinline__ void store_partial(uint8_t *q, uint4 v, int e0, int run_elems)
{
    const uint32_t w[4] = {v.x, v.y, v.z, v.w};
#pragma unroll
    for (int j = 0; j < 16 / ES; j++) {
        if (e0 + j < 0 || e0 + j >= run_elems) continue;
        if (ES == 4) reinterpret_cast<uint32_t *>(q)[j] = w[j];
        else reinterpret_cast<uint16_t *>(q)[j] = (uint16_t)(w[j >> 1] >> (16 * (j & 1)));
    }
}

template <int DT, int LAYOUT> __global__ __launch_bounds__(256) void tensor_kernel(TensorArgs a)
{
    extern __shared__ __attribute__((aligned(16))) uint8_t lds[];
    constexpr int ES = DT == MVHP_TENSOR_F32 ? 4 : 2;   // bytes per element
    constexpr int EPC = 16 / ES;                        // elements per chunk
    constexpr bool kInterleaved = LAYOUT == MVHP_TENSOR_NHWC;
    const int pic = a.first + (int)blockIdx.y;
    const int slot = a.slots ? a.slots[pic] : pic;
    if (slot < 0) return;                               // (the whole workgroup)
    const int y0 = (int)blockIdx.x * a.rows;
    const int nr = min(a.rows, a.ch - y0);
    if (nr <= 0) return;
    const int t = threadIdx.x;
    const int ox = (a.cw - a.sw) >> 1, oy = (a.ch - a.sh) >> 1;

    // ---- in: the source rows of the strip, one run of bytes
    const int sy0 = max(y0 - oy, 0), sy1 = min(y0 + nr - oy, a.sh);
    int phase = 0;
    if (sy1 > sy0) {
        const size_t row_bytes = (size_t)3 * a.sw;
        const uint8_t *run = a.src + (size_t)pic * row_bytes * a.sh + (size_t)sy0 * row_bytes;
        const int run_bytes = (sy1 - sy0) * (int)row_bytes;
        phase = (int)((uintptr_t)run & 15);
        const uint8_t *run0 = run - phase;
        const int chunks = (phase + run_bytes + 15) >> 4;
        for (int c = t; c < chunks; c += kThreads) {
            const uint8_t *q = run0 + (size_t)c * 16;
            uint4 v;
            if (q >= a.src && q + 16 <= a.src_end) {
                v = *reinterpret_cast<const uint4 *>(q);
            } else {   // the chunk of the call's first or last byte
                uint32_t w[4] = {0u, 0u, 0u, 0u};
#pragma unroll
                for (int j = 0; j < 16; j++)
                    if (q + j >= a.src && q + j < a.src_end) w[j >> 2] |= (uint32_t)q[j] << (8 * (j & 3));
                v = make_uint4(w[0], w[1], w[2], w[3]);
            }
            *reinterpret_cast<uint4 *>(lds + c * 16) = v;
        }
    }
    __syncthreads();

    // ---- out: the strip's run of each plane (NCHW) or of the interleaved picture (NHWC)
    uint8_t *tensor = a.out + (size_t)slot * a.tensor_bytes;
    const int run_elems = nr * a.cw * (kInterleaved ? 3 : 1);
    const uint32_t pad[3] = {(a.pad_rgb >> 16) & 255u, (a.pad_rgb >> 8) & 255u, a.pad_rgb & 255u};
    for (int p = 0; p < (kInterleaved ? 1 : 3); p++) {
        const size_t first_elem = kInterleaved ? (size_t)y0 * a.cw * 3 : ((size_t)p * a.ch + y0) * a.cw;
        uint8_t *run = tensor + first_elem * ES;
        const int head = (int)((uintptr_t)run & 15);   // (a multiple of ES: `out` is 16-byte aligned, everything else counts elements)
        uint8_t *run0 = run - head;
        const int chunks = (head + run_elems * ES + 15) >> 4;
        for (int c = t; c < chunks; c += kThreads) {
            const int e0 = (c * 16 - head) / ES;        // the chunk's first element in the run; negative inside the first chunk
            const int s0 = max(e0, 0);
            int pix = kInterleaved ? s0 / 3 : s0;
            int pos = kInterleaved ? s0 - pix * 3 : p;  // position in the channel order
            int ry = pix / a.cw;
            int x = pix - ry * a.cw;
            uint32_t w[4] = {0u, 0u, 0u, 0u};
#pragma unroll
            for (int j = 0; j < EPC; j++) {
                const int e = e0 + j;
                const bool valid = e >= 0 && e < run_elems;
                const int k = a.bgr ? 2 - pos : pos;    // colour
                const int sy = y0 + ry - oy, sx = x - ox;
                const bool inside = valid && (unsigned)sy < (unsigned)a.sh && (unsigned)sx < (unsigned)a.sw;
                const int li = inside ? ((sy - sy0) * a.sw + sx) * 3 + k + phase : 0;
                const uint32_t from_lds = lds[li];
                const uint32_t smp = inside ? from_lds : (k == 0 ? pad[0] : k == 1 ? pad[1] : pad[2]);
                const float sc = k == 0 ? a.scale[0] : k == 1 ? a.scale[1] : a.scale[2];
                const float bi = k == 0 ? a.bias[0] : k == 1 ? a.bias[1] : a.bias[2];
                const uint32_t bits = element_bits<DT>(fmaf((float)smp, sc, bi));
                if (ES == 4) w[j] = bits;
                else w[j >> 1] |= bits << (16 * (j & 1));
                if (e >= 0) {                           // the next element of the run
                    if (kInterleaved && ++pos < 3) continue;
                    if (kInterleaved) pos = 0;
                    if (++x == a.cw) { x = 0; ry++; }
                }
            }
            uint8_t *q = run0 + (size_t)c * 16;
            if (e0 >= 0 && e0 + EPC <= run_elems) {
                *reinterpret_cast<uint4 *>(q) = make_uint4(w[0], w[1], w[2], w[3]);
            } else {   // the run's first or last chunk: its elements of the run only
                store_partial<ES>(q, make_uint4(w[0], w[1], w[2], w[3]), e0, run_elems);
            }
        }
    }
}

template <int DT> hipError_t launch_layout(const TensorArgs &b, dim3 grid, size_t lds_bytes, hipStream_t stream)
{
    if (b.layout == MVHP_TENSOR_NHWC) hipLaunchKernelGGL((tensor_kernel<DT, MVHP_TENSOR_NHWC>), grid, dim3(kThreads), lds_bytes, stream, b);
    else hipLaunchKernelGGL((tensor_kernel<DT, MVHP_TENSOR_NCHW>), grid, dim3(kThreads), lds_bytes, stream, b);
    return hipGetLastError();
}

} // namespace

size_t tensor_lds_bytes(int rows, int sw)
{
    // the strip's source rows, up to 15 bytes in front of them and the rest of the last chunk
    return (((size_t)rows * 3 * (size_t)sw + 15 + 15) & ~(size_t)15) + 16;
}

hipError_t launch_tensor(const TensorArgs &a, hipStream_t stream)
{
    if (a.n == 0) return hipSuccess;
    TensorArgs b = a;
    if (b.rows < 1) b.rows = 1;
    const int strips = (b.ch + b.rows - 1) / b.rows;                       // (at most 16384: grid x)
    int per_launch = (1 << 23) / strips > 0 ? (1 << 23) / strips : 1;      // (a grid holds fewer than 2^32 threads)
    if (per_launch > 65535) per_launch = 65535;                            // (grid y)
    const size_t lds_bytes = tensor_lds_bytes(b.rows, b.sw);
    for (int first = 0; first < a.n; first += per_launch) {
        b.n = a.n - first < per_launch ? a.n - first : per_launch;
        b.first = a.first + first;
        const dim3 grid((unsigned)strips, (unsigned)b.n);
        const hipError_t e = b.dtype == MVHP_TENSOR_F32  ? launch_layout<MVHP_TENSOR_F32>(b, grid, lds_bytes, stream)
                             : b.dtype == MVHP_TENSOR_F16 ? launch_layout<MVHP_TENSOR_F16>(b, grid, lds_bytes, stream)
                                                          : launch_layout<MVHP_TENSOR_BF16>(b, grid, lds_bytes, stream);
        if (e != hipSuccess) return e;
    }
    return hipSuccess;
}

} // namespace mvhp
