// jpeg_encode.hip -- baseline JPEG (JFIF, 4:2:0, Annex K tables, restart intervals) from planar Y | Cb | Cr pictures on the
// device (DESIGN.md 3 "JPEG output"; tests/jpeg_ref.py states the same arithmetic in NumPy).
//
//   jpeg_dct_kernel      forward DCT + quantisation: eight lanes per 8x8 block (one per row, then one per column), levels in
//                        zigzag order as int16 plus a 64-bit map of the non-zero ones into the scratch buffer
//   jpeg_huff_kernel<0>  count: one lane per restart interval Huffman-codes its blocks (it walks the set bits of the maps, so a
//                        lane's trip count is its number of non-zero levels; the levels of a block come through a row of LDS
//                        per lane, the next block's already on their way) and writes the interval's byte length, stuffing and
//                        marker included
//   jpeg_scan_kernel     per picture: exclusive scan of the interval lengths (-> offsets inside the file) and the file's length
//   blob_place_kernel    (blob_place.h) one workgroup: pictures in order at 16-byte-aligned offsets of the blob, {offset, length, status} each;
//                        a picture that does not fit gets length 0 and takes no room
//   jpeg_huff_kernel<1>  write: the same walk again, storing the bytes at the offsets
//   jpeg_head_kernel     one wavefront per picture: the 625 header bytes and the EOI
// Nothing is shared between workgroups but the scratch buffer between launches; no waits inside a kernel.
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <string.h>

#include "blob_place.h"
#include "minivideo_hotpath.h"
#include "recon_kernels.h"

namespace mvhp {

namespace {

const uint8_t kBaseQ[2][64] = {   // Annex K.1 / K.2, row-major
    {16, 11, 10, 16, 24, 40, 51, 61, 12, 12, 14, 19, 26, 58, 60, 55, 14, 13, 16, 24, 40, 57, 69, 56,
     14, 17, 22, 29, 51, 87, 80, 62, 18, 22, 37, 56, 68, 109, 103, 77, 24, 35, 55, 64, 81, 104, 113, 92,
     49, 64, 78, 87, 103, 121, 120, 101, 72, 92, 95, 98, 112, 100, 103, 99},
    {17, 18, 24, 47, 99, 99, 99, 99, 18, 21, 26, 66, 99, 99, 99, 99, 24, 26, 56, 99, 99, 99, 99, 99,
     47, 66, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99,
     99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99}};

// Annex K.3: BITS (codes per length 1..16) and HUFFVAL of the four typical tables
const uint8_t kDcBits[2][16] = {{0, 1, 5, 1, 1, 1, 1, 1, 1, 0, 0, 0, 0, 0, 0, 0}, {0, 3, 1, 1, 1, 1, 1, 1, 1, 1, 1, 0, 0, 0, 0, 0}};
const uint8_t kAcBits[2][16] = {{0, 2, 1, 3, 3, 2, 4, 3, 5, 5, 4, 4, 0, 0, 1, 0x7d}, {0, 2, 1, 2, 4, 4, 3, 4, 7, 5, 4, 4, 0, 1, 2, 0x77}};
const uint8_t kAcVals[2][162] = {
    {0x01, 0x02, 0x03, 0x00, 0x04, 0x11, 0x05, 0x12, 0x21, 0x31, 0x41, 0x06, 0x13, 0x51, 0x61, 0x07, 0x22, 0x71, 0x14, 0x32,
     0x81, 0x91, 0xa1, 0x08, 0x23, 0x42, 0xb1, 0xc1, 0x15, 0x52, 0xd1, 0xf0, 0x24, 0x33, 0x62, 0x72, 0x82, 0x09, 0x0a, 0x16,
     0x17, 0x18, 0x19, 0x1a, 0x25, 0x26, 0x27, 0x28, 0x29, 0x2a, 0x34, 0x35, 0x36, 0x37, 0x38, 0x39, 0x3a, 0x43, 0x44, 0x45,
     0x46, 0x47, 0x48, 0x49, 0x4a, 0x53, 0x54, 0x55, 0x56, 0x57, 0x58, 0x59, 0x5a, 0x63, 0x64, 0x65, 0x66, 0x67, 0x68, 0x69,
     0x6a, 0x73, 0x74, 0x75, 0x76, 0x77, 0x78, 0x79, 0x7a, 0x83, 0x84, 0x85, 0x86, 0x87, 0x88, 0x89, 0x8a, 0x92, 0x93, 0x94,
     0x95, 0x96, 0x97, 0x98, 0x99, 0x9a, 0xa2, 0xa3, 0xa4, 0xa5, 0xa6, 0xa7, 0xa8, 0xa9, 0xaa, 0xb2, 0xb3, 0xb4, 0xb5, 0xb6,
     0xb7, 0xb8, 0xb9, 0xba, 0xc2, 0xc3, 0xc4, 0xc5, 0xc6, 0xc7, 0xc8, 0xc9, 0xca, 0xd2, 0xd3, 0xd4, 0xd5, 0xd6, 0xd7, 0xd8,
     0xd9, 0xda, 0xe1, 0xe2, 0xe3, 0xe4, 0xe5, 0xe6, 0xe7, 0xe8, 0xe9, 0xea, 0xf1, 0xf2, 0xf3, 0xf4, 0xf5, 0xf6, 0xf7, 0xf8,
     0xf9, 0xfa},
    {0x00, 0x01, 0x02, 0x03, 0x11, 0x04, 0x05, 0x21, 0x31, 0x06, 0x12, 0x41, 0x51, 0x07, 0x61, 0x71, 0x13, 0x22, 0x32, 0x81,
     0x08, 0x14, 0x42, 0x91, 0xa1, 0xb1, 0xc1, 0x09, 0x23, 0x33, 0x52, 0xf0, 0x15, 0x62, 0x72, 0xd1, 0x0a, 0x16, 0x24, 0x34,
     0xe1, 0x25, 0xf1, 0x17, 0x18, 0x19, 0x1a, 0x26, 0x27, 0x28, 0x29, 0x2a, 0x35, 0x36, 0x37, 0x38, 0x39, 0x3a, 0x43, 0x44,
     0x45, 0x46, 0x47, 0x48, 0x49, 0x4a, 0x53, 0x54, 0x55, 0x56, 0x57, 0x58, 0x59, 0x5a, 0x63, 0x64, 0x65, 0x66, 0x67, 0x68,
     0x69, 0x6a, 0x73, 0x74, 0x75, 0x76, 0x77, 0x78, 0x79, 0x7a, 0x82, 0x83, 0x84, 0x85, 0x86, 0x87, 0x88, 0x89, 0x8a, 0x92,
     0x93, 0x94, 0x95, 0x96, 0x97, 0x98, 0x99, 0x9a, 0xa2, 0xa3, 0xa4, 0xa5, 0xa6, 0xa7, 0xa8, 0xa9, 0xaa, 0xb2, 0xb3, 0xb4,
     0xb5, 0xb6, 0xb7, 0xb8, 0xb9, 0xba, 0xc2, 0xc3, 0xc4, 0xc5, 0xc6, 0xc7, 0xc8, 0xc9, 0xca, 0xd2, 0xd3, 0xd4, 0xd5, 0xd6,
     0xd7, 0xd8, 0xd9, 0xda, 0xe2, 0xe3, 0xe4, 0xe5, 0xe6, 0xe7, 0xe8, 0xe9, 0xea, 0xf2, 0xf3, 0xf4, 0xf5, 0xf6, 0xf7, 0xf8,
     0xf9, 0xfa}};

// kZigzag[k] = row-major index (v * 8 + u) of the k-th coefficient in zigzag order
const uint8_t kZigzag[64] = {0,  1,  8,  16, 9,  2,  3,  10, 17, 24, 32, 25, 18, 11, 4,  5,  12, 19, 26, 33, 40, 48,
                             41, 34, 27, 20, 13, 6,  7,  14, 21, 28, 35, 42, 49, 56, 57, 50, 43, 36, 29, 22, 15, 23,
                             30, 37, 44, 51, 58, 59, 52, 45, 38, 31, 39, 46, 53, 60, 61, 54, 47, 55, 62, 63};

// kernel arguments passed by value (the launches keep no state on the device)
struct JpegShape {
    int w, h;             // picture
    int mw, mcus;         // MCUs per row, per picture
    int restart, ipp;     // MCUs per restart interval, intervals per picture
    int n;
};
struct JpegQuant { uint8_t q[2][64]; uint8_t zzpos[64]; };   // row-major tables; zzpos[v * 8 + u] = zigzag position
struct JpegCodes { uint32_t dc[2][12]; uint32_t ac[2][256]; };   // (length << 16) | code, indexed by category / by (run << 4) | size
struct JpegHeader { uint8_t b[640]; };

void build_codes(const uint8_t *bits, const uint8_t *vals, uint32_t *out)
{
    uint32_t code = 0;
    int k = 0;
    for (int len = 1; len <= 16; len++) {   // Annex C
        for (int i = 0; i < bits[len - 1]; i++) out[vals[k++]] = ((uint32_t)len << 16) | code++;
        code <<= 1;
    }
}

// round(2^14 * c(u) / 2 * cos((2x + 1) u pi / 16))
#define MVHP_JPEG_M                                                                                                             \
    {{5793, 5793, 5793, 5793, 5793, 5793, 5793, 5793},     {8035, 6811, 4551, 1598, -1598, -4551, -6811, -8035},                 \
     {7568, 3135, -3135, -7568, -7568, -3135, 3135, 7568}, {6811, -1598, -8035, -4551, 4551, 8035, 1598, -6811},                 \
     {5793, -5793, -5793, 5793, 5793, -5793, -5793, 5793}, {4551, -8035, 1598, 6811, -6811, -1598, 8035, -4551},                 \
     {3135, -7568, 7568, -3135, -3135, 7568, -7568, 3135}, {1598, -4551, 6811, -8035, 8035, -6811, 4551, -1598}}

constexpr int kDctBlocks = 32;   // 8x8 blocks per workgroup of 256 lanes

__global__ __launch_bounds__(256) void jpeg_dct_kernel(const uint8_t *__restrict__ yuv, JpegShape g, JpegQuant qt,
                                                       int16_t *__restrict__ coefs, uint64_t *__restrict__ maps,
                                                       long long total_blocks)
{
    constexpr int M[8][8] = MVHP_JPEG_M;
    __shared__ int s_t[kDctBlocks][8][9];
    __shared__ __attribute__((aligned(16))) int16_t s_lv[kDctBlocks][64];
    __shared__ uint8_t s_q[128];
    __shared__ uint8_t s_zz[64];
    const int tid = threadIdx.x, lb = tid >> 3, r = tid & 7;
    if (tid < 128) s_q[tid] = qt.q[tid >> 6][tid & 63];
    if (tid < 64) s_zz[tid] = qt.zzpos[tid];
    long long blk = (long long)blockIdx.x * kDctBlocks + lb;
    const bool live = blk < total_blocks;
    if (!live) blk = 0;   // (computes block 0 again and stores nothing: every lane reaches the barriers)
    const int per_pic = g.mcus * 6;
    const long long pic = blk / per_pic;
    const int rem = (int)(blk - pic * per_pic);
    const int m = rem / 6, k = rem - m * 6;
    const int my = m / g.mw, mx = m - my * g.mw;
    const size_t frame = (size_t)g.w * g.h * 3 / 2;
    const uint8_t *plane = yuv + (size_t)pic * frame;
    int pw, ph, x0, y0;
    if (k < 4) {
        pw = g.w; ph = g.h; x0 = mx * 16 + (k & 1) * 8; y0 = my * 16 + (k >> 1) * 8;
    } else {
        pw = g.w / 2; ph = g.h / 2; x0 = mx * 8; y0 = my * 8;
        plane += (size_t)g.w * g.h + (size_t)(k - 4) * pw * ph;
    }
    {   // rows: lane r transforms row r (samples beyond the picture repeat the last column / row)
        const uint8_t *row = plane + (size_t)min(y0 + r, ph - 1) * pw;
        int s[8];
#pragma unroll
        for (int x = 0; x < 8; x++) s[x] = (int)row[min(x0 + x, pw - 1)] - 128;
#pragma unroll
        for (int u = 0; u < 8; u++) {
            int a = 0;
#pragma unroll
            for (int x = 0; x < 8; x++) a += M[u][x] * s[x];
            s_t[lb][r][u] = (a + 128) >> 8;   // 6 fractional bits; |a| <= 128 * 46344, |t| <= 23173
        }
    }
    __syncthreads();
    {   // columns: lane r transforms column u = r and quantises it; |z| <= 46344 * 23173 < 2^30.01
        int t[8];
#pragma unroll
        for (int y = 0; y < 8; y++) t[y] = s_t[lb][y][r];
        const uint8_t *q = s_q + (k >= 4 ? 64 : 0);
#pragma unroll
        for (int v = 0; v < 8; v++) {
            int z = 0;
#pragma unroll
            for (int y = 0; y < 8; y++) z += M[v][y] * t[y];
            const uint32_t qq = q[v * 8 + r];
            const uint32_t a = (uint32_t)(z < 0 ? -z : z);
            const int lv = (int)((a + (qq << 19)) / (qq << 20));   // z / 2^20 / q to nearest, ties away from zero
            s_lv[lb][s_zz[v * 8 + r]] = (int16_t)(z < 0 ? -lv : lv);
        }
    }
    __syncthreads();
    {   // lane r stores zigzag positions 8r .. 8r + 7 (16 bytes) and its byte of the non-zero map
        const uint4 w = *reinterpret_cast<const uint4 *>(&s_lv[lb][r * 8]);
        const uint32_t ws[4] = {w.x, w.y, w.z, w.w};
        uint32_t bits = 0;
#pragma unroll
        for (int i = 0; i < 4; i++) bits |= ((ws[i] & 0xffffu) ? 1u << (2 * i) : 0u) | ((ws[i] >> 16) ? 2u << (2 * i) : 0u);
        unsigned long long map = (unsigned long long)bits << (8 * r);
        map |= __shfl_xor(map, 1);
        map |= __shfl_xor(map, 2);
        map |= __shfl_xor(map, 4);
        if (live) {
            *reinterpret_cast<uint4 *>(coefs + (size_t)blk * 64 + r * 8) = w;
            if (r == 0) maps[blk] = map;
        }
    }
}

// One lane per restart interval.  WRITE = false: lens[i] = bytes of interval i, marker included.  WRITE = true: lens[i] is the
// interval's offset inside its file (jpeg_scan_kernel) and the bytes are stored; nothing is stored at or beyond the file's length.
template <bool WRITE>
__global__ __launch_bounds__(64) void jpeg_huff_kernel(JpegShape g, JpegCodes codes, const int16_t *__restrict__ coefs,
                                                       const uint64_t *__restrict__ maps, uint32_t *__restrict__ lens,
                                                       const mvhp_jpeg_entry_t *__restrict__ table, uint8_t *__restrict__ blob,
                                                       unsigned long long cap)
{
    __shared__ uint32_t s_dc[2][12];
    __shared__ uint32_t s_ac[2][256];
    __shared__ __attribute__((aligned(8))) uint32_t s_blk[64][34];   // two levels per word, zigzag order
    const int tid = threadIdx.x;
    for (int i = tid; i < 24; i += 64) s_dc[i / 12][i % 12] = codes.dc[i / 12][i % 12];
    for (int i = tid; i < 512; i += 64) s_ac[i >> 8][i & 255] = codes.ac[i >> 8][i & 255];
    __syncthreads();
    const long long i = (long long)blockIdx.x * 64 + tid;
    if (i >= (long long)g.n * g.ipp) return;
    const long long pic = i / g.ipp;
    const int r = (int)(i - pic * g.ipp);
    const int m0 = r * g.restart, m1 = min(m0 + g.restart, g.mcus);
    uint8_t *out = nullptr;
    uint32_t limit = 0, pos = 0;
    if (WRITE) {
        const mvhp_jpeg_entry_t e = table[pic];
        // (the table is checked against the capacity again: a write stage run on its own trusts no earlier launch)
        if (e.status != MVHP_JPEG_OK || e.offset > cap || e.length > cap - e.offset) return;
        out = blob + e.offset;
        limit = e.length;
        pos = lens[i];
    }
    const uint32_t start = pos;
    unsigned long long acc = 0;
    int nb = 0;
    auto emit = [&](uint32_t byte) {
        if (WRITE && pos < limit) out[pos] = (uint8_t)byte;
        pos++;
    };
    auto put = [&](uint32_t bits, int len) {   // len <= 27; fewer than 8 bits are pending
        acc = (acc << len) | bits;
        nb += len;
        while (nb >= 8) {
            const uint32_t byte = (uint32_t)(acc >> (nb - 8)) & 0xffu;
            nb -= 8;
            emit(byte);
            if (byte == 0xffu) emit(0);
        }
    };
    int pred_y = 0, pred_cb = 0, pred_cr = 0;
    // A lane reads its block's levels from a row of LDS of its own (34 words apart: lanes that read the same position are two to a
    // bank), filled from registers that were loaded while the block before was coded: one global-memory latency per block instead
    // of one per non-zero level on the lane's serial path.
    uint32_t *row = &s_blk[tid][0];
    auto level = [&](int pos) { return (int)(int16_t)(row[pos >> 1] >> ((pos & 1) * 16)); };
    const size_t blk0 = ((size_t)pic * g.mcus + m0) * 6;
    const int n_blk = (m1 - m0) * 6;
    uint4 nxt[8];
    unsigned long long map_n = maps[blk0];
    {
        const uint4 *src = reinterpret_cast<const uint4 *>(coefs + blk0 * 64);
#pragma unroll
        for (int j = 0; j < 8; j++) nxt[j] = src[j];
    }
    for (int b = 0, k = 0; b < n_blk; b++, k = (k == 5 ? 0 : k + 1)) {
        {
#pragma unroll
            for (int j = 0; j < 8; j++) {
                row[4 * j] = nxt[j].x;
                row[4 * j + 1] = nxt[j].y;
                row[4 * j + 2] = nxt[j].z;
                row[4 * j + 3] = nxt[j].w;
            }
        }
        unsigned long long map = map_n & ~1ull;
        if (b + 1 < n_blk) {
            const uint4 *src = reinterpret_cast<const uint4 *>(coefs + (blk0 + b + 1) * 64);
#pragma unroll
            for (int j = 0; j < 8; j++) nxt[j] = src[j];
            map_n = maps[blk0 + b + 1];
        }
        const int tab = k >= 4;
        {
            const int dc = level(0);
            int d;
            if (k < 4) { d = dc - pred_y; pred_y = dc; }
            else if (k == 4) { d = dc - pred_cb; pred_cb = dc; }
            else { d = dc - pred_cr; pred_cr = dc; }
            {
                const int cat = min(32 - __clz(d < 0 ? -d : d), 11);
                const uint32_t e = s_dc[tab][cat];
                const uint32_t v = (uint32_t)(d < 0 ? d - 1 : d) & ((1u << cat) - 1u);
                put(((e & 0xffffu) << cat) | v, (int)(e >> 16) + cat);
            }
            int prev = 0;
            while (map) {
                const int pos_k = __ffsll((long long)map) - 1;
                map &= map - 1;
                int run = pos_k - prev - 1;
                prev = pos_k;
                while (run >= 16) {
                    const uint32_t e = s_ac[tab][0xf0];
                    put(e & 0xffffu, (int)(e >> 16));
                    run -= 16;
                }
                const int lv = level(pos_k);
                const int size = 32 - __clz(lv < 0 ? -lv : lv);
                const uint32_t e = s_ac[tab][((run << 4) | size) & 255];
                const uint32_t v = (uint32_t)(lv < 0 ? lv - 1 : lv) & ((1u << size) - 1u);
                put(((e & 0xffffu) << size) | v, (int)(e >> 16) + size);
            }
            if (prev != 63) {
                const uint32_t e = s_ac[tab][0];
                put(e & 0xffffu, (int)(e >> 16));
            }
        }
    }
    if (nb > 0) {   // pad with ones to the byte
        const int pad = 8 - nb;
        put((1u << pad) - 1u, pad);
    }
    if (r + 1 < g.ipp) {   // RSTm; the last interval is followed by the EOI (jpeg_head_kernel)
        emit(0xffu);
        emit(0xd0u + (uint32_t)(r & 7));
    } else {
        pos += 2;
    }
    if (!WRITE) lens[i] = pos - start;
}

__global__ __launch_bounds__(256) void jpeg_scan_kernel(JpegShape g, uint32_t *__restrict__ lens, uint32_t *__restrict__ totals)
{
    __shared__ uint32_t s[256];
    const int tid = threadIdx.x;
    uint32_t *base = lens + (size_t)blockIdx.x * g.ipp;
    uint32_t carry = 625;   // the header
    for (int c0 = 0; c0 < g.ipp; c0 += 256) {
        const uint32_t v = c0 + tid < g.ipp ? base[c0 + tid] : 0;
        s[tid] = v;
        __syncthreads();
        for (int d = 1; d < 256; d <<= 1) {
            const uint32_t add = tid >= d ? s[tid - d] : 0;
            __syncthreads();
            s[tid] += add;
            __syncthreads();
        }
        if (c0 + tid < g.ipp) base[c0 + tid] = carry + s[tid] - v;
        carry += s[255];
        __syncthreads();
    }
    if (tid == 0) totals[blockIdx.x] = carry;
}

__global__ __launch_bounds__(64) void jpeg_head_kernel(JpegHeader hdr, const mvhp_jpeg_entry_t *__restrict__ table,
                                                       uint8_t *__restrict__ blob, unsigned long long cap)
{
    const mvhp_jpeg_entry_t e = table[blockIdx.x];
    if (e.status != MVHP_JPEG_OK || e.offset > cap || e.length > cap - e.offset) return;
    uint8_t *out = blob + e.offset;
    for (uint32_t t = threadIdx.x; t < 625u && t < e.length; t += 64) out[t] = hdr.b[t];
    if (threadIdx.x < 2 && e.length >= 627u) out[e.length - 2 + threadIdx.x] = threadIdx.x ? 0xd9 : 0xff;
}

JpegShape shape_of(const JpegArgs &a)
{
    JpegShape g;
    g.w = a.w; g.h = a.h;
    g.mw = (a.w + 15) / 16;
    g.mcus = g.mw * ((a.h + 15) / 16);
    g.restart = a.restart;
    g.ipp = (g.mcus + a.restart - 1) / a.restart;
    g.n = a.n;
    return g;
}

} // namespace

void jpeg_quant_tables(int quality, uint8_t out[128])
{
    const int q = quality < 1 ? 1 : quality > 100 ? 100 : quality;
    const int scale = q < 50 ? 5000 / q : 200 - 2 * q;   // the IJG rule
    for (int t = 0; t < 2; t++)
        for (int i = 0; i < 64; i++) {
            const int v = (kBaseQ[t][i] * scale + 50) / 100;
            out[t * 64 + i] = (uint8_t)(v < 1 ? 1 : v > 255 ? 255 : v);
        }
}

void jpeg_header(int w, int h, int quality, int restart, uint8_t out[MVHP_JPEG_HEADER_BYTES])
{
    uint8_t q[128];
    jpeg_quant_tables(quality, q);
    uint8_t *p = out;
    auto bytes = [&](const void *src, size_t n) { memcpy(p, src, n); p += n; };
    auto b16 = [&](int v) { *p++ = (uint8_t)(v >> 8); *p++ = (uint8_t)v; };
    bytes("\xff\xd8", 2);
    bytes("\xff\xe0\x00\x10JFIF\x00\x01\x01\x00\x00\x01\x00\x01\x00\x00", 18);
    bytes("\xff\xdb\x00\x84", 4);
    for (int t = 0; t < 2; t++) {
        *p++ = (uint8_t)t;
        for (int k = 0; k < 64; k++) *p++ = q[t * 64 + kZigzag[k]];
    }
    bytes("\xff\xc0\x00\x11\x08", 5);
    b16(h);
    b16(w);
    bytes("\x03\x01\x22\x00\x02\x11\x01\x03\x11\x01", 10);
    for (int t = 0; t < 2; t++) {
        uint8_t dcvals[12];
        for (int i = 0; i < 12; i++) dcvals[i] = (uint8_t)i;
        bytes("\xff\xc4", 2); b16(2 + 1 + 16 + 12); *p++ = (uint8_t)t;
        bytes(kDcBits[t], 16); bytes(dcvals, 12);
        bytes("\xff\xc4", 2); b16(2 + 1 + 16 + 162); *p++ = (uint8_t)(0x10 | t);
        bytes(kAcBits[t], 16); bytes(kAcVals[t], 162);
    }
    bytes("\xff\xdd\x00\x04", 4);
    b16(restart);
    bytes("\xff\xda\x00\x0c\x03\x01\x00\x02\x11\x03\x11\x00\x3f\x00", 14);
}

size_t jpeg_scratch_bytes(const JpegArgs &a)
{
    const JpegShape g = shape_of(a);
    const size_t blocks = (size_t)a.n * g.mcus * 6;
    return blocks * 128 + blocks * 8 + (((size_t)a.n * g.ipp * 4 + 15) & ~(size_t)15) + (size_t)a.n * 4;
}

hipError_t launch_jpeg_encode(const JpegArgs &a, hipStream_t stream)
{
    const JpegShape g = shape_of(a);
    const size_t blocks = (size_t)a.n * g.mcus * 6;
    const size_t intervals = (size_t)a.n * g.ipp;
    int16_t *coefs = reinterpret_cast<int16_t *>(a.scratch);
    uint64_t *maps = reinterpret_cast<uint64_t *>(a.scratch + blocks * 128);
    uint32_t *lens = reinterpret_cast<uint32_t *>(a.scratch + blocks * 136);
    uint32_t *totals = reinterpret_cast<uint32_t *>(a.scratch + blocks * 136 + ((intervals * 4 + 15) & ~(size_t)15));
    JpegCodes codes;
    memset(&codes, 0, sizeof(codes));
    uint8_t dcvals[12];
    for (int i = 0; i < 12; i++) dcvals[i] = (uint8_t)i;
    for (int t = 0; t < 2; t++) {
        build_codes(kDcBits[t], dcvals, codes.dc[t]);
        build_codes(kAcBits[t], kAcVals[t], codes.ac[t]);
    }
    const unsigned huff_grid = (unsigned)((intervals + 63) / 64);
    if (a.stages & MVHP_JPEG_STAGE_DCT) {
        JpegQuant qt;
        jpeg_quant_tables(a.quality, &qt.q[0][0]);
        for (int k = 0; k < 64; k++) qt.zzpos[kZigzag[k]] = (uint8_t)k;
        jpeg_dct_kernel<<<dim3((unsigned)((blocks + kDctBlocks - 1) / kDctBlocks)), dim3(256), 0, stream>>>(
            a.yuv, g, qt, coefs, maps, (long long)blocks);
    }
    if (a.stages & MVHP_JPEG_STAGE_COUNT) {
        jpeg_huff_kernel<false><<<dim3(huff_grid), dim3(64), 0, stream>>>(g, codes, coefs, maps, lens, nullptr, nullptr, 0);
        jpeg_scan_kernel<<<dim3((unsigned)a.n), dim3(256), 0, stream>>>(g, lens, totals);
        blob_place_kernel<<<dim3(1), dim3(256), 0, stream>>>(a.n, totals, (unsigned long long)a.cap, a.table);
    }
    if (a.stages & MVHP_JPEG_STAGE_WRITE) {
        JpegHeader hdr;
        memset(&hdr, 0, sizeof(hdr));
        jpeg_header(a.w, a.h, a.quality, a.restart, hdr.b);
        jpeg_huff_kernel<true><<<dim3(huff_grid), dim3(64), 0, stream>>>(g, codes, coefs, maps, lens, a.table, a.blob, (unsigned long long)a.cap);
        jpeg_head_kernel<<<dim3((unsigned)a.n), dim3(64), 0, stream>>>(hdr, a.table, a.blob, (unsigned long long)a.cap);
    }
    return hipGetLastError();
}

} // namespace mvhp
