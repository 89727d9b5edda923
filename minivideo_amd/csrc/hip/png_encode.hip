// png_encode.hip -- PNG files (8-bit RGB, row filters, Huffman-only deflate) from dense RGB8 pictures on the device (DESIGN.md 3
// "PNG output"; tests/png_ref.py states the same format in NumPy).  A picture is cut into segments of R rows; a segment is one
// IDAT chunk holding one deflate block that starts on a byte, so segments are coded independently and concatenated.
//
//   png_analyse_kernel   one workgroup per segment: a lane owns 16 filtered bytes of a row.  The five filters' sums choose the
//                        row's type (one byte per row into scratch); the histogram of the chosen filter's bytes (LDS, sixteen
//                        copies of the bins) and the segment's Adler-32 pair follow in a second walk over the same rows; then
//                        the code lengths (Huffman by (count, index), counts halved while a code passes 15 bits), dynamic
//                        against stored, and the chunk's length -- all from the histogram, nothing is coded here
//   png_scan_kernel      per picture: exclusive scan of the chunk lengths, the Adler-32 pairs combined, the file's length
//   blob_place_kernel    (blob_place.h) pictures in order at 16-byte-aligned offsets of the blob, {offset, length, status} each
//   png_write_kernel     one workgroup per segment: a lane filters its 16 bytes again with the known type and forms their codes;
//                        a workgroup prefix sum of the bit lengths gives every lane its bit offset; the strings are merged into
//                        a zeroed LDS tile with OR atomics; whole dwords of the tile leave as aligned stores (byte heads and
//                        tails), and the chunk's CRC-32 runs over the tile in pieces of 32 bytes, combined by x^(256 j)
//   png_head_kernel      signature, IHDR and IEND, built on the host and passed by value
// Nothing is shared between workgroups but the scratch buffer between launches; no waits inside a kernel.
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <string.h>

#include "blob_place.h"
#include "minivideo_hotpath.h"
#include "png_format.h"
#include "recon_kernels.h"

namespace mvhp {

namespace {

constexpr uint32_t kPoly = 0xedb88320u;   // CRC-32, reflected
constexpr uint32_t kAdler = 65521u;
constexpr int kDynHeaderBits = 17 + 19 * 3 + 257 * 4 + 4;
constexpr int kLensPitch = 272;           // bytes of scratch per segment's 257 code lengths
constexpr int kStageDwords = 2048 + 8;    // the write pass's tile: 256 lanes x 16 codes of 15 bits = 7680 bytes, the chunk's
                                          // first and last bytes (under 160), a carried dword and the destination's phase

// a(x) * b(x) mod the CRC polynomial, reflected (bit 31 = x^0); a != 0
constexpr __host__ __device__ uint32_t multmodp(uint32_t a, uint32_t b)
{
    uint32_t m = 1u << 31, p = 0;
    for (;;) {
        if (a & m) {
            p ^= b;
            if ((a & (m - 1)) == 0) break;
        }
        m >>= 1;
        b = (b & 1) ? (b >> 1) ^ kPoly : b >> 1;
    }
    return p;
}

struct PngTables {
    uint32_t crc[256];   // the byte-wise table
    uint32_t xp[256];    // x^(256 j): what 32 j bytes behind a piece do to its CRC
};

constexpr PngTables make_tables()
{
    PngTables t{};
    for (uint32_t i = 0; i < 256; i++) {
        uint32_t c = i;
        for (int k = 0; k < 8; k++) c = (c & 1) ? (c >> 1) ^ kPoly : c >> 1;
        t.crc[i] = c;
    }
    uint32_t p = 1u << 30;                                   // x^1
    for (int k = 0; k < 8; k++) p = multmodp(p, p);          // x^256
    t.xp[0] = 1u << 31;
    for (int j = 1; j < 256; j++) t.xp[j] = multmodp(t.xp[j - 1], p);
    return t;
}

constexpr PngTables kHostTables = make_tables();
__device__ const PngTables kTables = make_tables();

// kernel arguments passed by value (the launches keep no state on the device)
struct PngShape {
    int w, h;
    int R, S;             // rows per segment, segments per picture
    int row, frow;        // bytes of a row of samples (3 w) and of a filtered row (3 w + 1)
    int U;                // 16-byte units per filtered row
    int n;
};
struct PngSeg {           // scratch, one per segment
    uint32_t chunk;       // bytes of the IDAT chunk, framing included
    uint32_t a, b;        // Adler-32 pair of the segment's filtered bytes from (0, 0)
    uint32_t dynamic;     // 1: dynamic Huffman block, 0: stored
    uint32_t off;         // of the chunk inside the file (png_scan_kernel)
    uint32_t pad[3];
};
struct PngHead { uint8_t b[48]; };   // 33 bytes of signature + IHDR, 12 of IEND

// Samples of unit j of a row: X[i] / B[i] = sample byte 16 j - 4 + i of the row and of the row above (zero outside the row, and
// above row 0).  Filtered byte k of the unit (column 16 j + k of the filtered row, column 0 being the type) has x = X[k + 3],
// a = X[k], b = B[k + 3], c = B[k].
__device__ __forceinline__ void load_unit(const uint8_t *__restrict__ cur, const uint8_t *__restrict__ prev, int j, int row,
                                          uint32_t (&X)[19], uint32_t (&B)[19])
{
#pragma unroll
    for (int i = 0; i < 19; i++) {
        const int s = 16 * j - 4 + i;
        const bool in = (unsigned)s < (unsigned)row;
        X[i] = in ? cur[s] : 0u;
        B[i] = (in && prev) ? prev[s] : 0u;
    }
}

__device__ __forceinline__ uint32_t paeth(uint32_t a, uint32_t b, uint32_t c)
{
    const int pa = abs((int)b - (int)c), pb = abs((int)a - (int)c), pc = abs((int)a + (int)b - 2 * (int)c);
    return (pa <= pb && pa <= pc) ? a : (pb <= pc ? b : c);
}

__device__ __forceinline__ uint32_t filtered(int type, uint32_t x, uint32_t a, uint32_t b, uint32_t c)
{
    uint32_t p;
    switch (type) {
    case 0: p = 0; break;
    case 1: p = a; break;
    case 2: p = b; break;
    case 3: p = (a + b) >> 1; break;
    default: p = paeth(a, b, c); break;
    }
    return (x - p) & 255u;
}

__device__ __forceinline__ uint32_t cost_of(uint32_t f) { return f < 128u ? f : 256u - f; }

__device__ __forceinline__ unsigned long long wave_sum(unsigned long long v)
{
#pragma unroll
    for (int d = 32; d >= 1; d >>= 1) v += __shfl_down(v, d);
    return v;   // lane 0
}

__global__ __launch_bounds__(256) void png_analyse_kernel(PngShape g, const uint8_t *__restrict__ rgb, int pic0,
                                                          uint8_t *__restrict__ types, PngSeg *__restrict__ segs,
                                                          uint8_t *__restrict__ lens)
{
    __shared__ uint32_t s_hist[256][16];
    __shared__ uint32_t s_sum[256][5];
    __shared__ uint32_t s_type[256];
    __shared__ unsigned long long s_red[2][4];
    __shared__ uint32_t s_cnt[257];
    __shared__ uint16_t s_sorted[257];
    __shared__ uint32_t s_node[256];
    __shared__ uint16_t s_parent[513];
    __shared__ uint16_t s_depth[513];
    __shared__ uint32_t s_bits[4];
    const int tid = threadIdx.x;
    const int pic = pic0 + blockIdx.y, seg = blockIdx.x;
    const int y0 = seg * g.R, rows = min(g.R, g.h - y0);
    const uint32_t n_s = (uint32_t)rows * (uint32_t)g.frow;
    const uint8_t *img = rgb + (size_t)pic * g.h * g.row;
    for (int i = tid; i < 256 * 16; i += 256) (&s_hist[0][0])[i] = 0;
    unsigned long long sum_a = 0, sum_b = 0;
    for (int g0 = 0; g0 < rows; g0 += 256) {
        const int gr = min(256, rows - g0);
        for (int i = tid; i < gr * 5; i += 256) (&s_sum[0][0])[i] = 0;
        __syncthreads();
        for (int u = tid; u < gr * g.U; u += 256) {   // the five filters' sums
            const int lr = u / g.U, j = u - lr * g.U, y = y0 + g0 + lr;
            const uint8_t *cur = img + (size_t)y * g.row;
            uint32_t X[19], B[19];
            load_unit(cur, y ? cur - g.row : nullptr, j, g.row, X, B);
            uint32_t c0 = 0, c1 = 0, c2 = 0, c3 = 0, c4 = 0;
#pragma unroll
            for (int k = 0; k < 16; k++) {
                const int col = 16 * j + k;
                if (col >= 1 && col < g.frow) {
                    const uint32_t x = X[k + 3], a = X[k], b = B[k + 3], c = B[k];
                    c0 += cost_of(x);
                    c1 += cost_of((x - a) & 255u);
                    c2 += cost_of((x - b) & 255u);
                    c3 += cost_of((x - ((a + b) >> 1)) & 255u);
                    c4 += cost_of((x - paeth(a, b, c)) & 255u);
                }
            }
            atomicAdd(&s_sum[lr][0], c0);
            atomicAdd(&s_sum[lr][1], c1);
            atomicAdd(&s_sum[lr][2], c2);
            atomicAdd(&s_sum[lr][3], c3);
            atomicAdd(&s_sum[lr][4], c4);
        }
        __syncthreads();
        if (tid < gr) {
            int best = 0;
#pragma unroll
            for (int t = 1; t < 5; t++)
                if (s_sum[tid][t] < s_sum[tid][best]) best = t;   // (ties stay with the lower type)
            s_type[tid] = (uint32_t)best;
            types[(size_t)pic * g.h + y0 + g0 + tid] = (uint8_t)best;
        }
        __syncthreads();
        for (int u = tid; u < gr * g.U; u += 256) {   // histogram and Adler-32 sums of the chosen filter's bytes
            const int lr = u / g.U, j = u - lr * g.U, y = y0 + g0 + lr;
            const uint8_t *cur = img + (size_t)y * g.row;
            const int type = (int)s_type[lr];
            uint32_t X[19], B[19];
            load_unit(cur, y ? cur - g.row : nullptr, j, g.row, X, B);
            const uint32_t q0 = (uint32_t)(g0 + lr) * (uint32_t)g.frow + 16u * (uint32_t)j;   // of the unit in the segment
#pragma unroll
            for (int k = 0; k < 16; k++) {
                const int col = 16 * j + k;
                if (col < g.frow) {
                    const uint32_t f = col ? filtered(type, X[k + 3], X[k], B[k + 3], B[k]) : (uint32_t)type;
                    atomicAdd(&s_hist[f][tid & 15], 1u);
                    sum_a += f;
                    sum_b += (unsigned long long)(n_s - (q0 + k)) * f;
                }
            }
        }
        // (s_sum and s_type are next written behind the next round's first and second barrier: every lane has left this walk)
    }
    sum_a = wave_sum(sum_a);
    sum_b = wave_sum(sum_b);
    if ((tid & 63) == 0) { s_red[0][tid >> 6] = sum_a; s_red[1][tid >> 6] = sum_b; }
    __syncthreads();
    uint32_t mine = 0;   // count of literal `tid`
#pragma unroll
    for (int r = 0; r < 16; r++) mine += s_hist[tid][r];
    s_cnt[tid] = mine;
    if (tid == 0) s_cnt[256] = 1;   // end of block
    __syncthreads();
    const int leaves = __syncthreads_count(mine != 0) + 1;   // at least 2
    uint32_t len = 0, len_eob = 0;
    for (;;) {
        for (int sym = tid; sym < 257; sym += 256) {   // rank by (count, index)
            const uint32_t c = s_cnt[sym];
            if (c) {
                int rank = 0;
                for (int j = 0; j < 257; j++) {
                    const uint32_t cj = s_cnt[j];
                    rank += (cj != 0 && (cj < c || (cj == c && j < sym))) ? 1 : 0;
                }
                s_sorted[rank] = (uint16_t)sym;
            }
        }
        __syncthreads();
        if (tid == 0) {   // two queues: sorted leaves, and internal nodes in order of creation (their counts do not fall)
            int li = 0, ii = 0;
            for (int m = 0; m < leaves - 1; m++) {
                uint32_t total = 0;
                for (int t = 0; t < 2; t++) {
                    int node;
                    uint32_t c;
                    if (li < leaves && (ii >= m || s_cnt[s_sorted[li]] <= s_node[ii])) {   // a leaf wins a tie: lower index
                        node = s_sorted[li++];
                        c = s_cnt[node];
                    } else {
                        node = 257 + ii;
                        c = s_node[ii++];
                    }
                    s_parent[node] = (uint16_t)(257 + m);
                    total += c;
                }
                s_node[m] = total;
            }
            s_depth[257 + leaves - 2] = 0;
            for (int i = leaves - 3; i >= 0; i--) s_depth[257 + i] = (uint16_t)(s_depth[s_parent[257 + i]] + 1);
        }
        __syncthreads();
        len = s_cnt[tid] ? (uint32_t)s_depth[s_parent[tid]] + 1u : 0u;
        len_eob = (uint32_t)s_depth[s_parent[256]] + 1u;
        if (!__syncthreads_or(len > 15u || len_eob > 15u)) break;
        const uint32_t c = s_cnt[tid];
        __syncthreads();
        s_cnt[tid] = c ? (c + 1) >> 1 : 0;   // (end of block stays at 1)
        __syncthreads();
    }
    uint32_t bits = (uint32_t)wave_sum((unsigned long long)mine * len);
    if ((tid & 63) == 0) s_bits[tid >> 6] = bits;
    __syncthreads();
    const size_t si = (size_t)pic * g.S + seg;
    lens[si * kLensPitch + tid] = (uint8_t)len;
    if (tid == 0) {
        lens[si * kLensPitch + 256] = (uint8_t)len_eob;
        bits = s_bits[0] + s_bits[1] + s_bits[2] + s_bits[3] + len_eob + (uint32_t)kDynHeaderBits + 3u;
        const uint32_t dyn = ((bits + 7u) >> 3) + 4u, stored = 5u + n_s;
        PngSeg r;
        r.dynamic = dyn < stored ? 1u : 0u;
        r.chunk = 12u + (r.dynamic ? dyn : stored) + (seg == 0 ? 2u : 0u) + (seg == g.S - 1 ? 4u : 0u);
        r.a = (uint32_t)((s_red[0][0] + s_red[0][1] + s_red[0][2] + s_red[0][3]) % kAdler);
        r.b = (uint32_t)((s_red[1][0] % kAdler + s_red[1][1] % kAdler + s_red[1][2] % kAdler + s_red[1][3] % kAdler) % kAdler);
        r.off = 0;
        r.pad[0] = r.pad[1] = r.pad[2] = 0;
        segs[si] = r;
    }
}

__global__ __launch_bounds__(256) void png_scan_kernel(PngShape g, int pic0, PngSeg *__restrict__ segs,
                                                       uint32_t *__restrict__ totals, uint32_t *__restrict__ adlers)
{
    __shared__ uint32_t s[256];
    const int tid = threadIdx.x;
    const int pic = pic0 + blockIdx.x;
    PngSeg *base = segs + (size_t)pic * g.S;
    uint32_t carry = 33;   // signature + IHDR
    for (int c0 = 0; c0 < g.S; c0 += 256) {
        const uint32_t v = c0 + tid < g.S ? base[c0 + tid].chunk : 0;
        s[tid] = v;
        __syncthreads();
        for (int d = 1; d < 256; d <<= 1) {
            const uint32_t add = tid >= d ? s[tid - d] : 0;
            __syncthreads();
            s[tid] += add;
            __syncthreads();
        }
        if (c0 + tid < g.S) base[c0 + tid].off = carry + s[tid] - v;
        carry += s[255];
        __syncthreads();
    }
    if (tid == 0) {
        unsigned long long A = 1, B = 0;   // A += a_s; B += n_s * A_before + b_s
        for (int i = 0; i < g.S; i++) {
            const unsigned long long n_s = (unsigned long long)min(g.R, g.h - i * g.R) * (unsigned long long)g.frow;
            B = (B + (n_s % kAdler) * A + base[i].b) % kAdler;
            A = (A + base[i].a) % kAdler;
        }
        totals[pic] = carry + 12;   // IEND
        adlers[pic] = (uint32_t)((B << 16) | A);
    }
}

__device__ __forceinline__ void or_bits(uint32_t *stage, uint32_t bitpos, uint32_t v, int n)   // n <= 32 bits of v at bitpos
{
    const uint32_t dw = bitpos >> 5, sh = bitpos & 31u;
    atomicOr(&stage[dw], v << sh);
    if (sh + (uint32_t)n > 32u) atomicOr(&stage[dw + 1], v >> (32u - sh));
}

__global__ __launch_bounds__(256) void png_write_kernel(PngShape g, const uint8_t *__restrict__ rgb, int pic0,
                                                        const uint8_t *__restrict__ types, const PngSeg *__restrict__ segs,
                                                        const uint8_t *__restrict__ lens, const uint32_t *__restrict__ adlers,
                                                        const mvhp_jpeg_entry_t *__restrict__ table, uint8_t *__restrict__ blob,
                                                        unsigned long long cap)
{
    __shared__ uint32_t s_stage[kStageDwords];
    __shared__ uint32_t s_crc_t[256];
    __shared__ uint32_t s_code[257];     // (length << 16) | code, its first bit lowest
    __shared__ uint8_t s_len[260];
    __shared__ uint32_t s_blc[16], s_next[16];
    __shared__ uint32_t s_wave[4];
    __shared__ uint32_t s_crc;
    const int tid = threadIdx.x;
    const int pic = pic0 + blockIdx.y, seg = blockIdx.x;
    const mvhp_jpeg_entry_t e = table[pic];
    // (the table is checked against the capacity again: a write stage run on its own trusts no earlier launch)
    if (e.status != MVHP_PNG_OK || (e.offset & 15ull) || e.offset > cap || e.length > cap - e.offset) return;
    uint8_t *out = blob + e.offset;
    const uint32_t limit = e.length;     // nothing is stored at or beyond the file's length
    const size_t si = (size_t)pic * g.S + seg;
    const PngSeg rec = segs[si];
    const bool dynamic = rec.dynamic != 0, last = seg == g.S - 1;
    const int y0 = seg * g.R, rows = min(g.R, g.h - y0);
    const uint32_t n_s = (uint32_t)rows * (uint32_t)g.frow;
    const uint8_t *img = rgb + (size_t)pic * g.h * g.row;

    s_crc_t[tid] = kTables.crc[tid];
    for (int i = tid; i < kStageDwords; i += 256) s_stage[i] = 0;
    if (tid < 16) s_blc[tid] = 0;
    if (tid == 0) s_crc = 0xffffffffu;
    __syncthreads();
    if (dynamic) {   // canonical codes of the segment's lengths
        for (int sym = tid; sym < 257; sym += 256) {
            const uint32_t l = lens[si * kLensPitch + sym] & 15u;
            s_len[sym] = (uint8_t)l;
            if (l) atomicAdd(&s_blc[l], 1u);
        }
        __syncthreads();
        if (tid == 0) {
            uint32_t code = 0;
            s_next[0] = 0;
            for (int b = 1; b < 16; b++) {
                code = (code + (b > 1 ? s_blc[b - 1] : 0u)) << 1;
                s_next[b] = code;
            }
        }
        __syncthreads();
        for (int sym = tid; sym < 257; sym += 256) {
            const uint32_t l = s_len[sym];
            uint32_t rank = 0;
            for (int j = 0; j < sym; j++) rank += s_len[j] == l ? 1u : 0u;
            s_code[sym] = l ? (l << 16) | (__brev(s_next[l] + rank) >> (32u - l)) : 0u;
        }
    } else {
        s_code[tid] = (8u << 16) | (uint32_t)tid;
        if (tid == 0) s_code[256] = 0;
    }
    __syncthreads();

    // The tile holds the chunk's bytes from its type on (the length in front and the CRC behind are stored on their own), at the
    // phase of their destination: byte i of the tile goes to file position base + i, base a multiple of 4.
    const uint32_t p0 = rec.off + 4u, ph = p0 & 3u;
    uint32_t base = p0 - ph;             // file position of the tile's byte 0
    uint32_t bitpos = 8u * ph;           // where the next bit goes
    uint32_t fs = ph;                    // the tile's first byte that belongs to the chunk
    {   // the chunk's type, the zlib header, the block's header
        if (tid == 0) or_bits(s_stage, bitpos, 0x54414449u, 32);   // "IDAT"
        bitpos += 32;
        if (seg == 0) {
            if (tid == 0) or_bits(s_stage, bitpos, 0x0178u, 16);
            bitpos += 16;
        }
        if (dynamic) {
            if (tid == 0) {
                or_bits(s_stage, bitpos, 0x1e004u, 17);              // BFINAL 0, BTYPE 2, HLIT 0, HDIST 0, HCLEN 15
                or_bits(s_stage, bitpos + 17 + 9, 0x24924924u, 32);  // sixteen code-length-code lengths of 4 (16, 17, 18: 0),
                or_bits(s_stage, bitpos + 17 + 9 + 32, 0x9249u, 16); // three bits each
            }
            for (int sym = tid; sym < 257; sym += 256)               // the lengths, in the code-length code: four bits, symbol = code
                or_bits(s_stage, bitpos + 74 + 4 * sym, __brev((uint32_t)s_len[sym]) >> 28, 4);
            bitpos += kDynHeaderBits;                                // (the distance length: four zero bits)
        } else {
            if (tid == 0) {
                or_bits(s_stage, bitpos, last ? 1u : 0u, 8);
                or_bits(s_stage, bitpos + 8, (n_s & 0xffffu) | ((~n_s & 0xffffu) << 16), 32);
            }
            bitpos += 40;
        }
    }
    const int units = rows * g.U;
    for (int u0 = 0; u0 < units; u0 += 256) {
        const int u = u0 + tid;
        uint32_t fw[4] = {0, 0, 0, 0};   // this lane's filtered bytes
        int cnt = 0;
        uint32_t nbits = 0;
        if (u < units) {
            const int lr = u / g.U, j = u - lr * g.U, y = y0 + lr;
            const uint8_t *cur = img + (size_t)y * g.row;
            const int type = (int)types[(size_t)pic * g.h + y] & 7;
            uint32_t X[19], B[19];
            load_unit(cur, y ? cur - g.row : nullptr, j, g.row, X, B);
            cnt = min(16, g.frow - 16 * j);
#pragma unroll
            for (int k = 0; k < 16; k++) {
                if (k < cnt) {
                    const uint32_t f = (16 * j + k) ? filtered(type, X[k + 3], X[k], B[k + 3], B[k]) : (uint32_t)min(type, 4);
                    fw[k >> 2] |= f << (8 * (k & 3));
                    nbits += s_code[f] >> 16;
                }
            }
        }
        uint32_t incl = nbits;           // prefix sum of the bit lengths over the workgroup
#pragma unroll
        for (int d = 1; d < 64; d <<= 1) {
            const uint32_t t = __shfl_up(incl, d);
            if ((tid & 63) >= d) incl += t;
        }
        if ((tid & 63) == 63) s_wave[tid >> 6] = incl;
        __syncthreads();
        uint32_t before = 0, total = 0;
#pragma unroll
        for (int wv = 0; wv < 4; wv++) {
            if (wv < (tid >> 6)) before += s_wave[wv];
            total += s_wave[wv];
        }
        {   // merge this lane's string: whole dwords through a 64-bit accumulator
            uint32_t pos = bitpos + before + incl - nbits;
            uint32_t dw = pos >> 5;
            int nb = (int)(pos & 31u);
            unsigned long long acc = 0;
#pragma unroll
            for (int k = 0; k < 16; k++) {
                if (k < cnt) {
                    const uint32_t c = s_code[(fw[k >> 2] >> (8 * (k & 3))) & 255u];
                    acc |= (unsigned long long)(c & 0xffffu) << nb;
                    nb += (int)(c >> 16);
                    if (nb >= 32) {
                        atomicOr(&s_stage[dw++], (uint32_t)acc);
                        acc >>= 32;
                        nb -= 32;
                    }
                }
            }
            if (nb > 0 && acc) atomicOr(&s_stage[dw], (uint32_t)acc);
        }
        bitpos += total;
        const bool final = u0 + 256 >= units;
        if (final) {   // end of block, the empty stored block, the Adler-32
            if (dynamic) {
                const uint32_t c = s_code[256];
                if (tid == 0) {
                    or_bits(s_stage, bitpos, c & 0xffffu, (int)(c >> 16));
                    or_bits(s_stage, bitpos + (c >> 16), last ? 1u : 0u, 3);
                }
                bitpos = (bitpos + (c >> 16) + 3u + 7u) & ~7u;
                if (tid == 0) or_bits(s_stage, bitpos, 0xffff0000u, 32);
                bitpos += 32;
            }
            if (last) {
                if (tid == 0) or_bits(s_stage, bitpos, __builtin_bswap32(adlers[pic]), 32);
                bitpos += 32;
            }
        }
        __syncthreads();
        // flush: the tile's whole dwords (all of it at the end) leave for the file, and the CRC takes them in
        const uint32_t nd = final ? (bitpos + 31u) >> 5 : bitpos >> 5;
        const uint32_t fe = final ? bitpos >> 3 : nd * 4u;
        const uint8_t *stage8 = reinterpret_cast<const uint8_t *>(s_stage);
        const uint32_t crc_in = s_crc;
        uint32_t part = 0;
        if (fe > fs) {
            for (uint32_t i = tid; i < nd; i += 256) {
                const uint32_t lo = max(4u * i, fs), hi = min(4u * i + 4u, fe);
                const uint32_t fp = base + 4u * i;
                if (hi - lo == 4u && fp + 4u <= limit) {
                    *reinterpret_cast<uint32_t *>(out + fp) = s_stage[i];
                } else {
                    for (uint32_t b = lo; b < hi; b++)
                        if (base + b < limit) out[base + b] = stage8[b];
                }
            }
            // pieces of 32 bytes counted from the end; the state so far goes into the first four bytes
            const uint32_t L = fe - fs, pieces = (L + 31u) >> 5;
            if ((uint32_t)tid < pieces) {
                uint32_t c = 0;
                const int start = (int)fe - 32 * (tid + 1);
#pragma unroll 4
                for (int b = 0; b < 32; b++) {
                    const int idx = start + b;
                    if (idx >= (int)fs) {
                        uint32_t byte = stage8[idx];
                        const uint32_t rel = (uint32_t)idx - fs;
                        if (rel < 4u) byte ^= (crc_in >> (8u * rel)) & 255u;
                        c = s_crc_t[(c ^ byte) & 255u] ^ (c >> 8);
                    }
                }
                part = tid ? multmodp(kTables.xp[tid], c) : c;
            }
            if (L < 4u && tid == 0) part ^= crc_in >> (8u * L);
        } else if (tid == 0) {
            part = crc_in;
        }
#pragma unroll
        for (int d = 32; d >= 1; d >>= 1) part ^= __shfl_xor(part, d);
        const uint32_t keep = final ? 0u : s_stage[nd];   // the dword still being filled
        __syncthreads();
        if ((tid & 63) == 0) s_wave[tid >> 6] = part;
        for (uint32_t i = tid; i <= nd && i < (uint32_t)kStageDwords; i += 256) s_stage[i] = 0;
        __syncthreads();
        if (tid == 0) {
            s_crc = s_wave[0] ^ s_wave[1] ^ s_wave[2] ^ s_wave[3];
            s_stage[0] = keep;
        }
        base += nd * 4u;
        bitpos -= nd * 32u;
        if (nd) fs = 0;
        __syncthreads();
    }
    if (tid < 8) {   // the chunk's length in front, its CRC behind
        const uint32_t payload = rec.chunk - 12u;
        const uint32_t v = tid < 4 ? payload : s_crc ^ 0xffffffffu;
        const uint32_t fp = tid < 4 ? rec.off + tid : rec.off + 8u + payload + (tid - 4);
        if (fp < limit) out[fp] = (uint8_t)(v >> (8 * (3 - (tid & 3))));
    }
}

__global__ __launch_bounds__(64) void png_head_kernel(PngHead hd, int pic0, const mvhp_jpeg_entry_t *__restrict__ table,
                                                      uint8_t *__restrict__ blob, unsigned long long cap)
{
    const mvhp_jpeg_entry_t e = table[pic0 + blockIdx.x];
    if (e.status != MVHP_PNG_OK || (e.offset & 15ull) || e.offset > cap || e.length > cap - e.offset) return;
    uint8_t *out = blob + e.offset;
    const uint32_t t = threadIdx.x;
    if (t < 33u && t < e.length) out[t] = hd.b[t];
    if (t >= 33u && t < 45u && e.length >= 45u) out[e.length - 45u + t] = hd.b[t];
}

uint32_t host_crc(const uint8_t *p, size_t n)
{
    uint32_t c = 0xffffffffu;
    for (size_t i = 0; i < n; i++) c = kHostTables.crc[(c ^ p[i]) & 255u] ^ (c >> 8);
    return c ^ 0xffffffffu;
}

PngShape shape_of(const PngArgs &a)
{
    PngShape g;
    g.w = a.w; g.h = a.h;
    g.row = 3 * a.w; g.frow = 3 * a.w + 1;
    g.R = png_segment_rows(a.w);
    g.S = (a.h + g.R - 1) / g.R;
    g.U = (g.frow + 15) / 16;
    g.n = a.n;
    return g;
}

size_t align16(size_t v) { return (v + 15) & ~(size_t)15; }

} // namespace

void png_header(int w, int h, uint8_t out[MVHP_PNG_HEADER_BYTES])
{
    static const uint8_t sig[16] = {0x89, 'P', 'N', 'G', '\r', '\n', 0x1a, '\n', 0, 0, 0, 13, 'I', 'H', 'D', 'R'};
    memcpy(out, sig, 16);
    const uint32_t dims[2] = {(uint32_t)w, (uint32_t)h};
    for (int i = 0; i < 8; i++) out[16 + i] = (uint8_t)(dims[i >> 2] >> (8 * (3 - (i & 3))));
    out[24] = 8; out[25] = 2; out[26] = 0; out[27] = 0; out[28] = 0;
    const uint32_t c = host_crc(out + 12, 17);
    for (int i = 0; i < 4; i++) out[29 + i] = (uint8_t)(c >> (8 * (3 - i)));
}

size_t png_scratch_bytes(const PngArgs &a)
{
    const PngShape g = shape_of(a);
    const size_t segs = (size_t)a.n * g.S;
    return align16((size_t)a.n * a.h) + segs * sizeof(PngSeg) + segs * kLensPitch + 2 * align16((size_t)a.n * 4);
}

hipError_t launch_png_encode(const PngArgs &a, hipStream_t stream)
{
    const PngShape g = shape_of(a);
    const size_t segs_n = (size_t)a.n * g.S;
    uint8_t *types = a.scratch;
    PngSeg *segs = reinterpret_cast<PngSeg *>(a.scratch + align16((size_t)a.n * a.h));
    uint8_t *lens = reinterpret_cast<uint8_t *>(segs + segs_n);
    uint32_t *totals = reinterpret_cast<uint32_t *>(lens + segs_n * kLensPitch);
    uint32_t *adlers = reinterpret_cast<uint32_t *>(reinterpret_cast<uint8_t *>(totals) + align16((size_t)a.n * 4));
    PngHead hd;
    memset(&hd, 0, sizeof(hd));
    png_header(a.w, a.h, hd.b);
    static const uint8_t iend[12] = {0, 0, 0, 0, 'I', 'E', 'N', 'D', 0xae, 0x42, 0x60, 0x82};
    memcpy(hd.b + 33, iend, 12);
    if (a.stages & MVHP_PNG_STAGE_ANALYSE)
        for (int first = 0; first < a.n; first += 65535) {   // (grid y is at most 65535)
            const int n = a.n - first < 65535 ? a.n - first : 65535;
            png_analyse_kernel<<<dim3((unsigned)g.S, (unsigned)n), dim3(256), 0, stream>>>(g, a.rgb, first, types, segs, lens);
        }
    if (a.stages & MVHP_PNG_STAGE_PLACE) {
        png_scan_kernel<<<dim3((unsigned)a.n), dim3(256), 0, stream>>>(g, 0, segs, totals, adlers);
        blob_place_kernel<<<dim3(1), dim3(256), 0, stream>>>(a.n, totals, (unsigned long long)a.cap, a.table);
    }
    if (a.stages & MVHP_PNG_STAGE_WRITE) {
        for (int first = 0; first < a.n; first += 65535) {
            const int n = a.n - first < 65535 ? a.n - first : 65535;
            png_write_kernel<<<dim3((unsigned)g.S, (unsigned)n), dim3(256), 0, stream>>>(g, a.rgb, first, types, segs, lens, adlers,
                                                                                         a.table, a.blob, (unsigned long long)a.cap);
        }
        png_head_kernel<<<dim3((unsigned)a.n), dim3(64), 0, stream>>>(hd, 0, a.table, a.blob, (unsigned long long)a.cap);
    }
    return hipGetLastError();
}

} // namespace mvhp
