// blob_place.h -- where the files of one encoder call lie in the caller's blob (jpeg_encode.hip, png_encode.hip).
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "minivideo_hotpath.h"

namespace mvhp {
namespace {

// One workgroup: pictures in order at 16-byte-aligned offsets of the blob, {offset, length, status} each; a picture that does not
// fit gets length 0 and takes no room.
__global__ __launch_bounds__(256) void blob_place_kernel(int n, const uint32_t *__restrict__ totals, unsigned long long cap,
                                                         mvhp_jpeg_entry_t *__restrict__ table)
{
    __shared__ uint32_t s_len[1024];
    __shared__ unsigned long long s_off[1024];
    __shared__ unsigned long long s_pos;
    const int tid = threadIdx.x;
    if (tid == 0) s_pos = 0;
    for (int c0 = 0; c0 < n; c0 += 1024) {
        const int cn = min(1024, n - c0);
        for (int i = tid; i < cn; i += 256) s_len[i] = totals[c0 + i];
        __syncthreads();
        if (tid == 0) {
            unsigned long long pos = s_pos;
            for (int i = 0; i < cn; i++) {
                const uint32_t len = s_len[i];
                s_off[i] = pos;
                if (pos + len <= cap) pos = (pos + len + 15ull) & ~15ull;
                else s_len[i] = 0;   // too big: no room taken
            }
            s_pos = pos;
        }
        __syncthreads();
        for (int i = tid; i < cn; i += 256) {
            mvhp_jpeg_entry_t e;
            e.offset = s_off[i];
            e.length = s_len[i];
            e.status = s_len[i] ? MVHP_JPEG_OK : MVHP_JPEG_TOO_BIG;
            table[c0 + i] = e;
        }
        __syncthreads();
    }
}

} // namespace
} // namespace mvhp
