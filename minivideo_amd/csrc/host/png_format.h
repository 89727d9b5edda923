// png_format.h -- the sizes of the PNG encoder's file format (DESIGN.md 3 "PNG output") that host code needs without the device:
// the encoder's own launches (png_encode.hip) and the decode engine's blob (decode_engine.cpp) read them here.
#pragma once
#include <stddef.h>

namespace mvhp {

// rows per segment (= per IDAT chunk): about 32 KB of filtered bytes, at least one row; 0 for w < 1
inline int png_segment_rows(int w)
{
    if (w < 1) return 0;
    const int r = 32768 / (3 * w + 1);
    return r > 1 ? r : 1;
}

// the longest file of a w x h picture -- every segment stored: signature, IHDR and IEND (45), zlib header and Adler-32 (6), per
// segment a chunk's framing (12) and a stored block's header (5), the filtered bytes; 0 for sizes below 1
inline size_t png_max_bytes(int w, int h)
{
    if (w < 1 || h < 1) return 0;
    const int R = png_segment_rows(w);
    return 45 + 6 + (size_t)17 * (size_t)((h + R - 1) / R) + (size_t)h * (3 * (size_t)w + 1);
}

} // namespace mvhp
