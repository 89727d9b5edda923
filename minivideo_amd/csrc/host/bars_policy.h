// bars_policy.h -- black bars: the content rule, the union of the probes' boxes and the trim rule (opt-in, MINIVIDEO_TRIM=1;
// DESIGN.md 3 "Black bars").  Pure host arithmetic, no device, no floating point: the library compiles this text (mvhp_bars_need,
// mvhp_bars_union, mvhp_trim_rect, mvhp_output_geometry, api.cpp), as with blank_policy.h.
#ifndef MVHP_BARS_POLICY_H
#define MVHP_BARS_POLICY_H

#include <stdint.h>
#include <string.h>

#include <algorithm>
#include <string>

#include "blank_policy.h"
#include "minivideo_hotpath.h"

namespace mvbars {

// bright samples that make a row of `len` samples (a column of `len` rows) content
inline uint32_t need(uint32_t len) { return std::max<uint32_t>(1u, len >> 5); }

inline bool empty(const mvhp_luma_bars_t &b) { return b.w == 0 || b.h == 0; }

// The smallest box that holds every non-empty box; returns how many there were.  min and max: the order does not matter.
inline int unite(const mvhp_luma_bars_t *b, int n, mvhp_luma_bars_t &out)
{
    memset(&out, 0, sizeof(out));
    uint64_t x0 = 0, y0 = 0, x1 = 0, y1 = 0;
    int found = 0;
    for (int i = 0; b && i < n; i++) {
        if (empty(b[i])) continue;
        const uint64_t bx1 = (uint64_t)b[i].x + b[i].w, by1 = (uint64_t)b[i].y + b[i].h;
        if (!found) { x0 = b[i].x; y0 = b[i].y; x1 = bx1; y1 = by1; }
        else { x0 = std::min<uint64_t>(x0, b[i].x); y0 = std::min<uint64_t>(y0, b[i].y); x1 = std::max(x1, bx1); y1 = std::max(y1, by1); }
        found++;
    }
    if (found) { out.x = (uint32_t)x0; out.y = (uint32_t)y0; out.w = (uint32_t)(x1 - x0); out.h = (uint32_t)(y1 - y0); }
    return found;
}

// The trim rule (include/minivideo_hotpath.h, mvhp_trim_rect).  `out` may be `crop`.
inline int trim_rect(const mvhp_output_geometry_t &crop, const mvhp_luma_bars_t *u, mvhp_output_geometry_t &out)
{
    const uint64_t cx = crop.crop_x, cy = crop.crop_y, cw = crop.crop_w, ch = crop.crop_h;
    memset(&out, 0, sizeof(out));
    out.crop_x = (uint32_t)cx; out.crop_y = (uint32_t)cy;
    out.crop_w = out.out_w = (uint32_t)cw;
    out.crop_h = out.out_h = (uint32_t)ch;
    if (!u || empty(*u)) return 0;
    uint64_t x0 = std::max<uint64_t>(cx, u->x), x1 = std::min<uint64_t>(cx + cw, (uint64_t)u->x + u->w);
    uint64_t y0 = std::max<uint64_t>(cy, u->y), y1 = std::min<uint64_t>(cy + ch, (uint64_t)u->y + u->h);
    if (x1 <= x0 || y1 <= y0) return 0;
    x0 &= ~(uint64_t)1; y0 &= ~(uint64_t)1;               // (the crop is even: the result stays inside it)
    x1 = (x1 + 1) & ~(uint64_t)1; y1 = (y1 + 1) & ~(uint64_t)1;
    if (x1 - x0 < (cw + 1) / 2 || y1 - y0 < (ch + 1) / 2) return 0;   // more than half of a side gone: a dark scene, not a bar
    out.crop_x = (uint32_t)x0; out.crop_y = (uint32_t)y0;
    out.crop_w = out.out_w = (uint32_t)(x1 - x0);
    out.crop_h = out.out_h = (uint32_t)(y1 - y0);
    return 1;
}

struct Settings {
    bool on = false;
    int  level = MVHP_BARS_LEVEL_DEFAULT;
    int  probes = 8;
};

// The three switches (include/minivideo.h), given as the values of the environment (NULL = not set).  false: a malformed value
// -- whether or not the feature is switched on -- and `why` says which.
inline bool settings_from(const char *trim, const char *level, const char *probes, Settings &s, std::string &why)
{
    s = Settings();
    long v = 0;
    if (trim && *trim) {
        if (!mvblank::parse_int(trim, 0, 1, &v)) { why = std::string("MINIVIDEO_TRIM='") + trim + "' is not 0 or 1"; return false; }
        s.on = v != 0;
    }
    if (level && *level) {
        if (!mvblank::parse_int(level, 1, 254, &v)) { why = std::string("MINIVIDEO_TRIM_LEVEL='") + level + "' is not an integer between 1 and 254"; return false; }
        s.level = (int)v;
    }
    if (probes && *probes) {
        if (!mvblank::parse_int(probes, 1, 64, &v)) { why = std::string("MINIVIDEO_TRIM_PROBES='") + probes + "' is not an integer between 1 and 64"; return false; }
        s.probes = (int)v;
    }
    return true;
}

} // namespace mvbars

#endif
