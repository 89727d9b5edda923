// represent_policy.h -- representative pictures: the picture-score record of a plane histogram, the choice among a slot's
// candidates and the switches (opt-in, MINIVIDEO_REPRESENTATIVE=1; DESIGN.md 3 "Representative pictures").  Pure host arithmetic,
// no device, no floating point: the library compiles this text (mvhp_hist_stats, mvhp_represent_choose, api.cpp) and so does a
// CPU test (tests/test_represent.py), as with blank_policy.h.
#ifndef MVHP_REPRESENT_POLICY_H
#define MVHP_REPRESENT_POLICY_H

#include <stdint.h>
#include <string.h>

#include <string>

#include "blank_policy.h"
#include "minivideo_hotpath.h"

namespace mvrep {

constexpr int kBins = 768;   // y, cb and cr of mvhp_plane_hist_t, one after the other

inline const uint32_t *bins(const mvhp_plane_hist_t &h) { return h.y; }   // (y[256], cb[256], cr[256] are contiguous)

// The record mvhp_luma_stats_dev writes for the rectangle the histogram was counted over.
inline void hist_stats(const mvhp_plane_hist_t &h, mvhp_luma_stats_t &out)
{
    memset(&out, 0, sizeof(out));
    uint64_t n = 0;
    for (uint64_t v = 0; v < 256; v++) {
        out.sum += v * h.y[v];
        out.sumsq += v * v * h.y[v];
        n += h.y[v];
    }
    out.samples = (uint32_t)n;
}

// Over h[0..n): the candidates are the eligible entries (eligible == NULL: all) whose sizes equal those of the first eligible
// entry.  With k candidates and M[b] the sum of their counts in bin b: D_i = sum_b (k h_i[b] - M[b])^2, i.e. k^2 times the squared
// distance of candidate i to the candidates' mean histogram.  h <= 2^28 and k <= 17 (any k below 2^30 would do): |k h - M| <
// 17 * 2^28, a square below 2^66, D below 2^76 -- unsigned __int128.  The smallest D wins, the earliest on a tie; none: -1.
inline int choose(const mvhp_plane_hist_t *h, int n, const uint8_t *eligible)
{
    if (!h || n <= 0) return -1;
    int first = -1;
    for (int i = 0; i < n && first < 0; i++)
        if (!eligible || eligible[i]) first = i;
    if (first < 0) return -1;
    auto candidate = [&](int i) {
        return (!eligible || eligible[i]) && h[i].samples == h[first].samples && h[i].chroma_samples == h[first].chroma_samples;
    };
    typedef unsigned __int128 u128;
    uint64_t M[kBins] = {0};
    uint64_t k = 0;
    for (int i = first; i < n; i++) {
        if (!candidate(i)) continue;
        k++;
        for (int b = 0; b < kBins; b++) M[b] += bins(h[i])[b];
    }
    int best = -1;
    u128 best_d = 0;
    for (int i = first; i < n; i++) {
        if (!candidate(i)) continue;
        u128 d = 0;
        for (int b = 0; b < kBins; b++) {
            const uint64_t a = k * bins(h[i])[b], diff = a > M[b] ? a - M[b] : M[b] - a;
            d += (u128)diff * diff;
        }
        if (best < 0 || d < best_d) { best = i; best_d = d; }
    }
    return best;
}

struct Settings {
    bool on = false;
    int  alternates = 8;
};

// The two switches (include/minivideo.h), given as the values of the environment (NULL = not set).  false: a malformed value
// -- whether or not the feature is switched on -- and `why` says which.
inline bool settings_from(const char *on, const char *alts, Settings &s, std::string &why)
{
    s = Settings();
    long v = 0;
    if (on && *on) {
        if (!mvblank::parse_int(on, 0, 1, &v)) { why = std::string("MINIVIDEO_REPRESENTATIVE='") + on + "' is not 0 or 1"; return false; }
        s.on = v != 0;
    }
    if (alts && *alts) {
        if (!mvblank::parse_int(alts, 1, 16, &v)) {
            why = std::string("MINIVIDEO_REPRESENTATIVE_ALTERNATES='") + alts + "' is not an integer between 1 and 16";
            return false;
        }
        s.alternates = (int)v;
    }
    return true;
}

} // namespace mvrep

#endif
