// blank_policy.h -- picture scores and the blank-picture policy of minivideo_decode (opt-in, MINIVIDEO_SKIP_BLANK=1; DESIGN.md 3
// "Picture scores").  Pure host arithmetic, no device, no floating point: the library compiles this text (mvhp_luma_score,
// mvhp_blank_choose, api.cpp) and so does a CPU test (tests/test_blank.py), as with resample_taps.h and deblock_edge.h.
#ifndef MVHP_BLANK_POLICY_H
#define MVHP_BLANK_POLICY_H

#include <stdint.h>

#include <string>
#include <vector>

namespace mvblank {

// floor(16 (N Q - S^2) / N^2): the variance of N samples with sum S and sum of squares Q, in sixteenths (0 .. 260100 for
// 8-bit samples: half 0, half 255).  N <= 2^28, S <= 255 N, Q <= 255^2 N: 16 N Q < 2^76, hence 128 bits.  N = 0 gives 0;
// a record whose sums cannot come from samples (S^2 > N Q) gives 0 as well.
inline uint32_t luma_score(uint64_t sum, uint64_t sumsq, uint32_t samples)
{
    if (samples == 0) return 0;
    typedef unsigned __int128 u128;
    const u128 nq = (u128)samples * sumsq, ss = (u128)sum * sum;
    if (ss >= nq) return 0;
    const u128 v = 16 * (nq - ss) / ((u128)samples * samples);
    return v > 0xffffffffu ? 0xffffffffu : (uint32_t)v;
}

// Over a slot's candidates in order (the primary first): the first whose score is at least min_score; if there is none, the
// largest score, the earliest on a tie.  n <= 0: -1.
inline int choose(const uint32_t *scores, int n, uint32_t min_score)
{
    if (!scores || n <= 0) return -1;
    int best = 0;
    for (int i = 0; i < n; i++) {
        if (scores[i] >= min_score) return i;
        if (scores[i] > scores[best]) best = i;
    }
    return best;
}

// The alternates of slot k of `slots` (the IDR indices of the delivered pictures, in slot order) in a stream of n_idr IDR
// pictures: the IDR indices strictly between this slot's picture and the next slot's picture -- for the last slot, up to the
// end of the stream -- in stream order, at most `a` of them.
inline std::vector<int> alternates(const std::vector<int> &slots, int n_idr, int a, int k)
{
    std::vector<int> out;
    if (k < 0 || k >= (int)slots.size()) return out;
    const int end = (k + 1 < (int)slots.size()) ? slots[(size_t)k + 1] : n_idr;
    for (int i = slots[(size_t)k] + 1; i < end && i < n_idr && (int)out.size() < a; i++) out.push_back(i);
    return out;
}

// A decimal integer lo .. hi and nothing else (no sign, no blanks, at most nine digits).
inline bool parse_int(const char *t, long lo, long hi, long *out)
{
    if (!t || !*t) return false;
    long v = 0;
    int digits = 0;
    for (; *t >= '0' && *t <= '9' && digits < 9; t++, digits++) v = v * 10 + (*t - '0');
    if (*t != '\0' || v < lo || v > hi) return false;
    *out = v;
    return true;
}

struct Settings {
    bool     on = false;
    uint32_t min_score = 16u * 256u;   // a picture is blank when its score is below 16 x MINIVIDEO_BLANK_VARIANCE
    int      alternates = 4;
};

// The three switches (include/minivideo.h), given as the values of the environment (NULL = not set).  false: a malformed
// value -- whether or not the feature is switched on, so that a typing error does not pass unseen -- and `why` says which.
inline bool settings_from(const char *skip, const char *variance, const char *alts, Settings &s, std::string &why)
{
    s = Settings();
    long v = 0;
    if (skip && *skip) {
        if (!parse_int(skip, 0, 1, &v)) {
            why = std::string("MINIVIDEO_SKIP_BLANK='") + skip + "' is not 0 or 1";
            return false;
        }
        s.on = v != 0;
    }
    if (variance && *variance) {
        if (!parse_int(variance, 0, 16256, &v)) {
            why = std::string("MINIVIDEO_BLANK_VARIANCE='") + variance + "' is not an integer between 0 and 16256";
            return false;
        }
        s.min_score = 16u * (uint32_t)v;
    }
    if (alts && *alts) {
        if (!parse_int(alts, 1, 16, &v)) {
            why = std::string("MINIVIDEO_BLANK_ALTERNATES='") + alts + "' is not an integer between 1 and 16";
            return false;
        }
        s.alternates = (int)v;
    }
    return true;
}

} // namespace mvblank

#endif
