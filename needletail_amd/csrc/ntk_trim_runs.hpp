// The run search of the read trimmer (ntk_trim.hip, include/needletail_amd_trim.h), as a monoid over bit strings.  Plain C++ without
// any device call, so that it also compiles with g++: the CPU suite holds it to the model on every short bit string at every bit
// offset (tests/test_trim_abi.py), and a fault can be chased with gdb on a CPU build.
//
// A record's windows are a bit range [lo, hi) of the solid plane: bit e % 64 of word e / 64 is the window that ends at batch byte e
// (1 = solid).  RtRuns summarises a bit string: its length, its leading and trailing run of ones, and its longest run with the
// position of that run's first bit (the leftmost of equals; 0, 0 when there is no one).  rt_combine(a, b) is the summary of a followed
// by b; it is associative, with RtRuns() as its identity, so the words of a record may be folded in any grouping that keeps their
// order: across the lanes of a group by shuffles, and across the rounds of a long record by a carry.
#pragma once

#include <stdint.h>

#if defined(__HIPCC__) || defined(__CUDACC__)
#define RT_HD __host__ __device__ inline
#else
#define RT_HD inline
#endif

struct RtRuns {
    uint64_t len = 0;        // bits summarised
    uint64_t lead = 0;       // ones at the start (== len: all ones)
    uint64_t trail = 0;      // ones at the end
    uint64_t best = 0;       // the longest run of ones ...
    uint64_t best_pos = 0;   // ... and the position of its first bit; the leftmost of equals
};

RT_HD int rt_ctz64(uint64_t x) { return x ? __builtin_ctzll(x) : 64; }

// the summary of the low n bits (n <= 64) of x, bit 0 first; the bits above n are ignored
RT_HD RtRuns rt_word_runs(uint64_t x, uint32_t n)
{
    RtRuns r;
    if (n == 0) return r;
    const uint64_t mask = n < 64 ? (((uint64_t)1 << n) - 1) : ~(uint64_t)0;
    x &= mask;
    r.len = n;
    if (x == mask) {
        r.lead = r.trail = r.best = n;
        return r;
    }
    r.lead = (uint64_t)rt_ctz64(~x);
    r.trail = (uint64_t)__builtin_clzll(~(x << (64 - n)));   // x != mask: a zero among the n bits ends the count
    uint32_t at = 0;                                         // one step per run of ones
    while (x) {
        const uint32_t skip = (uint32_t)__builtin_ctzll(x);
        x >>= skip;
        at += skip;
        const uint32_t run = (uint32_t)rt_ctz64(~x);         // < 64: bit n - 1 or a lower one is zero
        if (run > r.best) { r.best = run; r.best_pos = at; }
        x >>= run;
        at += run;
    }
    return r;
}

// a followed by b
RT_HD RtRuns rt_combine(const RtRuns &a, const RtRuns &b)
{
    RtRuns r;
    r.len = a.len + b.len;
    r.lead = a.lead == a.len ? a.len + b.lead : a.lead;
    r.trail = b.trail == b.len ? b.len + a.trail : b.trail;
    r.best = a.best;
    r.best_pos = a.best_pos;
    const uint64_t mid = a.trail + b.lead;   // the run across the seam starts no earlier than a's best and no later than b's
    if (mid > r.best) { r.best = mid; r.best_pos = a.len - a.trail; }
    if (b.best > r.best) { r.best = b.best; r.best_pos = a.len + b.best_pos; }
    return r;
}

// the part of plane word w (the bits 64 w .. 64 w + 63) that lies in the bit range [lo, hi), summarised; RtRuns() when they are apart
RT_HD RtRuns rt_plane_word_runs(uint64_t word, uint64_t w, uint64_t lo, uint64_t hi)
{
    const uint64_t first = w * 64 > lo ? w * 64 : lo, end = w * 64 + 64 < hi ? w * 64 + 64 : hi;
    if (first >= end) return RtRuns();
    return rt_word_runs(word >> (first - w * 64), (uint32_t)(end - first));
}

// The kept interval of a record whose windows have the summary r, in record bytes: window i (0-based, of the record's candidates)
// ends at record byte k - 1 + i, so the run of n windows from window p covers the bytes [p, p + n + k - 1).  prefix: the leading run
// (the read is cut at its first weak window); otherwise the longest run.  min_length 0 counts as k; a shorter interval is empty.
RT_HD void rt_interval(const RtRuns &r, bool prefix, uint32_t k, uint64_t min_length, uint64_t &start, uint64_t &length)
{
    const uint64_t p = prefix ? 0 : r.best_pos, n = prefix ? r.lead : r.best;
    start = 0;
    length = 0;
    if (n == 0) return;
    const uint64_t len = n + k - 1;
    if (len < (min_length ? min_length : k)) return;
    start = p;
    length = len;
}
