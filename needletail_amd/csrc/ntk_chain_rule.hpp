// The rule of the chain library (ntk_chain.hip, include_pending/needletail_amd/chain.h).  Plain C++ without any device call, so that it
// also compiles with g++: the CPU suite sweeps ch_ilog2, the gap cost and the pair predicate with it against the host model
// (tests/test_ch_rule.py), also under the sanitizers.  Integer arithmetic only.
//
// Pair.  Anchors j < i of one read with equal ref_rev (rev = ref_rev & 1): dr = rpos_i - rpos_j; dq = qpos_i - qpos_j where rev is 0 and
// qpos_j - qpos_i where rev is 1.  j may precede i iff 1 <= dr <= max_dist, 1 <= dq <= max_dist and dd = |dr - dq| <= bw.  Then
// gain = min(dr, dq, k) and gap = dd == 0 ? 0 : ((dd * k * 41) >> 12) + (ilog2(dd) >> 1): minimap2 2.17's 0.01 * span * dd + log2(dd) / 2
// in integers (41 / 4096 for 0.01).  Recurrence.  f[i] = max(k, max over j of f[j] + gain - gap) as i32, j over the at most h anchors
// directly in front of i in the read's order that have i's ref_rev; p[i] is the j that attains the maximum, the LARGEST such j, and
// none (CH_NONE) where no candidate exceeds k.  A candidate is compared as one word, ch_candidate: (score << 32) | j where the score
// exceeds k and 0 otherwise, so the largest word is the rule's choice, tie-break included.  Runs.  A run is a maximal range of a read's
// anchors with one ref_rev whose consecutive rpos differ by at most max_dist: no pair crosses a run, since the order is by rpos.
#pragma once

#include <stdint.h>

#if defined(__HIPCC__) || defined(__CUDACC__)
#define CH_FN __host__ __device__ inline
#else
#define CH_FN inline
#endif

// The geometry of the kernels: blocks of CH_THREADS; every kernel that loops does so with a grid of at most CH_BLOCKS_PER_CU blocks per
// compute unit.  ch_dp_kernel gives every wave a ring of the last CH_RING anchors' rpos, qpos and f in LDS (12 B each: 6 KiB per wave), so
// h is at most CH_RING.  First choices, none measured.
constexpr uint32_t CH_THREADS = 256;
constexpr uint32_t CH_BLOCKS_PER_CU = 8;
constexpr uint32_t CH_RING = 512;
constexpr uint32_t CH_H_MAX = CH_RING;
static_assert((CH_RING & (CH_RING - 1)) == 0 && CH_RING * 12 * (CH_THREADS / 64) <= 64 * 1024, "a power of two of anchors per wave that fits the LDS");

constexpr uint32_t CH_NONE = 0xFFFFFFFFu;             // p of an anchor without a predecessor
constexpr uint32_t CH_K_MAX = 255;
constexpr uint32_t CH_MAX_DIST_MAX = 0x7FFFFFFFu;
constexpr uint64_t CH_READ_ANCHORS = (uint64_t)1 << 23;   // a read with this many anchors or more is refused: with k <= 255 a score stays below 2^31
// what the verification of the anchor arrays raises
constexpr uint32_t CH_BAD_OFFSETS = 1, CH_BAD_ORDER = 2, CH_LONG_READ = 4;

struct ch_rule_params {
    uint32_t k, max_dist, bw, h;
};

// floor(log2(v)), v >= 1
CH_FN uint32_t ch_ilog2(uint32_t v)
{
    return 31u - (uint32_t)__builtin_clz(v);
}

// the cost of a diagonal difference dd <= 2^31 - 1 under seed length k <= 255: below 2^34
CH_FN uint64_t ch_gap(uint32_t dd, uint32_t k)
{
    return dd == 0 ? 0 : (((uint64_t)dd * k * 41) >> 12) + (ch_ilog2(dd) >> 1);
}

// anchor j = (rpos_j, qpos_j) may precede anchor i = (rpos_i, qpos_i) on strand rev; if it may, what the step gains and costs
CH_FN bool ch_pair(uint32_t rev, uint32_t rpos_j, uint32_t qpos_j, uint32_t rpos_i, uint32_t qpos_i, const ch_rule_params &r, uint32_t &gain,
                   uint64_t &gap)
{
    const int64_t dr = (int64_t)rpos_i - (int64_t)rpos_j;
    const int64_t dq = rev ? (int64_t)qpos_j - (int64_t)qpos_i : (int64_t)qpos_i - (int64_t)qpos_j;
    if (dr < 1 || dr > (int64_t)r.max_dist || dq < 1 || dq > (int64_t)r.max_dist) return false;
    const int64_t dd = dr > dq ? dr - dq : dq - dr;
    if (dd > (int64_t)r.bw) return false;
    const int64_t least = dr < dq ? dr : dq;
    gain = least < (int64_t)r.k ? (uint32_t)least : r.k;
    gap = ch_gap((uint32_t)dd, r.k);
    return true;
}

// What predecessor j with score f_j offers anchor i, as the one word the maximum is taken of: 0 where j may not precede i or offers no
// more than k.  f_j < 2^31, so the score fits the upper word.
CH_FN uint64_t ch_candidate(uint32_t rev, uint32_t rpos_j, uint32_t qpos_j, int32_t f_j, uint32_t j, uint32_t rpos_i, uint32_t qpos_i,
                            const ch_rule_params &r)
{
    uint32_t gain = 0;
    uint64_t gap = 0;
    if (!ch_pair(rev, rpos_j, qpos_j, rpos_i, qpos_i, r, gain, gap)) return 0;
    const int64_t score = (int64_t)f_j + gain - (int64_t)gap;
    return score > (int64_t)r.k ? (uint64_t)score << 32 | j : 0;
}

// f and p of an anchor from the largest candidate word
CH_FN int32_t ch_f_of(uint64_t best, uint32_t k) { return best ? (int32_t)(best >> 32) : (int32_t)k; }
CH_FN uint32_t ch_p_of(uint64_t best) { return best ? (uint32_t)best : CH_NONE; }

// anchor i starts a run: the first of its read, another ref_rev than the anchor in front of it, or an rpos more than max_dist behind it
CH_FN bool ch_run_head(bool first_of_read, uint32_t ref_rev_prev, uint32_t rpos_prev, uint32_t ref_rev, uint32_t rpos, uint32_t max_dist)
{
    return first_of_read || ref_rev != ref_rev_prev || (uint64_t)rpos - rpos_prev > max_dist;
}

// the triple of anchor a is strictly in front of that of anchor b
CH_FN bool ch_before(uint32_t ref_rev_a, uint32_t rpos_a, uint32_t qpos_a, uint32_t ref_rev_b, uint32_t rpos_b, uint32_t qpos_b)
{
    if (ref_rev_a != ref_rev_b) return ref_rev_a < ref_rev_b;
    if (rpos_a != rpos_b) return rpos_a < rpos_b;
    return qpos_a < qpos_b;
}

// the number of j in [0, n) with a[j] <= x: the read of anchor x is one less where the offsets a are non-decreasing.  Terminates and stays
// inside [0, n] on any array.
CH_FN uint64_t ch_at_or_before(const uint64_t *a, uint64_t n, uint64_t x)
{
    uint64_t lo = 0, hi = n;
    while (lo < hi) {
        const uint64_t mid = lo + (hi - lo) / 2;
        if (a[mid] <= x) lo = mid + 1; else hi = mid;
    }
    return lo;
}

// the sort key that visits a read's anchors in order of (f descending, index ascending): 0 <= f < 2^31
CH_FN uint64_t ch_visit_key(int32_t f, uint32_t i) { return (uint64_t)(0x7FFFFFFFu - (uint32_t)f) << 32 | i; }
