// The rule of the mapping library (ntk_mapping.hip, include_pending/needletail_amd/mapping.h).  Plain C++ without any device call, so that
// it also compiles with g++: the CPU suite sweeps mp_lg8, the overlap predicate, mp_mapq and the rank key with it against the host model
// (tests/test_map_rule.py), also under the sanitizers.  Integer arithmetic only, carried in u64.
//
// Rank.  A read's chains by (score descending, chain index ascending): mp_rank_key, every bit of which is significant.  Overlap.  Chains i
// and j of one read overlap iff ol = min(qe_i, qe_j) - max(qs_i, qs_j) > 0 and ol * 1000 > mask_level_pm * min(qe_i - qs_i, qe_j - qs_j):
// on the query only.  Parent.  link[i] is the LOWEST-ranked chain of rank below i's that overlaps i; without one i is primary and its own
// parent, otherwise parent[i] = parent[link[i]].  Secondaries.  A non-primary chain is eligible iff score * 1000 >= pri_ratio_pm *
// score(parent), and kept iff eligible and fewer than best_n eligible chains of its read have a lower rank.  Mapping quality.  mp_mapq:
// minimap2 2.17's chain-only formula 40 * pen * (1 - sub / score) * ln score - 4.343 * ln(n_sub + 1) in integers, with
// mp_lg8(v) = floor(256 * log2 v).
#pragma once

#include <stdint.h>

#if defined(__HIPCC__) || defined(__CUDACC__)
#define MP_FN __host__ __device__ inline
#else
#define MP_FN inline
#endif

// The geometry of the kernels: blocks of MP_THREADS; every kernel that loops does so with a grid of at most MP_BLOCKS_PER_CU blocks per
// compute unit.  mp_parent_kernel gives every wave room in LDS for the intervals and parents of MP_LDS_CHAINS chains (12 B each: 6 KiB
// per wave); a read with more chains runs the same loop on global memory.  First choices, none measured.
constexpr uint32_t MP_THREADS = 256;
constexpr uint32_t MP_BLOCKS_PER_CU = 8;
constexpr uint32_t MP_LDS_CHAINS = 512;
static_assert(MP_LDS_CHAINS % 64 == 0 && MP_LDS_CHAINS * 12 * (MP_THREADS / 64) <= 64 * 1024, "whole strips of chains per wave that fit the LDS");

constexpr uint32_t MP_NONE = 0xFFFFFFFFu;                 // no link; no place among the reported chains
constexpr uint32_t MP_K_MAX = 255;
constexpr uint32_t MP_PM_MAX = 1000;                      // of mask_level_pm and pri_ratio_pm
constexpr uint32_t MP_BEST_N_MAX = 65535;
constexpr uint64_t MP_READ_CHAINS = (uint64_t)1 << 16;    // a read with this many chains or more is refused: the parent rule is quadratic per read
constexpr uint32_t MP_SCORE_MAX = 0x7FFFFFFFu;
constexpr uint32_t MP_ROW_WORDS = 16;
// the words of a row
constexpr uint32_t MP_QS = 0, MP_QE = 1, MP_RS = 2, MP_RE = 3, MP_REF_REV = 4, MP_SCORE = 5, MP_CNT = 6, MP_MLEN = 7, MP_BLEN = 8, MP_PARENT = 9,
                   MP_SUBSC = 10, MP_N_SUB = 11, MP_MAPQ = 12, MP_FLAGS = 13, MP_RANK = 14;
constexpr uint32_t MP_PRIMARY = 1, MP_SECONDARY = 2;      // the flags of a row
// what the verification of the arrays raises: the first five are NTK_ERR_BAD_ARG, the next three NTK_ERR_UNSUPPORTED; MP_MAYBE_BLEN asks
// for the exact sums of the chains (the bound k + (re - rs) + (qe - qs) does not fit a u32)
constexpr uint32_t MP_BAD_OFFSETS = 1, MP_NO_MEMBER = 2, MP_BAD_MEMBER = 4, MP_BAD_ORDER = 8, MP_BAD_SCORE = 16, MP_MANY_CHAINS = 32,
                   MP_LONG_END = 64, MP_LONG_BLEN = 128, MP_MAYBE_BLEN = 256;
constexpr uint32_t MP_BAD_ARG_FLAGS = MP_BAD_OFFSETS | MP_NO_MEMBER | MP_BAD_MEMBER | MP_BAD_ORDER | MP_BAD_SCORE;
constexpr uint32_t MP_UNSUPPORTED_FLAGS = MP_MANY_CHAINS | MP_LONG_END | MP_LONG_BLEN;

struct mp_rule_params {
    uint32_t k, mask_level_pm, pri_ratio_pm, best_n, min_chain_score;
};

// floor(log2(v)), v >= 1
MP_FN uint32_t mp_ilog2(uint32_t v)
{
    return 31u - (uint32_t)__builtin_clz(v);
}

// floor(256 * log2(v)), v >= 1: the exponent, then eight squarings of the mantissa m in [2^31, 2^32) give the eight fraction bits
MP_FN uint32_t mp_lg8(uint32_t v)
{
    const uint32_t e = mp_ilog2(v);
    uint64_t m = (uint64_t)v << (31 - e);
    uint32_t frac = 0;
    for (int i = 0; i < 8; i++) {
        m = (m * m) >> 31;
        frac <<= 1;
        if (m >> 32) { frac |= 1; m >>= 1; }
    }
    return e << 8 | frac;
}

// the steps of two consecutive members (rpos_j, qpos_j), (rpos_i, qpos_i) of a chain on strand rev, as ch_pair takes them
MP_FN void mp_step(uint32_t rev, uint32_t rpos_j, uint32_t qpos_j, uint32_t rpos_i, uint32_t qpos_i, int64_t &dr, int64_t &dq)
{
    dr = (int64_t)rpos_i - (int64_t)rpos_j;
    dq = rev ? (int64_t)qpos_j - (int64_t)qpos_i : (int64_t)qpos_i - (int64_t)qpos_j;
}

// what a step adds to mlen and to blen
MP_FN uint64_t mp_step_mlen(int64_t dr, int64_t dq, uint32_t k)
{
    const int64_t least = dr < dq ? dr : dq;
    return least < (int64_t)k ? (uint64_t)least : k;
}
MP_FN uint64_t mp_step_blen(int64_t dr, int64_t dq) { return (uint64_t)(dr > dq ? dr : dq); }

// the query intervals [qs_i, qe_i) and [qs_j, qe_j) overlap under a mask level in per mille
MP_FN bool mp_overlap(uint32_t qs_i, uint32_t qe_i, uint32_t qs_j, uint32_t qe_j, uint32_t mask_level_pm)
{
    const int64_t ol = (int64_t)(qe_i < qe_j ? qe_i : qe_j) - (int64_t)(qs_i > qs_j ? qs_i : qs_j);
    if (ol <= 0) return false;
    const uint64_t li = qe_i - qs_i, lj = qe_j - qs_j;
    return (uint64_t)ol * 1000 > (uint64_t)mask_level_pm * (li < lj ? li : lj);
}

// a non-primary chain of this score under a parent of that score may be a secondary
MP_FN bool mp_eligible(uint32_t score, uint32_t parent_score, uint32_t pri_ratio_pm)
{
    return (uint64_t)score * 1000 >= (uint64_t)pri_ratio_pm * parent_score;
}

// the mapping quality of a primary chain: 1 <= score < 2^31, cnt >= 1, subsc the largest score among its n_sub children or 0
MP_FN uint32_t mp_mapq(uint32_t score, uint32_t cnt, uint32_t subsc, uint32_t n_sub, uint32_t min_chain_score)
{
    const uint64_t by_score = score < 100 ? score : 100, by_cnt = 10 * (uint64_t)(cnt < 10 ? cnt : 10);
    const uint64_t pen = by_score < by_cnt ? by_score : by_cnt;
    const uint32_t sub = subsc > min_chain_score ? subsc : min_chain_score;
    const uint64_t d = score > sub ? score - sub : 0;
    const uint64_t t = (40 * pen * d * mp_lg8(score)) / score;     // below 2^56 before the division
    const int64_t raw = (int64_t)(((t * 45426) >> 16) / 25600);    // 45426 / 65536 for ln 2
    const int64_t q = raw - (int64_t)(((uint64_t)mp_lg8(n_sub + 1) * 771 + 32768) >> 16);
    return q < 0 ? 0 : q > 60 ? 60 : (uint32_t)q;
}

// the sort key that ranks a read's chains by (score descending, chain index ascending): 1 <= score < 2^31
MP_FN uint64_t mp_rank_key(uint32_t score, uint32_t c) { return (uint64_t)(MP_SCORE_MAX - score) << 32 | c; }

// the number of j in [0, n) with a[j] <= x: the read of chain x, and the chain of member x, is one less where the offsets a are
// non-decreasing.  Terminates and stays inside [0, n] on any array.
MP_FN uint64_t mp_at_or_before(const uint64_t *a, uint64_t n, uint64_t x)
{
    uint64_t lo = 0, hi = n;
    while (lo < hi) {
        const uint64_t mid = lo + (hi - lo) / 2;
        if (a[mid] <= x) lo = mid + 1; else hi = mid;
    }
    return lo;
}
