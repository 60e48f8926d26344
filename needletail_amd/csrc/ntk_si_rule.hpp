// The rule of the seed-index library (ntk_seed_index.hip, include_staged/needletail_amd/seed_index.h).  Plain C++ without any device
// call, so that it also compiles with g++: the CPU suite sweeps the search and the classification with it over every small key set and
// holds them to the definition (tests/test_si_rule.py), also under the sanitizers.
//
// The index holds its distinct values ascending (`keys`).  A seed's value is searched with si_find, the LOWER bound: the first key that
// is not below it, so a value is a key iff keys[si_find(...)] equals it.  A seed whose value is no key is ABSENT; one whose key has more
// than max_occ occurrences (max_occ != 0) is REPETITIVE - occ == max_occ is kept; every other seed is a HIT and makes one anchor per
// occurrence.  An occurrence is held as ref = r << 1 | strand; the anchor's ref_rev flips bit 0 by the seed's strand.  Anchors are
// ordered by (ref_rev, rpos, qpos): the 64-bit sort key is (ref_rev << 32) | rpos, and qpos decides between equal keys.
#pragma once

#include <stdint.h>

#if defined(__HIPCC__) || defined(__CUDACC__)
#define SI_FN __host__ __device__ inline
#else
#define SI_FN inline
#endif

// The geometry of the kernels: blocks of SI_THREADS; every kernel that loops does so with a grid of at most SI_BLOCKS_PER_CU blocks per
// compute unit.  A read with at most SI_SORT_TILE anchors is sorted by one block in LDS (12 B per anchor: 24 KiB); a longer one goes
// through the segmented radix sort.  The spectrum kernel keeps the bins below SI_SPECTRUM_LDS in LDS.  First choices, none measured.
constexpr uint32_t SI_THREADS = 256;
constexpr uint32_t SI_BLOCKS_PER_CU = 8;
constexpr uint32_t SI_SORT_TILE = 2048;
constexpr uint32_t SI_SPECTRUM_LDS = 1024;
static_assert((SI_SORT_TILE & (SI_SORT_TILE - 1)) == 0 && SI_SORT_TILE * 12 <= 64 * 1024, "a power of two of anchors that fits the LDS");

constexpr uint32_t SI_ABSENT = 0, SI_REPETITIVE = 1, SI_HIT = 2;
// what the verification of a list raises
constexpr uint32_t SI_BAD_OFFSETS = 1, SI_BAD_POS = 2;

// the first i in [0, n) with keys[i] >= v, n where there is none; keys ascending
SI_FN uint64_t si_find(const uint64_t *keys, uint64_t n, uint64_t v)
{
    uint64_t lo = 0, hi = n;
    while (lo < hi) {
        const uint64_t mid = lo + (hi - lo) / 2;
        if (keys[mid] < v) lo = mid + 1; else hi = mid;
    }
    return lo;
}

// the number of j in [0, n) with a[j] <= x, a non-decreasing: the record of entry x is one less
SI_FN uint64_t si_at_or_before(const uint64_t *a, uint64_t n, uint64_t x)
{
    uint64_t lo = 0, hi = n;
    while (lo < hi) {
        const uint64_t mid = lo + (hi - lo) / 2;
        if (a[mid] <= x) lo = mid + 1; else hi = mid;
    }
    return lo;
}

// a seed whose value is (present) or is not a key with `occ` occurrences, under max_occ (0: no limit)
SI_FN uint32_t si_classify(bool present, uint64_t occ, uint32_t max_occ)
{
    if (!present) return SI_ABSENT;
    return max_occ != 0 && occ > max_occ ? SI_REPETITIVE : SI_HIT;
}

SI_FN uint32_t si_ref(uint32_t record, uint32_t info) { return record << 1 | (info & 1u); }

// rev = the occurrence's strand flag xor the seed's
SI_FN uint32_t si_ref_rev(uint32_t ref, uint32_t qinfo) { return ref ^ (qinfo & 1u); }

SI_FN uint64_t si_sort_key(uint32_t ref_rev, uint32_t rpos)
{
    return (uint64_t)ref_rev << 32 | rpos;
}

// (key, qpos) of anchor a is in front of that of anchor b
SI_FN bool si_before(uint64_t key_a, uint32_t qpos_a, uint64_t key_b, uint32_t qpos_b)
{
    return key_a < key_b || (key_a == key_b && qpos_a < qpos_b);
}
