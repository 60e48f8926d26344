// The per-lane logic of the all-pairs MinHash comparison (ntk_minhash_set.hip, include/needletail_amd_minhash_set.h).  Plain C++ without
// any device call, so that it also compiles with g++: the CPU suite walks it in rounds of 64 with an emulated ballot and holds it to the
// model on every pair of subsets of a small universe (tests/test_mhset_rank.py), and a fault can be chased with gdb on a CPU build.
//
// The rule.  A and B are strictly ascending, already cut at max_hash.  The union is never built: for element a_i of A let p be the number
// of B's elements below a_i (a lower bound), shared whether B[p] == a_i, and s the number of shared elements among A[0..i).  Then a_i is
// member i + p - s (0-based) of the ascending union, and it counts iff num == 0 or that position is below num.  The positions rise with
// i, so once one is at or past num every later one is too.  No load is ever padded: a lower bound runs on exactly n elements and B[p] is
// read only where p < n, so no hash value, 0 and 2^64 - 1 included, can be taken for anything else.
#pragma once

#include <stdint.h>

#if defined(__HIPCC__) || defined(__CUDACC__)
#define MS_HD __host__ __device__ inline
#else
#define MS_HD inline
#endif

// the number of elements of b[0..n) below x
MS_HD uint32_t ms_lower_bound(const uint64_t *b, uint32_t n, uint64_t x)
{
    uint32_t lo = 0, len = n;
    while (len) {
        const uint32_t half = len >> 1;
        if (b[lo + half] < x) { lo += half + 1; len -= half + 1; }
        else len = half;
    }
    return lo;
}

// the number of elements of h[0..n) at or below max_hash: a sketch's length after the cut
MS_HD uint64_t ms_cut_length(const uint64_t *h, uint64_t n, uint64_t max_hash)
{
    uint64_t lo = 0, len = n;
    while (len) {
        const uint64_t half = len >> 1;
        if (h[lo + half] <= max_hash) { lo += half + 1; len -= half + 1; }
        else len = half;
    }
    return lo;
}

struct MsHit {
    uint32_t p;      // elements of B below x; nb when x is above all of them
    bool shared;     // B holds x (at p)
};

MS_HD MsHit ms_probe(const uint64_t *b, uint32_t nb, uint64_t x)
{
    MsHit h;
    h.p = ms_lower_bound(b, nb, x);
    h.shared = h.p < nb && b[h.p] == x;
    return h;
}

// the shared flags of the lanes below `lane` in a round's ballot
MS_HD uint32_t ms_lanes_below(uint64_t ballot, uint32_t lane)
{
    return (uint32_t)__builtin_popcountll(ballot & (((uint64_t)1 << lane) - 1));
}

// the 0-based position of a_i in the ascending union; s: shared elements among A[0..i)
MS_HD uint64_t ms_union_position(uint64_t i, uint32_t p, uint64_t s) { return i + p - s; }

MS_HD bool ms_counted(uint64_t position, uint64_t num) { return num == 0 || position < num; }

// With one side of at least num elements the union has at least num members, so n_union is num whatever is shared, and a walk may end at
// the first position at or past num.  Otherwise the walk goes to A's end: the number of ALL shared elements decides n_union.
MS_HD bool ms_union_is_num(uint64_t num, uint64_t na, uint64_t nb) { return num != 0 && (na >= num || nb >= num); }

// n_union from S, the number of all shared elements, counted or not
MS_HD uint64_t ms_union(uint64_t num, uint64_t na, uint64_t nb, uint64_t S)
{
    const uint64_t all = na + nb - S;
    return num == 0 || all < num ? all : num;
}

// what a lane adds up over its rounds
struct MsLane {
    uint32_t n_shared = 0;   // counted shared elements
    double dot = 0.0;        // ca * cb over them
    double norm2 = 0.0;      // ca^2 over the counted elements of A
};

// One lane's step of one round: `live` lanes hold element i of A with the probe `hit`; `ballot` has the shared flags of the round's live
// lanes, `carry` the shared elements of the rounds before.  Returns the element's position in the union (meaningless on a dead lane).
MS_HD uint64_t ms_lane_step(MsLane &acc, bool live, uint64_t i, MsHit hit, uint64_t ballot, uint32_t lane, uint64_t carry, uint64_t num,
                            double ca, double cb)
{
    const uint64_t position = ms_union_position(i, hit.p, carry + ms_lanes_below(ballot, lane));
    if (live && ms_counted(position, num)) {
        acc.norm2 += ca * ca;
        if (hit.shared) {
            acc.n_shared++;
            acc.dot += ca * cb;
        }
    }
    return position;
}
