// The rule of the exact k-mer set algebra (ntk_kmer_sets.hip, include/needletail_amd_kmer_sets.h).  Plain constexpr C++ without any
// device call, so that it also compiles with g++: the CPU suite walks tiles with it exactly as the join kernel does and holds it to a
// set model on every pair of subsets of a small universe (tests/test_kset_rule.py), and a fault can be chased with gdb on a CPU build.
//
// The rule.  A and B are k-mer lists: strictly ascending keys of KW words each (a wide key is compared by hi, then lo), every key value
// legal, nothing padded.  The union is never built.  In the MERGED ORDER elements go by key, and on equal keys A's comes before B's.
// ks_split(d) is the number of A elements among the first d merged ones, one binary search on the diagonal.  Tile t covers the merged
// positions [tT, min((t + 1)T, n_a + n_b)): A[i0, i1) and B[j0, j1) from two splits.  A shared key may straddle a seam, its A element
// last in tile t and its B element first in tile t + 1; since each list ascends strictly the two are then adjacent, so a tile stages
// one look-behind element of A and one look-ahead element of B (KsView) and nothing further is ever needed:
//   an A element a: p = #{B[j0, j1) < a} (a lower bound), shared iff B[j0 + p] exists among the staged nb and equals a;
//   a B element b:  q = #{A[i0, i1) <= b} (an upper bound), shared iff the staged A element before it exists and equals b.
// Every key of the union is emitted once: by its A element if A has it, otherwise by its B element.  Inside the tile the element sits at
// merged slot x + p (A element x of the tile) or y + q (B element y); the emitting elements leave in the order of their slots.
// Every search runs on exactly the staged elements: on input that does not ascend the result is unspecified, but no index leaves the
// view and no slot leaves [0, T).
#pragma once

#include <stdint.h>

#if defined(__HIPCC__) || defined(__CUDACC__)
#define KS_HD __host__ __device__ inline constexpr
#else
#define KS_HD inline constexpr
#endif

// the values of include/needletail_amd_kmer_sets.h (the library asserts that they agree)
enum : uint32_t { KS_INTERSECT = 1, KS_UNION = 2, KS_SUBTRACT = 3, KS_COUNTERS_SUBTRACT = 4 };
enum : uint32_t { KS_MIN = 1, KS_MAX = 2, KS_SUM = 3, KS_LEFT = 4, KS_RIGHT = 5 };

template <int KW>
KS_HD bool ks_less(const uint64_t *x, const uint64_t *y)
{
    if (KW == 1) return x[0] < y[0];
    return x[0] < y[0] || (x[0] == y[0] && x[1] < y[1]);
}

template <int KW>
KS_HD bool ks_equal(const uint64_t *x, const uint64_t *y)
{
    if (KW == 1) return x[0] == y[0];
    return x[0] == y[0] && x[1] == y[1];
}

// the number of A elements among the first d merged elements, 0 <= d <= n_a + n_b
template <int KW>
KS_HD uint64_t ks_split(const uint64_t *a, uint64_t n_a, const uint64_t *b, uint64_t n_b, uint64_t d)
{
    uint64_t lo = d > n_b ? d - n_b : 0, hi = d < n_a ? d : n_a;
    while (lo < hi) {
        const uint64_t mid = lo + ((hi - lo) >> 1);           // mid < hi <= min(d, n_a)
        const uint64_t j = d - 1 - mid;                        // 0 <= j < n_b
        if (!ks_less<KW>(b + j * KW, a + mid * KW)) lo = mid + 1;   // a[mid] <= b[j]: a[mid] comes first, it is among the d
        else hi = mid;
    }
    return lo;
}

// the number of elements of v[0, n) below x
template <int KW>
KS_HD uint32_t ks_lower_bound(const uint64_t *v, uint32_t n, const uint64_t *x)
{
    uint32_t lo = 0, len = n;
    while (len) {
        const uint32_t half = len >> 1;
        if (ks_less<KW>(v + (uint64_t)(lo + half) * KW, x)) { lo += half + 1; len -= half + 1; }
        else len = half;
    }
    return lo;
}

// the number of elements of v[0, n) at or below x
template <int KW>
KS_HD uint32_t ks_upper_bound(const uint64_t *v, uint32_t n, const uint64_t *x)
{
    uint32_t lo = 0, len = n;
    while (len) {
        const uint32_t half = len >> 1;
        if (!ks_less<KW>(x, v + (uint64_t)(lo + half) * KW)) { lo += half + 1; len -= half + 1; }
        else len = half;
    }
    return lo;
}

// What tile t stages: A[sa0, sa0 + na) = the look-behind element (if any) and the tile's A part, B[j0, j0 + nb) = the tile's B part and
// the look-ahead element (if any).  The tile's own elements: the staged A elements from a_first on (la of them) and the first lb of B.
struct KsView {
    uint64_t i0, j0;      // the tile's first element of each list
    uint64_t sa0;         // the first staged element of A: i0 or i0 - 1
    uint32_t a_first;     // i0 - sa0
    uint32_t la, lb;      // the tile's own elements; la + lb <= T
    uint32_t na, nb;      // staged elements: a_first + la, and lb or lb + 1
};

// the view of the tile between the merged positions d0 <= d1 with the splits s0 = split(d0) and s1 = split(d1).  On lists that ascend
// s0 <= s1 and d0 - s0 <= d1 - s1; where unsorted input breaks that the tile is empty.
KS_HD KsView ks_view(uint64_t s0, uint64_t s1, uint64_t d0, uint64_t d1, uint64_t n_b)
{
    KsView v = {s0, d0 - s0, s0, 0, 0, 0, 0, 0};
    if (s1 < s0 || d1 - s1 < d0 - s0) return v;
    const uint64_t j1 = d1 - s1;
    v.la = (uint32_t)(s1 - s0); v.lb = (uint32_t)(j1 - v.j0);
    v.a_first = s0 > 0 ? 1 : 0;
    v.sa0 = s0 - v.a_first;
    v.na = v.a_first + v.la;
    v.nb = v.lb + (j1 < n_b ? 1 : 0);
    return v;
}

// where an element of the tile stands
struct KsHit {
    uint32_t slot;      // its merged position inside the tile, below la + lb
    uint32_t twin;      // the staged index of the other list's element with the same key (only where shared)
    bool shared;
};

// A element x (0 <= x < la) of the tile; sa and sb: the staged keys of the view
template <int KW>
KS_HD KsHit ks_probe_a(const KsView &v, const uint64_t *sa, const uint64_t *sb, uint32_t x)
{
    const uint64_t *key = sa + (uint64_t)(v.a_first + x) * KW;
    const uint32_t p = ks_lower_bound<KW>(sb, v.lb, key);   // p <= lb, and sb[p] is staged iff p < nb
    return KsHit{x + p, p, p < v.nb && ks_equal<KW>(sb + (uint64_t)p * KW, key)};
}

// B element y (0 <= y < lb) of the tile
template <int KW>
KS_HD KsHit ks_probe_b(const KsView &v, const uint64_t *sa, const uint64_t *sb, uint32_t y)
{
    const uint64_t *key = sb + (uint64_t)y * KW;
    const uint32_t q = v.a_first + ks_upper_bound<KW>(sa + (uint64_t)v.a_first * KW, v.la, key);   // staged A elements at or below b
    return KsHit{y + q - v.a_first, q - 1, q > 0 && ks_equal<KW>(sa + (uint64_t)(q - 1) * KW, key)};
}

KS_HD uint64_t ks_sat_add(uint64_t a, uint64_t b) { return a + b < a ? ~(uint64_t)0 : a + b; }

KS_HD uint64_t ks_rule(uint32_t rule, uint64_t a, uint64_t b)
{
    return rule == KS_MIN ? (a < b ? a : b) : rule == KS_MAX ? (a < b ? b : a) : rule == KS_SUM ? ks_sat_add(a, b) : rule == KS_LEFT ? a : b;
}

KS_HD bool ks_op_ok(uint32_t op, uint32_t rule)
{
    return (op == KS_INTERSECT || op == KS_UNION) ? (rule >= KS_MIN && rule <= KS_RIGHT)
                                                  : ((op == KS_SUBTRACT || op == KS_COUNTERS_SUBTRACT) && rule == 0);
}

// which counts an A element's output needs (its own, its twin's), so that no other count is read
KS_HD bool ks_a_needs_a(uint32_t op, bool shared) { return op == KS_INTERSECT ? shared : op == KS_SUBTRACT ? !shared : true; }
KS_HD bool ks_a_needs_b(uint32_t op, bool shared) { return shared && op != KS_SUBTRACT; }

// an A element's output: whether its key is kept, and with which count (ca, cb: the counts the two needs above asked for)
KS_HD bool ks_out_a(uint32_t op, uint32_t rule, bool shared, uint64_t ca, uint64_t cb, uint64_t &count)
{
    if (op == KS_INTERSECT) { count = ks_rule(rule, ca, cb); return shared; }
    if (op == KS_UNION) { count = shared ? ks_rule(rule, ca, cb) : ca; return true; }
    if (op == KS_SUBTRACT) { count = ca; return !shared; }
    const uint64_t b = shared ? cb : 0;   // KS_COUNTERS_SUBTRACT
    count = ca - b;
    return ca > b;
}

// a B element's output: only the union keeps a key that A lacks, with B's count
KS_HD bool ks_out_b(uint32_t op, bool shared) { return op == KS_UNION && !shared; }

KS_HD uint32_t ks_bin(uint64_t count, uint32_t n_bins) { return count < n_bins - 1 ? (uint32_t)count : n_bins - 1; }

// what compare adds up inside the kernel; the other seven totals follow from these and the two lengths (ks_totals)
struct KsSums {
    uint64_t n_shared = 0, sum_a = 0, sum_a_shared = 0, sum_b_shared = 0, sum_b_only = 0, sum_min = 0;
};
enum { KS_N_SUMS = 6 };

// an A element in compare: its joint bin, and its share of the sums (cb: the twin's count, 0 where there is none)
KS_HD uint32_t ks_compare_a(KsSums &s, bool shared, uint64_t ca, uint64_t cb, uint32_t n_bins_a, uint32_t n_bins_b)
{
    s.sum_a += ca;
    if (shared) {
        s.n_shared++;
        s.sum_a_shared += ca; s.sum_b_shared += cb;
        s.sum_min += ca < cb ? ca : cb;
    }
    return ks_bin(ca, n_bins_a) * n_bins_b + ks_bin(shared ? cb : 0, n_bins_b);
}

// a B element without a twin in compare (one with a twin was handled by it)
KS_HD uint32_t ks_compare_b(KsSums &s, uint64_t cb, uint32_t n_bins_b)
{
    s.sum_b_only += cb;
    return ks_bin(cb, n_bins_b);
}

// The thirteen totals, in the order of struct ntk_kmer_sets_totals.  Sums are modulo 2^64; max(a, b) = a + b - min(a, b) key by key, so
// sum_max = sum_a + sum_b - sum_min holds modulo 2^64 as well.
KS_HD void ks_totals(const uint64_t *s /* KS_N_SUMS words, in KsSums' order */, uint64_t n_a, uint64_t n_b, uint64_t *t)
{
    const uint64_t n_shared = s[0], sum_a = s[1], sum_a_shared = s[2], sum_b_shared = s[3], sum_b_only = s[4], sum_min = s[5];
    const uint64_t sum_b = sum_b_shared + sum_b_only;
    t[0] = n_a; t[1] = n_b; t[2] = n_shared; t[3] = n_a - n_shared; t[4] = n_b - n_shared;
    t[5] = sum_a; t[6] = sum_b; t[7] = sum_a_shared; t[8] = sum_b_shared;
    t[9] = sum_a - sum_a_shared; t[10] = sum_b_only;
    t[11] = sum_min; t[12] = sum_a + sum_b - sum_min;
}
