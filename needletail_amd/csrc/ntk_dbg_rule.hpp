// The rule of the compacted de Bruijn graph of a k-mer list (ntk_dbg.hip, include/needletail_amd_dbg.h).  Plain constexpr C++ without
// any device call, so that it also compiles with g++: the CPU suite walks the directory, the bucket search, the edge byte, the mate, the
// link and the ranking rounds with it exactly as the kernels do, element by element, and holds the result to a set model
// (tests/test_dbg_rule.py, tests/_dbg_model.py), and a fault can be chased with gdb on a CPU build.
//
// The rule.  Keys are canonical k-mers, k odd (no k-mer is its own reverse complement, so nothing below has a tie), A C G T = 0 1 2 3,
// the first base most significant, strictly ascending.  s = the string of key x.
//   HALF-EDGE (x, side, c): leads to the string t = u[1:] + c with u = s (side 0) or rc(s) (side 1); its target is y = canon(t).  Bit
//     4 side + c of x's EDGE BYTE is set iff y is in the list (y == x included).
//   MATE: (y, side', c') with side' = 1 iff t is y's canonical string, c' = the complement of u's first base.  Its target is x.
//   LINK: a half-edge whose bit is the only one of its nibble, with y != x, whose mate's bit is the only one of the mate's nibble.
//     next[2 i + side] = 2 j + side' for a link from key index i to key index j, DBG_NONE otherwise.  Links pair up and every
//     (k-mer, side) has at most one, so the link graph is a disjoint union of paths and cycles: the unitigs.
//   STATE d = 2 i + out: k-mer i about to be left through side `out`, which spells it forward (out 0) or reverse-complemented (out 1).
//     succ(d) = next[d] ^ 1 (entered through side', left through the other one).  Each unitig is two chains of states, one per direction.
//   RANKING: pointer doubling over the states carries (pointer, hops, smallest key index covered).  A state without a successor is a
//     terminal and points to itself.  After r rounds a pointer covers 2^r hops: ceil(log2 n) + 1 rounds settle every path and let every
//     state of a cycle see the cycle's smallest key index m.  A cycle is then cut in front of m (the states whose successor is m's
//     become terminals) and ranked again like a path.
//   SPELLING: a path starts at the end k-mer with the smaller key (the chain whose terminal is the larger end), a lone k-mer is forward,
//     a cycle starts at state 2 m.  Unitigs are numbered by ascending start key.
// Every search runs inside [0, n) and every index a step returns is below n (or DBG_NONE): on a list that does not ascend or holds keys
// that are not canonical the answer is unspecified, but nothing outside the arrays is touched, and since a link is kept only when the
// mate's recorded target is the k-mer itself, links pair up whatever the input: the structure is paths and cycles, always.
#pragma once

#include <stdint.h>

#if defined(__HIPCC__) || defined(__CUDACC__)
#define DBG_HD __host__ __device__ inline constexpr
#else
#define DBG_HD inline constexpr
#endif

constexpr uint32_t DBG_NONE = 0xFFFFFFFFu;
constexpr uint32_t DBG_K_MIN = 3, DBG_K_MAX = 31;
constexpr uint64_t DBG_N_MAX = 0x7FFFFFFFull;       // key indices, positions and states (2 n of them) fit 32 bits
constexpr uint32_t DBG_CYCLE_BIT = 0x80000000u;     // of a start k-mer's length word (dbg_resolve)
// the words the device adds up (dbg_totals makes the struct of the header from them)
enum : uint32_t { DBG_SUM_HIST = 0, DBG_SUM_SELF = 25, DBG_SUM_LINKS = 26, DBG_N_SUMS = 27 };
enum : uint32_t { DBG_N_TOTALS = 31 };

DBG_HD bool dbg_k_ok(uint32_t k) { return k >= DBG_K_MIN && k <= DBG_K_MAX && (k & 1); }
DBG_HD uint64_t dbg_mask(uint32_t k) { return ((uint64_t)1 << (2 * k)) - 1; }
DBG_HD uint32_t dbg_popc4(uint32_t nib) { return (uint32_t)(0x4332322132212110ull >> (4 * (nib & 15))) & 15; }
DBG_HD uint32_t dbg_only_bit(uint32_t nib) { return (nib >> 1) - (nib >> 3); }   // the index of a nibble's only bit

// the reverse complement of the k-mer value x (2 k bits)
DBG_HD uint64_t dbg_rc(uint64_t x, uint32_t k)
{
    x = ~x;
    x = ((x >> 2) & 0x3333333333333333ull) | ((x & 0x3333333333333333ull) << 2);
    x = ((x >> 4) & 0x0F0F0F0F0F0F0F0Full) | ((x & 0x0F0F0F0F0F0F0F0Full) << 4);
    x = ((x >> 8) & 0x00FF00FF00FF00FFull) | ((x & 0x00FF00FF00FF00FFull) << 8);
    x = ((x >> 16) & 0x0000FFFF0000FFFFull) | ((x & 0x0000FFFF0000FFFFull) << 16);
    x = (x >> 32) | (x << 32);
    return x >> (64 - 2 * k);
}

// t = u[1:] + c, and rc(t) from ru = rc(u)
DBG_HD uint64_t dbg_ext(uint64_t u, uint32_t k, uint32_t c) { return ((u << 2) & dbg_mask(k)) | c; }
DBG_HD uint64_t dbg_ext_rc(uint64_t ru, uint32_t k, uint32_t c) { return ((uint64_t)(c ^ 3) << (2 * k - 2)) | (ru >> 2); }

// ---- the prefix directory ----------------------------------------------------------------------------------------------------------
// b = min(2 k, ceil(log2 n)) bits; rdir has 2^b + 1 words and is kept REVERSED, so that filling the empty buckets is a forward running
// minimum: rdir[2^b - p] = the first index whose prefix is >= p, rdir[0] = n.

DBG_HD uint32_t dbg_dir_bits(uint32_t k, uint64_t n)
{
    uint32_t b = 0;
    while (((uint64_t)1 << b) < n) b++;
    return b < 2 * k ? b : 2 * k;
}

DBG_HD uint64_t dbg_dir_words(uint32_t k, uint64_t n) { return ((uint64_t)1 << dbg_dir_bits(k, n)) + 1; }
DBG_HD uint64_t dbg_prefix(uint64_t v, uint32_t k, uint32_t b) { return (v & dbg_mask(k)) >> (2 * k - b); }

// what key index i marks before the running minimum: the slot and whether it is the first key of its bucket
DBG_HD bool dbg_dir_mark(const uint64_t *keys, uint32_t k, uint32_t b, uint32_t i, uint64_t &slot)
{
    const uint64_t p = dbg_prefix(keys[i], k, b);
    slot = ((uint64_t)1 << b) - p;
    return i == 0 || dbg_prefix(keys[i - 1], k, b) != p;
}

// the first index of [lo, hi) whose key is >= v; hi if there is none
DBG_HD uint32_t dbg_lower(const uint64_t *keys, uint32_t lo, uint32_t hi, uint64_t v)
{
    while (lo < hi) {
        const uint32_t mid = lo + ((hi - lo) >> 1);
        if (keys[mid] < v) lo = mid + 1;
        else hi = mid;
    }
    return lo;
}

// the same over the whole list, through v's bucket
DBG_HD uint32_t dbg_lower_dir(const uint64_t *keys, uint32_t n, const uint32_t *rdir, uint32_t k, uint32_t b, uint64_t v)
{
    const uint64_t slot = ((uint64_t)1 << b) - dbg_prefix(v, k, b);   // 1 .. 2^b
    uint32_t lo = rdir[slot], hi = rdir[slot - 1];
    if (hi > n) hi = n;
    if (lo > hi) lo = hi;
    return dbg_lower(keys, lo, hi, v);
}

// ---- the edge byte -----------------------------------------------------------------------------------------------------------------

struct DbgAdj {
    uint32_t edges = 0;                       // the edge byte
    uint32_t tgt[2] = {DBG_NONE, DBG_NONE};   // per side: the target's key index where the nibble has exactly one bit
    uint32_t n_self = 0;                      // set bits whose target is the k-mer itself
};

// The eight half-edges of key index i.  Per side, the targets that are canonical as written are consecutive values t0 .. t0 + 3: one
// search finds the first key >= t0 and the (at most four) keys from there are compared.  The others are looked up as rc(t), one each.
DBG_HD DbgAdj dbg_adjacency(const uint64_t *keys, uint32_t n, const uint32_t *rdir, uint32_t k, uint32_t b, uint32_t i)
{
    DbgAdj a;
    const uint64_t x = keys[i] & dbg_mask(k), rx = dbg_rc(x, k);
    for (uint32_t side = 0; side < 2; side++) {
        const uint64_t u = side ? rx : x, ru = side ? x : rx;
        const uint64_t t0 = dbg_ext(u, k, 0);
        uint32_t nib = 0, written = 0, last = DBG_NONE;
        for (uint32_t c = 0; c < 4; c++)
            if ((t0 | c) < dbg_ext_rc(ru, k, c)) written |= 1u << c;
        if (written) {
            const uint32_t q = dbg_lower_dir(keys, n, rdir, k, b, t0);
            for (uint32_t j = 0; j < 4; j++) {
                if (q + j >= n) break;
                const uint64_t d = keys[q + j] - t0;
                if (d < 4 && ((written >> d) & 1)) {
                    nib |= 1u << d;
                    last = q + j;
                    a.n_self += q + j == i;
                }
            }
        }
        for (uint32_t c = 0; c < 4; c++) {
            if ((written >> c) & 1) continue;
            const uint64_t rt = dbg_ext_rc(ru, k, c);
            const uint32_t q = dbg_lower_dir(keys, n, rdir, k, b, rt);
            if (q < n && keys[q] == rt) {
                nib |= 1u << c;
                last = q;
                a.n_self += q == i;
            }
        }
        a.edges |= nib << (4 * side);
        a.tgt[side] = dbg_popc4(nib) == 1 ? last : DBG_NONE;
    }
    return a;
}

// the bin of the degree histogram: [popcount side 0][popcount side 1]
DBG_HD uint32_t dbg_deg_bin(uint32_t edges) { return dbg_popc4(edges & 15) * 5 + dbg_popc4(edges >> 4); }

// ---- the link ----------------------------------------------------------------------------------------------------------------------

// the mate (y, side2, c2) of the half-edge (x, side, c)
DBG_HD void dbg_mate(uint64_t x, uint32_t k, uint32_t side, uint32_t c, uint32_t &side2, uint32_t &c2)
{
    const uint64_t rx = dbg_rc(x, k), u = side ? rx : x, ru = side ? x : rx;
    side2 = dbg_ext(u, k, c) < dbg_ext_rc(ru, k, c) ? 1 : 0;
    c2 = 3 ^ (uint32_t)(u >> (2 * k - 2));
}

// next[2 i + side]
DBG_HD uint32_t dbg_link(const uint64_t *keys, const uint8_t *edges, const uint32_t *tgt, uint32_t n, uint32_t k, uint32_t i, uint32_t side)
{
    const uint32_t nib = ((uint32_t)edges[i] >> (4 * side)) & 15;
    if (dbg_popc4(nib) != 1) return DBG_NONE;
    const uint32_t j = tgt[2 * (uint64_t)i + side];
    if (j >= n || j == i) return DBG_NONE;
    uint32_t side2 = 0, c2 = 0;
    dbg_mate(keys[i] & dbg_mask(k), k, side, dbg_only_bit(nib), side2, c2);
    if (dbg_popc4(((uint32_t)edges[j] >> (4 * side2)) & 15) != 1) return DBG_NONE;
    if (tgt[2 * (uint64_t)j + side2] != i) return DBG_NONE;   // always true on a k-mer list: the mate's only bit is the mate
    return 2 * j + side2;
}

// ---- the ranking -------------------------------------------------------------------------------------------------------------------
// a state's word: the pointer in the low half, the hops to it in the high half

DBG_HD uint64_t dbg_pack(uint32_t ptr, uint32_t dist) { return ((uint64_t)dist << 32) | ptr; }
DBG_HD uint32_t dbg_ptr(uint64_t w) { return (uint32_t)w; }
DBG_HD uint32_t dbg_dist(uint64_t w) { return (uint32_t)(w >> 32); }

DBG_HD uint32_t dbg_rounds_max(uint64_t n)
{
    uint32_t b = 0;
    while (((uint64_t)1 << b) < n) b++;
    return b + 1;
}

DBG_HD void dbg_rank_init(const uint32_t *next, uint32_t d, uint64_t &pd, uint32_t &mn)
{
    const uint32_t nx = next[d];
    pd = nx == DBG_NONE ? dbg_pack(d, 0) : dbg_pack(nx ^ 1, 1);
    mn = d >> 1;
}

// one round for state d; true when its pointer moved
DBG_HD bool dbg_rank_round(const uint64_t *pd_in, const uint32_t *mn_in, uint64_t *pd_out, uint32_t *mn_out, uint32_t d)
{
    const uint64_t w = pd_in[d];
    const uint32_t p = dbg_ptr(w);
    const uint64_t q = pd_in[p];
    const uint32_t m = mn_in[d], mp = mn_in[p];
    pd_out[d] = dbg_pack(dbg_ptr(q), dbg_dist(w) + dbg_dist(q));
    mn_out[d] = mp < m ? mp : m;
    return dbg_ptr(q) != p;
}

// After the first pass: a state whose pointer is no terminal is on a cycle and mn[d] is the cycle's smallest key index.  It starts
// again, cut in front of that k-mer.  In place: a state reads its own words and `next` only.  True for a state on a cycle.
DBG_HD bool dbg_rank_cut(const uint32_t *next, uint64_t *pd, const uint32_t *mn, uint32_t d)
{
    if (next[dbg_ptr(pd[d])] == DBG_NONE) return false;
    const uint32_t s = next[d] ^ 1;   // a state on a cycle has a successor
    pd[d] = (s >> 1) == mn[d] ? dbg_pack(d, 0) : dbg_pack(s, 1);
    return true;
}

struct DbgPlace {
    uint32_t start = 0;     // key index of the unitig's first k-mer
    uint32_t pos_flip = 0;  // position << 1 | flipped
    uint32_t len = 0;       // at the start k-mer: the unitig's k-mers, DBG_CYCLE_BIT set for a cycle; 0 elsewhere
};

// where k-mer i stands, from the settled words of its two states
DBG_HD DbgPlace dbg_resolve(const uint32_t *next, const uint64_t *pd, const uint32_t *mn, uint32_t i)
{
    DbgPlace r;
    const uint64_t a = pd[2 * (uint64_t)i], b = pd[2 * (uint64_t)i + 1];
    const uint32_t t0 = dbg_ptr(a), t1 = dbg_ptr(b), d0 = dbg_dist(a), d1 = dbg_dist(b);
    uint32_t len = 0, flip = 0, pos = 0;
    if (next[t0] == DBG_NONE) {   // a path: the chain that ends at the larger end is the spelled one; the other one counts the position
        len = d0 + d1 + 1;
        flip = (t0 >> 1) >= (t1 >> 1) ? 0 : 1;
        pos = flip ? d0 : d1;
        r.start = (flip ? t0 : t1) >> 1;
    } else {                      // a cycle: the chain of state 2 m, whose terminal is the state in front of it, next[2 m + 1]
        const uint32_t m = mn[2 * (uint64_t)i];
        const uint32_t last = dbg_dist(pd[2 * (uint64_t)m]);
        flip = t0 == next[2 * (uint64_t)m + 1] ? 0 : 1;
        const uint32_t d = flip ? d1 : d0;
        pos = last >= d ? last - d : 0;
        len = (last + 1) | DBG_CYCLE_BIT;
        r.start = m;
    }
    r.pos_flip = (pos << 1) | flip;
    r.len = pos == 0 && r.start == i ? len : 0;
    return r;
}

// flags of a unitig row: bit 0 cycle, bits 8..11 the popcount of the nibble behind the first k-mer, bits 12..15 of the one past the last
DBG_HD uint64_t dbg_row_flags(bool cycle, uint32_t first_edges, uint32_t first_flip, uint32_t last_edges, uint32_t last_flip)
{
    const uint32_t behind = dbg_popc4(first_edges >> (4 * (1 - first_flip))), ahead = dbg_popc4(last_edges >> (4 * last_flip));
    return (uint64_t)(cycle ? 1 : 0) | ((uint64_t)behind << 8) | ((uint64_t)ahead << 12);
}

// ---- the spelling ------------------------------------------------------------------------------------------------------------------

// base j (0 = first) of the k-mer value v
DBG_HD uint8_t dbg_base(uint64_t v, uint32_t k, uint32_t j) { return (uint8_t)("ACGT"[(v >> (2 * (k - 1 - j))) & 3]); }

// The totals of the header (DBG_N_TOTALS words: n_half_edges, deg_hist[5][5], n_isolated, n_tips, n_branching, n_self, n_links) from the
// device's sums.
inline void dbg_totals(const uint64_t *sums, uint64_t *out)
{
    uint64_t half = 0, tips = 0, branching = 0;
    for (uint32_t a = 0; a < 5; a++)
        for (uint32_t b = 0; b < 5; b++) {
            const uint64_t c = sums[DBG_SUM_HIST + a * 5 + b];
            out[1 + a * 5 + b] = c;
            half += (a + b) * c;
            if ((a == 0) != (b == 0)) tips += c;
            if (a > 1 || b > 1) branching += c;
        }
    out[0] = half;
    out[26] = sums[DBG_SUM_HIST];
    out[27] = tips;
    out[28] = branching;
    out[29] = sums[DBG_SUM_SELF];
    out[30] = sums[DBG_SUM_LINKS];
}
