// The rule of the minimizer-list library (ntk_minimizer_list.hip, include/needletail_amd/minimizer_list.h).  Plain C++ without any device
// call, so that it also compiles with g++: the CPU suite runs the doubling argmin, the open-entry flag and the span rule with it over every
// small key array and holds them to a model written from the definition (tests/test_ml_rule.py), also under the sanitizers.
//
// Window ends are numbered along the batch.  End x has a key (its k-mer's value, or the hash of it) where the materialise face marks it
// valid.  The window that ends at x is the ends x - w + 1 .. x; it is WHOLE when all w of them are valid.  Its minimizer is the end with
// the smallest (key, end) pair: the smallest key, and of equal keys the leftmost.  A pair is unique, so the minimum over a range is the
// minimum over any two ranges that cover it: M_2q[x] = min(M_q[x - q], M_q[x]) doubles the range, and a window of any w is two
// overlapping ranges of the largest power of two Q <= w: min(M_Q[x - w + Q], M_Q[x]).  A range that holds an end that is not valid is
// BAD, and a window is whole iff its range is not bad.
//
// A whole window OPENS an entry unless the window one end before it is whole and picked the same end.  An entry's span is the number of
// consecutive windows it won: the windows after its first that are whole and open nothing, w at most.
#pragma once

#include <stdint.h>

#if defined(__HIPCC__) || defined(__CUDACC__)
#define ML_FN __host__ __device__ inline
#else
#define ML_FN inline
#endif
#define ML_HD ML_FN constexpr

// the values of include/needletail_amd/minimizer_list.h (the library asserts that they agree)
constexpr uint32_t ML_W_MAX = 256;
constexpr uint32_t ML_ORDER_LEX = 0, ML_ORDER_HASH = 1;
constexpr uint64_t ML_XOR = 0x9E3779B97F4A7C15ull;
// The geometry of ml_select_kernel and ml_scatter_kernel: a block of ML_THREADS takes ML_TILE window ends at a time, with w ends in
// front of them (ML_SLOTS = ML_TILE + ML_W_MAX slots of LDS at most); both kernels loop over the tiles with a grid of at most
// ML_BLOCKS_PER_CU blocks per compute unit.
constexpr uint32_t ML_THREADS = 256;
constexpr uint32_t ML_TILE = 1024;
constexpr uint32_t ML_SLOTS = ML_TILE + ML_W_MAX;
constexpr uint32_t ML_PER_THREAD = ML_SLOTS / ML_THREADS;
constexpr uint32_t ML_BLOCKS_PER_CU = 8;
static_assert(ML_SLOTS % ML_THREADS == 0, "a thread takes ML_PER_THREAD slots");
// a pair's second word: the slot in its low bits, ML_BAD above them
constexpr uint32_t ML_BAD = 0x8000, ML_SLOT = 0x7FFF;
static_assert(ML_SLOTS <= ML_SLOT, "a slot fits below the flag");
// a window end's word between the two kernels: bits 7:0 = the end minus the end it picked, then "whole" and "opens an entry"
constexpr uint32_t ML_SEL_WHOLE = 0x100, ML_SEL_OPEN = 0x200, ML_SEL_DELTA = 0xFF;
static_assert(ML_W_MAX - 1 <= ML_SEL_DELTA, "the distance to the picked end fits its bits");

// the murmur3 finaliser (fmix64 of ntk_consumer.hpp)
ML_HD uint64_t ml_fmix64(uint64_t x)
{
    x ^= x >> 33; x *= 0xff51afd7ed558ccdull;
    x ^= x >> 33; x *= 0xc4ceb9fe1a85ec53ull;
    x ^= x >> 33;
    return x;
}

// the key of a value under an order
ML_HD uint64_t ml_key(uint32_t order, uint64_t value) { return order == ML_ORDER_HASH ? ml_fmix64(value ^ ML_XOR) : value; }

// THE COMPARE, stated once: (key, position) pairs, so of equal keys the leftmost is the smaller
ML_HD bool ml_less(uint64_t key_a, uint32_t pos_a, uint64_t key_b, uint32_t pos_b) { return key_a < key_b || (key_a == key_b && pos_a < pos_b); }

struct MlPair {
    uint64_t key;
    uint32_t pos;   // slot | ML_BAD
};

// the pair of slot i of a staged tile: an end that is not valid makes every range it is in bad (its key is never the answer's)
ML_HD MlPair ml_pair(uint64_t key, uint32_t slot, bool valid) { return MlPair{valid ? key : 0, slot | (valid ? 0u : ML_BAD)}; }

// the minimum of two ranges' pairs; bad if either is
ML_HD MlPair ml_pair_min(MlPair a, MlPair b)
{
    const bool take_b = ml_less(b.key, b.pos & ML_SLOT, a.key, a.pos & ML_SLOT);
    return MlPair{take_b ? b.key : a.key, ((take_b ? b.pos : a.pos) & ML_SLOT) | ((a.pos | b.pos) & ML_BAD)};
}

// the largest power of two <= w (w >= 1)
ML_HD uint32_t ml_top_q(uint32_t w)
{
    uint32_t q = 1;
    while (2 * q <= w) q *= 2;
    return q;
}

// One doubling step at slot i: M_2q[i] from M_q, a callable slot -> MlPair.  Slots below q keep their pair (no window reads them).
template <class M>
ML_FN MlPair ml_double_at(const M &m, uint32_t i, uint32_t q)
{
    return i >= q ? ml_pair_min(m(i - q), m(i)) : m(i);
}

// The window that ends at slot i >= w - 1, from M_Q with Q = ml_top_q(w): two overlapping ranges.
template <class M>
ML_FN MlPair ml_window_at(const M &m, uint32_t i, uint32_t w, uint32_t q)
{
    return ml_pair_min(m(i - w + q), m(i));
}

ML_HD bool ml_whole(MlPair win) { return (win.pos & ML_BAD) == 0; }

// the open-entry flag of a window, from its own pair and that of the window one end before it
ML_HD bool ml_opens(MlPair before, MlPair win)
{
    return ml_whole(win) && !(ml_whole(before) && (before.pos & ML_SLOT) == (win.pos & ML_SLOT));
}

// a window end's word: slot i picked the slot of `win`
ML_HD uint32_t ml_sel_word(uint32_t i, MlPair before, MlPair win)
{
    return !ml_whole(win) ? 0u : ((i - (win.pos & ML_SLOT)) | ML_SEL_WHOLE | (ml_opens(before, win) ? ML_SEL_OPEN : 0u));
}

// the entry that opens at end x goes on through the end whose word is `word`
ML_HD bool ml_continues(uint32_t word) { return (word & (ML_SEL_WHOLE | ML_SEL_OPEN)) == ML_SEL_WHOLE; }

// The span of the entry that opens at end x: sel(x + j) is the word of a later end, and the ends from `limit` on have no window.
template <class Sel>
ML_FN uint32_t ml_span(const Sel &sel, uint64_t x, uint64_t limit, uint32_t w)
{
    uint32_t span = 1;
    while (span < w && x + span < limit && ml_continues(sel(x + span))) span++;
    return span;
}

// an entry's info word
ML_HD uint32_t ml_info(bool strand, uint32_t span) { return (span << 1) | (strand ? 1u : 0u); }
