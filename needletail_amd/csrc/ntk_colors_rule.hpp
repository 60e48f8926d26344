// The rule of the coloured k-mer index (ntk_colors.hip, include/needletail_amd_colors.h).  Plain C++ without any device call, so that it
// also compiles with g++: the CPU suite runs insert-or-OR, lookup, the per-record accumulation and the best / second pass with it over
// heap arrays of the library's sizes and holds them to a dict model (tests/test_colors_rule.py), also under the sanitizers, and a fault
// can be chased with gdb on a CPU build.
//
// The index.  keys[slots] and masks[slots]; slots = the smallest power of two (>= 2) with capacity <= 3/4 slots.  A key's home is
// fmix64(key) & (slots - 1), then linear probing over at most min(slots, 4096) slots.  KC_EMPTY = ~0 marks a free slot; a key is written
// once (claimed from KC_EMPTY) and its mask only ever gains bits.  The one key that equals KC_EMPTY keeps its mask in a side word.
// Bits at or above n_colors never enter a mask, and a key whose mask would be 0 is not inserted.  An occurrence that finds neither its
// key nor a free slot within the bound is DROPPED, and the index then refuses to be read.
//
// The screen.  m(x) = the index's mask of k-mer x, 0 when absent.  hits[c] counts the k-mers with bit c, single[c] those with
// m == 1 << c.  best = the colour with the most hits, ties to the smallest colour, KC_NONE without a hit; second = the same rule over
// the other colours.
#pragma once

#include <stdint.h>

#if defined(__HIPCC__) || defined(__CUDACC__)
#define KC_FN __host__ __device__ inline
#else
#define KC_FN inline
#endif
#define KC_HD KC_FN constexpr

// the values of include/needletail_amd_colors.h (the library asserts that they agree)
constexpr uint32_t KC_COLORS_MAX = 64;
constexpr uint64_t KC_NONE = ~(uint64_t)0;
constexpr uint64_t KC_EMPTY = ~(uint64_t)0;
constexpr uint32_t KC_PROBE_MAX = 4096;
// what kc_insert_or answers
enum : int { KC_DROPPED = -1, KC_MERGED = 0, KC_INSERTED = 1 };

// the murmur3 finaliser, the count table's hash
KC_HD uint64_t kc_fmix64(uint64_t x)
{
    x ^= x >> 33; x *= 0xff51afd7ed558ccdull;
    x ^= x >> 33; x *= 0xc4ceb9fe1a85ec53ull;
    x ^= x >> 33;
    return x;
}

KC_HD uint64_t kc_slots(uint64_t capacity)
{
    uint64_t slots = 2;
    while (capacity * 4 > slots * 3) slots <<= 1;
    return slots;
}

KC_HD uint32_t kc_probe_bound(uint64_t slots) { return slots < KC_PROBE_MAX ? (uint32_t)slots : KC_PROBE_MAX; }

KC_HD uint64_t kc_home(uint64_t key, uint64_t slots) { return kc_fmix64(key) & (slots - 1); }

// the bits a mask of an index of n_colors (1..64) may hold
KC_HD uint64_t kc_color_bits(uint32_t n_colors) { return n_colors >= 64 ? ~(uint64_t)0 : (((uint64_t)1 << n_colors) - 1); }

// OR `mask` (not 0, within kc_color_bits) into the entry of `key` (not KC_EMPTY), inserting the key if absent.  Mem: key(slot) reads a
// key; claim(slot, key) writes `key` if the slot holds KC_EMPTY and answers what the slot held before; or_mask(slot, mask).  A plain
// read may see a stale KC_EMPTY, so only what claim answers decides whether the slot is ours, this key's already, or another key's.
template <class Mem>
KC_FN int kc_insert_or(Mem &m, uint64_t slots, uint32_t probe_max, uint64_t key, uint64_t mask)
{
    uint64_t slot = kc_home(key, slots);
    for (uint32_t p = 0; p < probe_max; p++, slot = (slot + 1) & (slots - 1)) {
        uint64_t cur = m.key(slot);
        bool fresh = false;
        if (cur == KC_EMPTY) {
            cur = m.claim(slot, key);
            if (cur == KC_EMPTY) { cur = key; fresh = true; }
        }
        if (cur == key) {
            m.or_mask(slot, mask);
            return fresh ? KC_INSERTED : KC_MERGED;
        }
    }
    return KC_DROPPED;
}

// the mask of `key`, 0 when absent; `side`: the mask of the key that equals KC_EMPTY.  Mem: key(slot), mask(slot).
template <class Mem>
KC_FN uint64_t kc_lookup(const Mem &m, uint64_t slots, uint32_t probe_max, uint64_t side, uint64_t key)
{
    if (key == KC_EMPTY) return side;
    uint64_t slot = kc_home(key, slots);
    for (uint32_t p = 0; p < probe_max; p++, slot = (slot + 1) & (slots - 1)) {
        const uint64_t cur = m.key(slot);
        if (cur == key) return m.mask(slot);
        if (cur == KC_EMPTY) break;
    }
    return 0;
}

// what a k-mer with mask m adds: to hits[c] ...
KC_HD bool kc_has(uint64_t m, uint32_t c) { return (m >> c) & 1u; }
// ... to n_single, and with kc_has(m, c) to single[c]
KC_HD bool kc_is_single(uint64_t m) { return m != 0 && (m & (m - 1)) == 0; }

// THE TIE RULE, stated once: colour c with h hits beats colour b with g hits when it has more, or as many and the smaller number
KC_HD bool kc_beats(uint64_t h, uint64_t c, uint64_t g, uint64_t b) { return h > g || (h == g && c < b); }

// best and second of one finished row of the matrix: only colours with a hit stand
struct KcBest {
    uint64_t best, second;
};

KC_HD KcBest kc_best(const uint64_t *hits, uint32_t n_colors)
{
    uint64_t best = KC_NONE, second = KC_NONE, hb = 0, hs = 0;
    for (uint32_t c = 0; c < n_colors; c++) {
        const uint64_t h = hits[c];
        if (h == 0) continue;
        if (best == KC_NONE || kc_beats(h, c, hb, best)) {
            second = best; hs = hb;
            best = c; hb = h;
        } else if (second == KC_NONE || kc_beats(h, c, hs, second)) {
            second = c; hs = h;
        }
    }
    return KcBest{best, second};
}
