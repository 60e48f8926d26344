// The rule of the coloured k-mer index (needletail_amd/csrc/ntk_colors_rule.hpp) on the CPU, step by step as the kernels of ntk_colors.hip
// take it: insert-or-OR and lookup over heap arrays of exactly the library's sizes, the per-record accumulation in the wave's lane order
// (rounds of 64 window ends, one "ballot" per colour, lane c keeping column c), then the best / second pass over the finished row.
// tests/test_colors_rule.py feeds it cases on stdin and holds what it prints to tests/_colors_model.py; the same program is built with
// -fsanitize=address,undefined.
//
// Input, per case:
//   C n_colors capacity n_adds      then n_adds lines "key mask" (hex)
//   Q n_queries                     then n_queries hex keys on one line
//   R n_records                     then per record one line "n w0 w1 ..." with w = a hex key, or - for a window that is not emitted
// Output, per case:
//   S n_keys n_dropped n_masked_bits slots probe_bound side
//   P per_color[0 .. n_colors)
//   L the masks of the queries
//   per record: H n_kmers n_hit n_single best second | hits | single
#include "../needletail_amd/csrc/ntk_colors_rule.hpp"

#include <cinttypes>
#include <cstdio>
#include <cstdlib>
#include <cstring>

struct HostMem {
    uint64_t *keys, *masks;
    uint64_t key(uint64_t slot) const { return keys[slot]; }
    uint64_t mask(uint64_t slot) const { return masks[slot]; }
    uint64_t claim(uint64_t slot, uint64_t key)
    {
        const uint64_t before = keys[slot];
        if (before == KC_EMPTY) keys[slot] = key;
        return before;
    }
    void or_mask(uint64_t slot, uint64_t m) { masks[slot] |= m; }
};

static uint64_t ballot(const bool *p)
{
    uint64_t b = 0;
    for (int l = 0; l < 64; l++) b |= (uint64_t)p[l] << l;
    return b;
}

static bool read_hex(uint64_t &v)
{
    char tok[64];
    if (scanf("%63s", tok) != 1) return false;
    v = strtoull(tok, nullptr, 16);
    return true;
}

int main()
{
    unsigned n_colors;
    uint64_t capacity, n_adds;
    while (scanf(" C %u %" SCNu64 " %" SCNu64, &n_colors, &capacity, &n_adds) == 3) {
        const uint64_t slots = kc_slots(capacity), bits = kc_color_bits(n_colors);
        const uint32_t probe = kc_probe_bound(slots);
        HostMem mem{new uint64_t[slots], new uint64_t[slots]};
        for (uint64_t s = 0; s < slots; s++) { mem.keys[s] = KC_EMPTY; mem.masks[s] = 0; }
        uint64_t n_keys = 0, n_dropped = 0, n_masked = 0, side = 0;
        for (uint64_t i = 0; i < n_adds; i++) {   // kc_add_kernel, one key at a time
            uint64_t key, m;
            if (!read_hex(key) || !read_hex(m)) return 2;
            n_masked += (uint64_t)__builtin_popcountll(m & ~bits);
            m &= bits;
            if (m == 0) continue;
            if (key == KC_EMPTY) { side |= m; continue; }
            const int got = kc_insert_or(mem, slots, probe, key, m);
            n_keys += got == KC_INSERTED;
            n_dropped += got == KC_DROPPED;
        }
        printf("S %" PRIu64 " %" PRIu64 " %" PRIu64 " %" PRIu64 " %u %" PRIx64 "\n", n_keys + (side ? 1 : 0), n_dropped, n_masked, slots, probe, side);
        printf("P");
        for (unsigned c = 0; c < n_colors; c++) {   // kc_census_kernel
            uint64_t n = (side >> c) & 1u;
            for (uint64_t s = 0; s < slots; s++) n += mem.keys[s] != KC_EMPTY && kc_has(mem.masks[s], c);
            printf(" %" PRIu64, n);
        }
        printf("\n");
        uint64_t n_queries, n_records;
        if (scanf(" Q %" SCNu64, &n_queries) != 1) return 2;
        printf("L");
        for (uint64_t i = 0; i < n_queries; i++) {
            uint64_t q;
            if (!read_hex(q)) return 2;
            printf(" %" PRIx64, kc_lookup(mem, slots, probe, side, q));
        }
        printf("\n");
        if (scanf(" R %" SCNu64, &n_records) != 1) return 2;
        for (uint64_t r = 0; r < n_records; r++) {
            uint64_t n;
            if (scanf("%" SCNu64, &n) != 1) return 2;
            uint64_t *value = new uint64_t[n ? n : 1];
            bool *emitted = new bool[n ? n : 1];
            for (uint64_t i = 0; i < n; i++) {
                char tok[64];
                if (scanf("%63s", tok) != 1) return 2;
                emitted[i] = strcmp(tok, "-") != 0;
                value[i] = emitted[i] ? strtoull(tok, nullptr, 16) : 0;
            }
            // screen_rounds: lane l takes window 64 * round + l; lane c keeps hits[c] and single[c]
            uint64_t hits[64] = {}, single[64] = {}, n_kmers = 0, n_hit = 0, n_single = 0;
            for (uint64_t e0 = 0; e0 < n; e0 += 64) {
                uint64_t m[64];
                bool ok[64], any[64], one[64], has[64];
                for (int l = 0; l < 64; l++) {
                    const uint64_t e = e0 + l;
                    ok[l] = e < n && emitted[e];
                    m[l] = ok[l] ? kc_lookup(mem, slots, probe, side, value[e]) : 0;
                    any[l] = m[l] != 0;
                    one[l] = kc_is_single(m[l]);
                }
                n_kmers += (uint64_t)__builtin_popcountll(ballot(ok));
                if (!ballot(any)) continue;
                n_hit += (uint64_t)__builtin_popcountll(ballot(any));
                n_single += (uint64_t)__builtin_popcountll(ballot(one));
                for (unsigned c = 0; c < n_colors; c++) {
                    for (int l = 0; l < 64; l++) has[l] = kc_has(m[l], c);
                    hits[c] += (uint64_t)__builtin_popcountll(ballot(has));
                    for (int l = 0; l < 64; l++) has[l] = one[l] && kc_has(m[l], c);
                    single[c] += (uint64_t)__builtin_popcountll(ballot(has));
                }
            }
            const KcBest b = kc_best(hits, n_colors);   // kc_best_kernel
            printf("H %" PRIu64 " %" PRIu64 " %" PRIu64 " %" PRIu64 " %" PRIu64 " |", n_kmers, n_hit, n_single, b.best, b.second);
            for (unsigned c = 0; c < n_colors; c++) printf(" %" PRIu64, hits[c]);
            printf(" |");
            for (unsigned c = 0; c < n_colors; c++) printf(" %" PRIu64, single[c]);
            printf("\n");
            delete[] value;
            delete[] emitted;
        }
        delete[] mem.keys;
        delete[] mem.masks;
    }
    return 0;
}
