// The rule of the seed-index library (needletail_amd/csrc/ntk_si_rule.hpp) as a stand-alone program for tests/test_si_rule.py.
//
//   si_rule sweep   every key set of up to 6 of the 8 values of the universe, every max_occ 0..4 and every value of the universe as a
//                   seed: one line "mask max_occ value at class"; key number j of a set has occ 1 + j % 5.  Then, per set, the
//                   counts si_at_or_before gives for every value: "mask value count".
//   si_rule sort    a fixed set of anchors (every ref_rev of 4, rpos of 3 and qpos of 3, in a scrambled order) sorted with the rule's
//                   key and comparison: one line "ref_rev rpos qpos" each.  Compiled with -DSI_RULE_SWAPPED_KEY the program sorts on
//                   a key with rpos above ref_rev instead: the wrong library the test must tell from the right one.
#include "../needletail_amd/csrc/ntk_si_rule.hpp"

#include <algorithm>
#include <cstdio>
#include <cstring>
#include <vector>

static uint64_t universe(unsigned i) { return i == 7 ? ~(uint64_t)0 : (uint64_t)i * 0x2492492492492492ull; }   // 0 .. 2^64 - 1

static int sweep()
{
    for (unsigned mask = 0; mask < 256; mask++) {
        if (__builtin_popcount(mask) > 6) continue;
        std::vector<uint64_t> keys;
        for (unsigned i = 0; i < 8; i++)
            if (mask >> i & 1) keys.push_back(universe(i));
        // an array of exactly the keys: the sanitizer sees a read one behind them
        uint64_t *k = new uint64_t[keys.size()];
        if (!keys.empty()) memcpy(k, keys.data(), keys.size() * sizeof(uint64_t));
        for (uint32_t max_occ = 0; max_occ <= 4; max_occ++)
            for (unsigned v = 0; v < 8; v++) {
                const uint64_t at = si_find(k, keys.size(), universe(v));
                const bool present = at < keys.size() && k[at] == universe(v);
                printf("%u %u %u %llu %u\n", mask, max_occ, v, (unsigned long long)at, si_classify(present, present ? 1 + at % 5 : 0, max_occ));
            }
        for (unsigned v = 0; v < 8; v++) printf("%u %u %llu\n", mask, v, (unsigned long long)si_at_or_before(k, keys.size(), universe(v)));
        delete[] k;
    }
    return 0;
}

struct Anchor { uint32_t ref_rev, rpos, qpos; };

static uint64_t key_of(const Anchor &a)
{
#ifdef SI_RULE_SWAPPED_KEY
    return (uint64_t)a.rpos << 32 | a.ref_rev;
#else
    return si_sort_key(a.ref_rev, a.rpos);
#endif
}

static int sort_anchors()
{
    const uint32_t refs[4] = {si_ref_rev(si_ref(0, 0), 1), si_ref_rev(si_ref(0x7FFFFFFF, 1), 0), si_ref_rev(si_ref(3, 7), 1), si_ref_rev(si_ref(2, 2), 2)};
    const uint32_t pos[3] = {0xFFFFFFFFu, 0, 77};
    std::vector<Anchor> a;
    for (unsigned i = 0; i < 36; i++) {
        const unsigned j = i * 23 % 36;   // 23 and 36 have no common factor: every triple once, scrambled
        a.push_back({refs[j % 4], pos[j / 4 % 3], pos[j / 12]});
    }
    std::sort(a.begin(), a.end(), [](const Anchor &x, const Anchor &y) { return si_before(key_of(x), x.qpos, key_of(y), y.qpos); });
    for (const Anchor &x : a) printf("%u %u %u\n", x.ref_rev, x.rpos, x.qpos);
    return 0;
}

int main(int argc, char **argv)
{
    if (argc == 2 && !strcmp(argv[1], "sweep")) return sweep();
    if (argc == 2 && !strcmp(argv[1], "sort")) return sort_anchors();
    fprintf(stderr, "usage: si_rule sweep | sort\n");
    return 2;
}
