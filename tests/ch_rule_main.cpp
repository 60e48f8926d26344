// The rule of the chain library (needletail_amd/csrc/ntk_chain_rule.hpp) as a stand-alone program for tests/test_ch_rule.py.
//
//   ch_rule gap     for every k of 1, 15, 255 and every dd of the sweep (0..4, every 2^e and 2^e +- 1 below 2^31, and bw, bw + 1 of the two
//                   parameter sets): one line "k dd ilog2 gap" (ilog2 of max(dd, 1)).
//   ch_rule pair    for every k, both parameter sets (max_dist, bw), both strands and every (dr, dq) of the sweep - dr and dq of 0, 1,
//                   k - 1, k, k + 1, max_dist, max_dist + 1, dq of -1 and -max_dist, and pairs with dd of bw and bw + 1 on both sides:
//                   one line "k set rev dr dq ok gain gap candidate-score p", the last two from ch_candidate with f_j = 100 and j = 7
//                   through ch_f_of and ch_p_of.  Compiled with -DCH_RULE_WRONG_GAP the program costs a gap with 40 for 41: the wrong
//                   library the test must tell from the right one.
//   ch_rule misc    ch_run_head, ch_before, ch_at_or_before and ch_visit_key on fixed inputs, one line each.
#include "../needletail_amd/csrc/ntk_chain_rule.hpp"

#include <algorithm>
#include <cstdio>
#include <cstring>
#include <vector>

static const uint32_t kK[3] = {1, 15, 255};
static const uint32_t kSets[2][2] = {{5000, 500}, {200, 10}};

static std::vector<uint32_t> dd_sweep()
{
    std::vector<uint32_t> v = {0, 1, 2, 3, 4};
    for (uint32_t e = 0; e < 31; e++) {
        const uint32_t p = (uint32_t)1 << e;
        if (p > 1) v.push_back(p - 1);
        v.push_back(p);
        if (p + 1 < ((uint32_t)1 << 31)) v.push_back(p + 1);
    }
    v.push_back(0x7FFFFFFFu);
    for (const auto &s : kSets) { v.push_back(s[1]); v.push_back(s[1] + 1); }
    std::sort(v.begin(), v.end());
    v.erase(std::unique(v.begin(), v.end()), v.end());
    return v;
}

static uint64_t gap_of(uint32_t dd, uint32_t k)
{
#ifdef CH_RULE_WRONG_GAP
    return dd == 0 ? 0 : (((uint64_t)dd * k * 40) >> 12) + (ch_ilog2(dd) >> 1);
#else
    return ch_gap(dd, k);
#endif
}

static int gap()
{
    for (uint32_t k : kK)
        for (uint32_t dd : dd_sweep())
            printf("%u %u %u %llu\n", k, dd, ch_ilog2(dd ? dd : 1), (unsigned long long)gap_of(dd, k));
    return 0;
}

static int pair()
{
    const int64_t base = 1000000;
    for (uint32_t k : kK)
        for (unsigned set = 0; set < 2; set++) {
            const ch_rule_params r = {k, kSets[set][0], kSets[set][1], 64};
            const int64_t md = r.max_dist, bw = r.bw;
            std::vector<int64_t> d = {0, 1, (int64_t)k - 1, k, (int64_t)k + 1, md, md + 1};
            std::vector<std::pair<int64_t, int64_t>> sweep;
            for (int64_t dr : d)
                for (int64_t dq : d) sweep.push_back({dr, dq});
            for (int64_t dr : d) { sweep.push_back({dr, -1}); sweep.push_back({dr, -md}); }
            for (int64_t a : {(int64_t)1, (int64_t)k, (int64_t)100})
                for (int64_t extra : {bw, bw + 1}) { sweep.push_back({a, a + extra}); sweep.push_back({a + extra, a}); }
            for (uint32_t rev = 0; rev < 2; rev++)
                for (const auto &s : sweep) {
                    const uint32_t rj = (uint32_t)base, qj = (uint32_t)base, ri = (uint32_t)(base + s.first);
                    const uint32_t qi = (uint32_t)(rev ? base - s.second : base + s.second);
                    uint32_t gain = 0;
                    uint64_t cost = 0;
                    const bool ok = ch_pair(rev, rj, qj, ri, qi, r, gain, cost);
                    const uint64_t cand = ch_candidate(rev, rj, qj, 100, 7, ri, qi, r);
                    printf("%u %u %u %lld %lld %d %u %llu %d %u\n", k, set, rev, (long long)s.first, (long long)s.second, (int)ok, ok ? gain : 0,
                           (unsigned long long)(ok ? cost : 0), ch_f_of(cand, k), ch_p_of(cand));
                }
        }
    return 0;
}

static int misc()
{
    // run heads: the first of a read; another ref_rev; gaps of max_dist and max_dist + 1; rpos at the top of its range
    printf("%d %d %d %d %d\n", (int)ch_run_head(true, 0, 0, 0, 0, 5000), (int)ch_run_head(false, 2, 100, 3, 100, 5000),
           (int)ch_run_head(false, 2, 100, 2, 5100, 5000), (int)ch_run_head(false, 2, 100, 2, 5101, 5000),
           (int)ch_run_head(false, 2, 1, 2, 0xFFFFFFFFu, 0x7FFFFFFFu));
    // the order of the triples: ref_rev, then rpos, then qpos; equal triples are not in front of each other
    printf("%d %d %d %d %d %d\n", (int)ch_before(0, 9, 9, 1, 0, 0), (int)ch_before(1, 0, 0, 0, 9, 9), (int)ch_before(1, 4, 9, 1, 5, 0),
           (int)ch_before(1, 5, 3, 1, 5, 4), (int)ch_before(1, 5, 4, 1, 5, 4), (int)ch_before(1, 5, 5, 1, 5, 4));
    // an anchor's read: offsets with empty reads, on an array of exactly their size
    uint64_t *off = new uint64_t[6];
    const uint64_t values[6] = {2, 2, 5, 5, 5, 9};
    memcpy(off, values, sizeof values);
    for (uint64_t x = 0; x < 11; x++) printf("%llu ", (unsigned long long)ch_at_or_before(off, 6, x));
    printf("%llu\n", (unsigned long long)ch_at_or_before(off, 0, 3));
    delete[] off;
    printf("%llu %llu %llu\n", (unsigned long long)ch_visit_key(0x7FFFFFFF, 0), (unsigned long long)ch_visit_key(15, 0xFFFFFFFFu),
           (unsigned long long)ch_visit_key(0, 1));
    return 0;
}

int main(int argc, char **argv)
{
    if (argc == 2 && !strcmp(argv[1], "gap")) return gap();
    if (argc == 2 && !strcmp(argv[1], "pair")) return pair();
    if (argc == 2 && !strcmp(argv[1], "misc")) return misc();
    fprintf(stderr, "usage: ch_rule gap | pair | misc\n");
    return 2;
}
