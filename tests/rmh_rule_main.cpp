// The guess / accept / raise rule of the per-record MinHash sketches (needletail_amd/csrc/ntk_rmh_rule.hpp) on the CPU, driven by
// tests/test_rmh_rule.py.  A record is a multiset of hashes; a round is emulated as the library runs it: the filter adds every
// occurrence of every hash in [lo, tau] to what the record holds, the distinct hashes held are counted, the record is accepted or its
// threshold raised and lo set behind the old one.
//
//   rmh_rule_main walk U0 .. U9       every multiset of at most 8 hashes of the universe x num 1..9 x every first threshold of the
//                                     universe and ~0: the accepted result must be the plain cut; prints "cases rounds_max raises"
//   rmh_rule_main trace NUM TAU H...  one record: prints the thresholds of its rounds, then "hash count" lines of the result
//   rmh_rule_main guess NUM N         rmh_guess(n, NUM) for n = 0 .. N, one per line
#include "../needletail_amd/csrc/ntk_rmh_rule.hpp"

#include <algorithm>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <map>
#include <vector>

using Sketch = std::vector<std::pair<uint64_t, uint64_t>>;

// the num smallest distinct hashes with all their occurrences
static Sketch plain_cut(const std::vector<uint64_t> &hashes, uint64_t num)
{
    std::map<uint64_t, uint64_t> all;
    for (uint64_t h : hashes) all[h]++;
    Sketch out(all.begin(), all.end());
    if (out.size() > num) out.resize(num);
    return out;
}

// The rounds.  Returns the result; `taus` gets the threshold of every round.  Fails (exit 1) where a raise does not rise or the rounds
// do not end.
static Sketch by_rounds(const std::vector<uint64_t> &hashes, uint64_t num, uint64_t tau, std::vector<uint64_t> &taus)
{
    std::map<uint64_t, uint64_t> held;
    uint64_t lo = 0;
    for (int round = 0; round < 40; round++) {
        taus.push_back(tau);
        for (uint64_t h : hashes)
            if (h >= lo && h <= tau) held[h]++;
        // the fold keeps the first num per record after every round
        while (held.size() > num) held.erase(std::prev(held.end()));
        if (rmh_accept(tau, held.size(), num)) return Sketch(held.begin(), held.end());
        const uint64_t next = rmh_raise(tau, held.size(), num);
        if (next <= tau) { fprintf(stderr, "raise(%llu) = %llu does not rise\n", (unsigned long long)tau, (unsigned long long)next); exit(1); }
        lo = tau + 1;
        tau = next;
    }
    fprintf(stderr, "the rounds do not end\n");
    exit(1);
}

int main(int argc, char **argv)
{
    if (argc >= 12 && !strcmp(argv[1], "walk")) {
        uint64_t u[10];
        for (int i = 0; i < 10; i++) u[i] = strtoull(argv[2 + i], nullptr, 0);
        uint64_t cases = 0, rounds_max = 0, raises = 0;
        std::vector<uint64_t> hashes, taus;
        // multisets as non-decreasing index sequences of length 0 .. 8
        int idx[8];
        for (int len = 0; len <= 8; len++) {
            for (int i = 0; i < len; i++) idx[i] = 0;
            for (;;) {
                hashes.clear();
                for (int i = 0; i < len; i++) hashes.push_back(u[idx[i]]);
                for (uint64_t num = 1; num <= 9; num++) {
                    const Sketch want = plain_cut(hashes, num);
                    for (int t = 0; t <= 10; t++) {
                        taus.clear();
                        const Sketch got = by_rounds(hashes, num, t < 10 ? u[t] : kRmhAll, taus);
                        if (got != want) {
                            fprintf(stderr, "num %llu, first threshold %d: the accepted result is not the cut\n", (unsigned long long)num, t);
                            return 1;
                        }
                        if (taus.back() != kRmhAll && got.size() < num) {
                            fprintf(stderr, "accepted below ~0 with fewer than num hashes\n");
                            return 1;
                        }
                        cases++;
                        raises += taus.size() - 1;
                        if (taus.size() > rounds_max) rounds_max = taus.size();
                    }
                }
                int i = len - 1;
                while (i >= 0 && idx[i] == 9) i--;
                if (i < 0) break;
                const int v = idx[i] + 1;
                for (; i < len; i++) idx[i] = v;
            }
        }
        printf("%llu %llu %llu\n", (unsigned long long)cases, (unsigned long long)rounds_max, (unsigned long long)raises);
        return 0;
    }
    if (argc >= 4 && !strcmp(argv[1], "trace")) {
        const uint64_t num = strtoull(argv[2], nullptr, 0), tau = strtoull(argv[3], nullptr, 0);
        std::vector<uint64_t> hashes, taus;
        for (int i = 4; i < argc; i++) hashes.push_back(strtoull(argv[i], nullptr, 0));
        const Sketch got = by_rounds(hashes, num, tau, taus);
        for (size_t i = 0; i < taus.size(); i++) printf("%s%llu", i ? " " : "", (unsigned long long)taus[i]);
        printf("\n");
        for (const auto &e : got) printf("%llu %llu\n", (unsigned long long)e.first, (unsigned long long)e.second);
        return 0;
    }
    if (argc == 4 && !strcmp(argv[1], "guess")) {
        const uint64_t num = strtoull(argv[2], nullptr, 0), n = strtoull(argv[3], nullptr, 0);
        for (uint64_t i = 0; i <= n; i++) printf("%llu\n", (unsigned long long)rmh_guess(i, num));
        return 0;
    }
    fprintf(stderr, "usage: rmh_rule_main walk U0 .. U9 | trace NUM TAU H... | guess NUM N\n");
    return 2;
}
