// A stand-alone host program around needletail_amd/csrc/ntk_mhset_rank.hpp (tests/test_mhset_rank.py builds and runs it, once plain and
// once with -fsanitize=address,undefined).  It walks A in rounds of 64 lanes with an emulated ballot, step for step as pair_wave of
// ntk_minhash_set.hip does, and writes seven doubles per case: n_a, n_b, n_shared, n_union, dot, norm2_a, norm2_b.
//
//   mhset_rank_main subsets NUM MAX_HASH U0..U7 CA0..CA7 CB0..CB7   every pair (A, B) of subsets of the universe U (ascending), A's mask
//                                                                   outermost: 65536 cases
//   mhset_rank_main file PATH                                       uint64 words: n_cases, then per case na, nb, num, max_hash,
//                                                                   a[na], ca[na], b[nb], cb[nb]
#include "../needletail_amd/csrc/ntk_mhset_rank.hpp"

#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

struct Walk {
    uint64_t n_shared, n_union;
    double dot, norm2;
};

// one wave: A (after the cut) walked against B (after the cut)
static Walk walk(const uint64_t *a, const uint64_t *ca, uint32_t na, const uint64_t *b, const uint64_t *cb, uint32_t nb, uint64_t num)
{
    const bool to_num = ms_union_is_num(num, na, nb);
    MsLane acc[64];
    uint64_t carry = 0;
    for (uint64_t base = 0; base < na; base += 64) {
        MsHit hit[64];
        bool live[64];
        double x[64], y[64];
        uint64_t ballot = 0;
        for (uint32_t lane = 0; lane < 64; lane++) {
            const uint64_t i = base + lane;
            live[lane] = i < na;
            hit[lane].p = 0; hit[lane].shared = false;
            x[lane] = y[lane] = 1.0;
            if (live[lane]) {
                // exactly nb elements are handed over: the sanitizer build faults on any probe past them
                hit[lane] = ms_probe(b, nb, a[i]);
                if (ca) x[lane] = (double)ca[i];
                if (cb && hit[lane].shared) y[lane] = (double)cb[hit[lane].p];
            }
            if (hit[lane].shared) ballot |= (uint64_t)1 << lane;
        }
        uint64_t last = 0;
        for (uint32_t lane = 0; lane < 64; lane++)
            last = ms_lane_step(acc[lane], live[lane], base + lane, hit[lane], ballot, lane, carry, num, x[lane], y[lane]);
        carry += (uint64_t)__builtin_popcountll(ballot);
        if (to_num && last >= num) break;   // lane 63's position
    }
    Walk w = {0, 0, 0.0, 0.0};
    for (int off = 32; off > 0; off >>= 1)   // the butterfly of the wave reductions
        for (int lane = 0; lane < off; lane++) {
            acc[lane].n_shared += acc[lane + off].n_shared;
            acc[lane].dot += acc[lane + off].dot;
            acc[lane].norm2 += acc[lane + off].norm2;
        }
    w.n_shared = acc[0].n_shared; w.dot = acc[0].dot; w.norm2 = acc[0].norm2;
    w.n_union = ms_union(num, na, nb, carry);
    return w;
}

static void one_case(const std::vector<uint64_t> &a, const std::vector<uint64_t> &ca, const std::vector<uint64_t> &b,
                     const std::vector<uint64_t> &cb, uint64_t num, uint64_t max_hash, FILE *out)
{
    const uint32_t na = (uint32_t)ms_cut_length(a.data(), a.size(), max_hash), nb = (uint32_t)ms_cut_length(b.data(), b.size(), max_hash);
    // exact-size copies of the cut sketches, so that a read past a sketch's end is a heap overflow the sanitizer sees
    const std::vector<uint64_t> a2(a.begin(), a.begin() + na), ca2(ca.begin(), ca.begin() + na), b2(b.begin(), b.begin() + nb),
        cb2(cb.begin(), cb.begin() + nb);
    const Walk first = walk(a2.data(), ca2.data(), na, b2.data(), cb2.data(), nb, num);
    const Walk swapped = walk(b2.data(), cb2.data(), nb, a2.data(), ca2.data(), na, num);
    const double row[7] = {(double)na, (double)nb, (double)first.n_shared, (double)first.n_union, first.dot, first.norm2, swapped.norm2};
    fwrite(row, sizeof(double), 7, out);
}

int main(int argc, char **argv)
{
    if (argc == 28 && !strcmp(argv[1], "subsets")) {
        const uint64_t num = strtoull(argv[2], nullptr, 10), max_hash = strtoull(argv[3], nullptr, 10);
        uint64_t u[8], ca[8], cb[8];
        for (int j = 0; j < 8; j++) {
            u[j] = strtoull(argv[4 + j], nullptr, 10);
            ca[j] = strtoull(argv[12 + j], nullptr, 10);
            cb[j] = strtoull(argv[20 + j], nullptr, 10);
        }
        for (unsigned ma = 0; ma < 256; ma++)
            for (unsigned mb = 0; mb < 256; mb++) {
                std::vector<uint64_t> a, xa, b, xb;
                for (int j = 0; j < 8; j++) {
                    if (ma >> j & 1) { a.push_back(u[j]); xa.push_back(ca[j]); }
                    if (mb >> j & 1) { b.push_back(u[j]); xb.push_back(cb[j]); }
                }
                one_case(a, xa, b, xb, num, max_hash, stdout);
            }
        return 0;
    }
    if (argc == 3 && !strcmp(argv[1], "file")) {
        FILE *f = fopen(argv[2], "rb");
        if (!f) return 3;
        uint64_t n_cases = 0;
        if (fread(&n_cases, 8, 1, f) != 1) return 3;
        for (uint64_t c = 0; c < n_cases; c++) {
            uint64_t head[4];
            if (fread(head, 8, 4, f) != 4) return 3;
            std::vector<uint64_t> a(head[0]), ca(head[0]), b(head[1]), cb(head[1]);
            if (fread(a.data(), 8, a.size(), f) != a.size() || fread(ca.data(), 8, ca.size(), f) != ca.size() ||
                fread(b.data(), 8, b.size(), f) != b.size() || fread(cb.data(), 8, cb.size(), f) != cb.size())
                return 3;
            one_case(a, ca, b, cb, head[2], head[3], stdout);
        }
        fclose(f);
        return 0;
    }
    fprintf(stderr, "usage: mhset_rank_main subsets NUM MAX_HASH U*8 CA*8 CB*8 | file PATH\n");
    return 2;
}
