// A stand-alone host program around needletail_amd/csrc/ntk_kset_rule.hpp (tests/test_kset_rule.py builds and runs it, once plain and
// once with -fsanitize=address,undefined).  It walks the merged order tile by tile, step for step as ks_split_kernel and ks_join_kernel of
// ntk_kmer_sets.hip do: the splits, the view, exact-size heap copies of what a tile stages (so that a search past a range's end is a
// heap overflow the sanitizer sees), every element's probe, the bins and sums of COMPARE, the tile counts of COUNT, and WRITE's slots
// stored in slot order below the tile's count.
//
// Every case writes uint64 words: the joint histogram (bins_a * bins_b), the thirteen totals, then for each of the twelve (op, rule)
// pairs of OPS below: n, `pad` keys (pad * kw words) and `pad` counts, the entries past n zero.
//
//   kset_rule_main subsets KW T BINS_A BINS_B U[8 * KW] CA[8] CB[8]   every pair (A, B) of subsets of the ascending universe U, A's mask
//                                                                    outermost: 65536 cases, pad = 8
//   kset_rule_main file PATH                                         uint64 words: n_cases, then per case kw, T, n_a, n_b, bins_a, bins_b,
//                                                                    a_keys, a_counts, b_keys, b_counts; pad = n_a + n_b
#include "../needletail_amd/csrc/ntk_kset_rule.hpp"

#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

typedef std::vector<uint64_t> Words;

static const uint32_t OPS[12][2] = {
    {KS_INTERSECT, KS_MIN}, {KS_INTERSECT, KS_MAX}, {KS_INTERSECT, KS_SUM}, {KS_INTERSECT, KS_LEFT}, {KS_INTERSECT, KS_RIGHT},
    {KS_UNION, KS_MIN}, {KS_UNION, KS_MAX}, {KS_UNION, KS_SUM}, {KS_UNION, KS_LEFT}, {KS_UNION, KS_RIGHT},
    {KS_SUBTRACT, 0}, {KS_COUNTERS_SUBTRACT, 0}};

static void put(const Words &w, FILE *out)
{
    if (!w.empty()) fwrite(w.data(), 8, w.size(), out);   // (an empty vector's data() may be null)
}

struct Lists {
    Words a, ca, b, cb;
    uint64_t n_a, n_b;
};

// what a tile stages, as exact-size heap arrays
template <int KW>
struct Stage {
    KsView v;
    Words sa, sb;

    Stage(const Lists &l, const Words &splits, uint64_t t, uint64_t T)
    {
        const uint64_t n = l.n_a + l.n_b, d0 = t * T, d1 = d0 + T < n ? d0 + T : n;
        v = ks_view(splits[t], splits[t + 1], d0, d1, l.n_b);
        sa.assign(l.a.begin() + v.sa0 * KW, l.a.begin() + (v.sa0 + v.na) * KW);
        sb.assign(l.b.begin() + v.j0 * KW, l.b.begin() + (v.j0 + v.nb) * KW);
        sa.shrink_to_fit(); sb.shrink_to_fit();
    }
};

template <int KW>
static Words splits_of(const Lists &l, uint64_t T, uint64_t &n_tiles)
{
    const uint64_t n = l.n_a + l.n_b;
    n_tiles = (n + T - 1) / T;
    Words s(n_tiles + 1);
    for (uint64_t t = 0; t <= n_tiles; t++) s[t] = ks_split<KW>(l.a.data(), l.n_a, l.b.data(), l.n_b, t * T < n ? t * T : n);
    return s;
}

template <int KW>
static void compare(const Lists &l, uint64_t T, uint32_t bins_a, uint32_t bins_b, FILE *out)
{
    Words hist((size_t)bins_a * bins_b, 0);
    KsSums acc;
    uint64_t n_tiles = 0;
    const Words splits = splits_of<KW>(l, T, n_tiles);
    for (uint64_t t = 0; t < n_tiles; t++) {
        const Stage<KW> s(l, splits, t, T);
        const KsView &v = s.v;
        for (uint32_t e = 0; e < v.la + v.lb; e++) {
            if (e < v.la) {
                const KsHit hit = ks_probe_a<KW>(v, s.sa.data(), s.sb.data(), e);
                const uint64_t ca = l.ca.at(v.i0 + e), cb = hit.shared ? l.cb.at(v.j0 + hit.twin) : 0;
                hist.at(ks_compare_a(acc, hit.shared, ca, cb, bins_a, bins_b))++;
            } else {
                const uint32_t y = e - v.la;
                const KsHit hit = ks_probe_b<KW>(v, s.sa.data(), s.sb.data(), y);
                if (!hit.shared) hist.at(ks_compare_b(acc, l.cb.at(v.j0 + y), bins_b))++;
            }
        }
    }
    const uint64_t sums[KS_N_SUMS] = {acc.n_shared, acc.sum_a, acc.sum_a_shared, acc.sum_b_shared, acc.sum_b_only, acc.sum_min};
    uint64_t totals[13];
    ks_totals(sums, l.n_a, l.n_b, totals);
    put(hist, out);
    fwrite(totals, 8, 13, out);
}

// one tile of COUNT (slots == nullptr) or WRITE: the kept elements; WRITE parks them at their slots
template <int KW>
static uint32_t tile_pass(const Lists &l, const Stage<KW> &s, uint32_t op, uint32_t rule, bool with_counts, std::vector<int> *slot_src,
                          Words *slot_count)
{
    const KsView &v = s.v;
    uint32_t kept = 0;
    for (uint32_t e = 0; e < v.la + v.lb; e++) {
        if (e < v.la) {
            const KsHit hit = ks_probe_a<KW>(v, s.sa.data(), s.sb.data(), e);
            const uint64_t ca = with_counts && ks_a_needs_a(op, hit.shared) ? l.ca.at(v.i0 + e) : 0;
            const uint64_t cb = with_counts && ks_a_needs_b(op, hit.shared) ? l.cb.at(v.j0 + hit.twin) : 0;
            uint64_t count = 0;
            if (ks_out_a(op, rule, hit.shared, ca, cb, count)) {
                kept++;
                if (slot_src) { slot_src->at(hit.slot) = (int)(v.a_first + e); slot_count->at(hit.slot) = count; }
            }
        } else {
            const uint32_t y = e - v.la;
            const KsHit hit = ks_probe_b<KW>(v, s.sa.data(), s.sb.data(), y);
            if (ks_out_b(op, hit.shared)) {
                kept++;
                if (slot_src) { slot_src->at(hit.slot) = (int)(v.na + y); slot_count->at(hit.slot) = l.cb.at(v.j0 + y); }
            }
        }
    }
    return kept;
}

template <int KW>
static void apply(const Lists &l, uint64_t T, uint32_t op, uint32_t rule, uint64_t pad, FILE *out)
{
    uint64_t n_tiles = 0;
    const Words splits = splits_of<KW>(l, T, n_tiles);
    Words bases(n_tiles + 1, 0);
    for (uint64_t t = 0; t < n_tiles; t++)   // COUNT, then the exclusive scan
        bases[t + 1] = bases[t] + tile_pass<KW>(l, Stage<KW>(l, splits, t, T), op, rule, op == KS_COUNTERS_SUBTRACT, nullptr, nullptr);
    const uint64_t total = bases[n_tiles];
    if (total > pad) abort();
    Words keys(pad * KW, 0), counts(pad, 0);
    for (uint64_t t = 0; t < n_tiles; t++) {   // WRITE
        const Stage<KW> s(l, splits, t, T);
        Words staged(s.sa);
        staged.insert(staged.end(), s.sb.begin(), s.sb.end());
        const uint32_t len = s.v.la + s.v.lb;
        std::vector<int> slot_src(len, -1);   // exactly the tile's slots: a slot at or past len is an overflow
        Words slot_count(len, 0);
        (void)tile_pass<KW>(l, s, op, rule, true, &slot_src, &slot_count);
        const uint64_t limit = bases[t + 1] - bases[t];
        uint64_t rank = 0;
        for (uint32_t m = 0; m < len; m++) {
            if (slot_src[m] < 0) continue;
            if (rank < limit) {
                for (int q = 0; q < KW; q++) keys.at((bases[t] + rank) * KW + q) = staged.at((size_t)slot_src[m] * KW + q);
                counts.at(bases[t] + rank) = slot_count[m];
            }
            rank++;
        }
    }
    fwrite(&total, 8, 1, out);
    put(keys, out);
    put(counts, out);
}

static void one_case(int kw, const Lists &l, uint64_t T, uint32_t bins_a, uint32_t bins_b, uint64_t pad, FILE *out)
{
    if (kw == 1) compare<1>(l, T, bins_a, bins_b, out); else compare<2>(l, T, bins_a, bins_b, out);
    for (const auto &o : OPS) {
        if (!ks_op_ok(o[0], o[1])) abort();
        if (kw == 1) apply<1>(l, T, o[0], o[1], pad, out); else apply<2>(l, T, o[0], o[1], pad, out);
    }
}

static Lists exact(const Words &a, const Words &ca, const Words &b, const Words &cb)
{
    Lists l;
    l.a = a; l.ca = ca; l.b = b; l.cb = cb;
    for (Words *w : {&l.a, &l.ca, &l.b, &l.cb}) w->shrink_to_fit();
    l.n_a = ca.size(); l.n_b = cb.size();
    return l;
}

int main(int argc, char **argv)
{
    if (argc >= 6 && !strcmp(argv[1], "subsets")) {
        const int kw = atoi(argv[2]);
        const uint64_t T = strtoull(argv[3], nullptr, 10);
        const uint32_t bins_a = (uint32_t)atoi(argv[4]), bins_b = (uint32_t)atoi(argv[5]);
        if ((kw != 1 && kw != 2) || T == 0 || argc != 6 + 8 * kw + 16) return 2;
        uint64_t u[16], ca[8], cb[8];
        for (int j = 0; j < 8 * kw; j++) u[j] = strtoull(argv[6 + j], nullptr, 10);
        for (int j = 0; j < 8; j++) {
            ca[j] = strtoull(argv[6 + 8 * kw + j], nullptr, 10);
            cb[j] = strtoull(argv[14 + 8 * kw + j], nullptr, 10);
        }
        for (unsigned ma = 0; ma < 256; ma++)
            for (unsigned mb = 0; mb < 256; mb++) {
                Words a, xa, b, xb;
                for (int j = 0; j < 8; j++) {
                    if (ma >> j & 1) { a.insert(a.end(), u + j * kw, u + (j + 1) * kw); xa.push_back(ca[j]); }
                    if (mb >> j & 1) { b.insert(b.end(), u + j * kw, u + (j + 1) * kw); xb.push_back(cb[j]); }
                }
                one_case(kw, exact(a, xa, b, xb), T, bins_a, bins_b, 8, stdout);
            }
        return 0;
    }
    if (argc == 3 && !strcmp(argv[1], "file")) {
        FILE *f = fopen(argv[2], "rb");
        if (!f) return 3;
        uint64_t n_cases = 0;
        if (fread(&n_cases, 8, 1, f) != 1) return 3;
        for (uint64_t c = 0; c < n_cases; c++) {
            uint64_t head[6];
            if (fread(head, 8, 6, f) != 6 || (head[0] != 1 && head[0] != 2) || head[1] == 0) return 3;
            Words a(head[2] * head[0]), ca(head[2]), b(head[3] * head[0]), cb(head[3]);
            if (fread(a.data(), 8, a.size(), f) != a.size() || fread(ca.data(), 8, ca.size(), f) != ca.size() ||
                fread(b.data(), 8, b.size(), f) != b.size() || fread(cb.data(), 8, cb.size(), f) != cb.size())
                return 3;
            one_case((int)head[0], exact(a, ca, b, cb), head[1], (uint32_t)head[4], (uint32_t)head[5], head[2] + head[3], stdout);
        }
        fclose(f);
        return 0;
    }
    fprintf(stderr, "usage: kset_rule_main subsets KW T BINS_A BINS_B U*8KW CA*8 CB*8 | file PATH\n");
    return 2;
}
