// The CPU walk of needletail_amd/csrc/ntk_dbg_rule.hpp (tests/test_dbg_rule.py): every per-element step in the order ntk_dbg.hip launches
// them - directory marks and the running minimum, the edge bytes with their targets, the links, the ranking rounds between two buffers
// with the cut of the cycles, the resolve, the two scans, the order, the rows and the spelling - on heap arrays of exactly the sizes the
// library allocates, so that an index that leaves an array is a sanitizer report.  Also checks, on every case, that a bit is set iff
// its mate's is.
//
// stdin: cases of "k n" and n lines "key(hex) count(hex)".  stdout, per case:
//   E <n edge bytes>            T <31 totals>           K <n pairs unitig pos_flip>      U <n_unitigs> <n_bases> <rounds> <mates_ok>
//   R <start n_kmers sum flags> and S <bases>, one of each per unitig
#include "../needletail_amd/csrc/ntk_dbg_rule.hpp"

#include <cinttypes>
#include <cstdio>
#include <cstring>
#include <memory>
#include <string>

template <class T>
static std::unique_ptr<T[]> exact(uint64_t n) { return std::unique_ptr<T[]>(new T[n]()); }

struct Scan { uint64_t units, kmers; };

static uint32_t rounds(uint32_t n, std::unique_ptr<uint64_t[]> pd[2], std::unique_ptr<uint32_t[]> mn[2], int &cur)
{
    uint32_t done = 0;
    for (uint32_t r = 0; r < dbg_rounds_max(n); r++) {
        bool moved = false;
        for (uint64_t d = 0; d < 2 * (uint64_t)n; d++) moved |= dbg_rank_round(pd[cur].get(), mn[cur].get(), pd[cur ^ 1].get(), mn[cur ^ 1].get(), (uint32_t)d);
        cur ^= 1;
        done++;
        if (!moved) break;
    }
    return done;
}

static int run_case(uint32_t k, uint32_t n, const uint64_t *keys, const uint64_t *counts)
{
    const uint32_t b = dbg_dir_bits(k, n);
    const uint64_t words = dbg_dir_words(k, n);
    uint64_t sums[DBG_N_SUMS] = {}, totals[DBG_N_TOTALS] = {};
    auto edges = exact<uint8_t>(n);
    auto kmer_rows = exact<uint32_t>(2 * (uint64_t)n);
    uint64_t n_unitigs = 0, n_rounds = 0;
    bool mates_ok = true;
    std::string rows_text;
    if (n) {
        // the directory
        auto rdir = exact<uint32_t>(words);
        memset(rdir.get(), 0xFF, words * sizeof(uint32_t));
        for (uint32_t i = 0; i < n; i++) {
            uint64_t slot = 0;
            if (dbg_dir_mark(keys, k, b, i, slot) && i < rdir[slot]) rdir[slot] = i;
            if (i == 0) rdir[0] = n;
        }
        for (uint64_t w = 1; w < words; w++)
            if (rdir[w - 1] < rdir[w]) rdir[w] = rdir[w - 1];
        // the edge bytes
        auto tgt = exact<uint32_t>(2 * (uint64_t)n);
        for (uint32_t i = 0; i < n; i++) {
            const DbgAdj a = dbg_adjacency(keys, n, rdir.get(), k, b, i);
            edges[i] = (uint8_t)a.edges;
            tgt[2 * (uint64_t)i] = a.tgt[0];
            tgt[2 * (uint64_t)i + 1] = a.tgt[1];
            sums[DBG_SUM_HIST + dbg_deg_bin(a.edges)]++;
            sums[DBG_SUM_SELF] += a.n_self;
        }
        // a bit is set iff its mate's is (the target found again through the directory)
        for (uint32_t i = 0; i < n; i++)
            for (uint32_t bit = 0; bit < 8; bit++) {
                if (!((edges[i] >> bit) & 1)) continue;
                const uint64_t x = keys[i] & dbg_mask(k), rx = dbg_rc(x, k);
                const uint32_t side = bit >> 2, c = bit & 3;
                const uint64_t t = dbg_ext(side ? rx : x, k, c), rt = dbg_ext_rc(side ? x : rx, k, c), y = t < rt ? t : rt;
                const uint32_t j = dbg_lower_dir(keys, n, rdir.get(), k, b, y);
                uint32_t side2 = 0, c2 = 0;
                dbg_mate(x, k, side, c, side2, c2);
                if (j >= n || keys[j] != y || !((edges[j] >> (4 * side2 + c2)) & 1)) mates_ok = false;
            }
        // the links
        auto next = exact<uint32_t>(2 * (uint64_t)n);
        for (uint64_t d = 0; d < 2 * (uint64_t)n; d++) {
            next[d] = dbg_link(keys, edges.get(), tgt.get(), n, k, (uint32_t)(d >> 1), (uint32_t)(d & 1));
            sums[DBG_SUM_LINKS] += next[d] != DBG_NONE;
        }
        // the ranking
        std::unique_ptr<uint64_t[]> pd[2] = {exact<uint64_t>(2 * (uint64_t)n), exact<uint64_t>(2 * (uint64_t)n)};
        std::unique_ptr<uint32_t[]> mn[2] = {exact<uint32_t>(2 * (uint64_t)n), exact<uint32_t>(2 * (uint64_t)n)};
        int cur = 0;
        for (uint64_t d = 0; d < 2 * (uint64_t)n; d++) dbg_rank_init(next.get(), (uint32_t)d, pd[0][d], mn[0][d]);
        n_rounds += rounds(n, pd, mn, cur);
        bool cycles = false;
        for (uint64_t d = 0; d < 2 * (uint64_t)n; d++) cycles |= dbg_rank_cut(next.get(), pd[cur].get(), mn[cur].get(), (uint32_t)d);
        if (cycles) n_rounds += rounds(n, pd, mn, cur);
        // the unitigs
        auto start = exact<uint32_t>(n), pos_flip = exact<uint32_t>(n), len = exact<uint32_t>(n), perm = exact<uint32_t>(n);
        for (uint32_t i = 0; i < n; i++) {
            const DbgPlace r = dbg_resolve(next.get(), pd[cur].get(), mn[cur].get(), i);
            start[i] = r.start < n ? r.start : i;
            pos_flip[i] = r.pos_flip;
            len[i] = r.len;
        }
        auto scan = exact<Scan>((uint64_t)n + 1);
        Scan run{0, 0};
        for (uint32_t i = 0; i <= n; i++) {
            scan[i] = run;
            if (i < n && len[i]) { run.units++; run.kmers += len[i] & ~DBG_CYCLE_BIT; }
        }
        n_unitigs = scan[n].units;
        for (uint32_t i = 0; i < n; i++) {
            const uint64_t at = scan[start[i]].kmers + (pos_flip[i] >> 1);
            if (at < n) perm[at] = (i << 1) | (pos_flip[i] & 1);
        }
        auto prefix = exact<uint64_t>((uint64_t)n + 1);
        uint64_t acc = 0;
        for (uint32_t j = 0; j <= n; j++) {
            prefix[j] = acc;
            if (j < n && (perm[j] >> 1) < n) acc += counts[perm[j] >> 1];
        }
        auto unitig_rows = exact<uint64_t>(4 * n_unitigs);
        for (uint32_t i = 0; i < n; i++) {
            kmer_rows[2 * (uint64_t)i] = (uint32_t)scan[start[i]].units;
            kmer_rows[2 * (uint64_t)i + 1] = pos_flip[i];
            if (!len[i] || scan[i].units >= n_unitigs) continue;
            const uint64_t L = len[i] & ~DBG_CYCLE_BIT;
            const uint64_t first = scan[i].kmers < n ? scan[i].kmers : n, end = first + L < n ? first + L : n;
            const uint32_t last = perm[end ? end - 1 : 0], li = (last >> 1) < n ? last >> 1 : i;
            uint64_t *row = unitig_rows.get() + 4 * scan[i].units;
            row[0] = i;
            row[1] = L;
            row[2] = prefix[end] - prefix[first];
            row[3] = dbg_row_flags((len[i] & DBG_CYCLE_BIT) != 0, edges[i], pos_flip[i] & 1, edges[li], last & 1);
        }
        // the spelling
        auto offsets = exact<uint64_t>(n_unitigs + 1);
        uint64_t total = 0;
        for (uint64_t u = 0; u <= n_unitigs; u++) {
            offsets[u] = total;
            if (u < n_unitigs) total += (unitig_rows[4 * u + 1] < n ? unitig_rows[4 * u + 1] : n) + k;
        }
        auto out = exact<uint8_t>(total);
        for (uint32_t i = 0; i < n; i++) {
            const uint32_t u = kmer_rows[2 * (uint64_t)i], pf = kmer_rows[2 * (uint64_t)i + 1];
            if (u >= n_unitigs) continue;
            const uint64_t L = unitig_rows[4 * (uint64_t)u + 1], pos = pf >> 1;
            if (pos >= L) continue;
            const uint64_t at = offsets[u] + pos, end = offsets[u + 1];
            const uint64_t x = keys[i] & dbg_mask(k), v = (pf & 1) ? dbg_rc(x, k) : x;
            if (pos + 1 < L) {
                if (at < end) out[at] = dbg_base(v, k, 0);
            } else if (at + k < end) {
                for (uint32_t j = 0; j < k; j++) out[at + j] = dbg_base(v, k, j);
                out[at + k] = (uint8_t)'\n';
            }
        }
        for (uint64_t u = 0; u < n_unitigs; u++) {
            char line[128];
            snprintf(line, sizeof line, "R %" PRIu64 " %" PRIu64 " %" PRIu64 " %" PRIu64 "\nS ", unitig_rows[4 * u], unitig_rows[4 * u + 1],
                     unitig_rows[4 * u + 2], unitig_rows[4 * u + 3]);
            rows_text += line;
            for (uint64_t p = offsets[u]; p + 1 < offsets[u + 1]; p++) rows_text += out[p] ? (char)out[p] : '?';
            rows_text += '\n';
        }
    }
    dbg_totals(sums, totals);
    printf("E");
    for (uint32_t i = 0; i < n; i++) printf(" %u", edges[i]);
    printf("\nT");
    for (uint32_t t = 0; t < DBG_N_TOTALS; t++) printf(" %" PRIu64, totals[t]);
    printf("\nK");
    for (uint64_t i = 0; i < 2 * (uint64_t)n; i++) printf(" %u", kmer_rows[i]);
    printf("\nU %" PRIu64 " %" PRIu64 " %" PRIu64 " %d\n%s", n_unitigs, n + n_unitigs * (k - 1), n_rounds, mates_ok ? 1 : 0, rows_text.c_str());
    return 0;
}

int main()
{
    uint32_t k = 0, n = 0;
    while (scanf("%u %u", &k, &n) == 2) {
        if (!dbg_k_ok(k) || n > DBG_N_MAX) return 2;
        auto keys = exact<uint64_t>(n), counts = exact<uint64_t>(n);
        for (uint32_t i = 0; i < n; i++)
            if (scanf("%" SCNx64 " %" SCNx64, &keys[i], &counts[i]) != 2) return 2;
        if (run_case(k, n, keys.get(), counts.get())) return 1;
    }
    return 0;
}
