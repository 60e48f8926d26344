// The rule of the alignment library (needletail_amd/csrc/ntk_align_rule.hpp) as a stand-alone program for tests/test_align_rule.py, which
// compiles it with g++ -fsanitize=address,undefined.  Every input line is one between part: a b q e band_pad n m, then n reference codes
// and m query codes; the answer is H[n][m], the cells in band, the number of runs and the runs, first to last.
//   segment  aln_segment_host: the header's cell, band, storage and traceback functions under a row-major loop
//   sweep    the same functions under the DP kernel's order, restated lane by lane: strips of 64 rows, lane l of a strip at column
//            j_lo + t - l at step t, its upper neighbours what lane l - 1 left one and two steps earlier, the row above a strip in an array
#include "../needletail_amd/csrc/ntk_align_rule.hpp"

#include <cstdio>
#include <cstring>
#include <iostream>
#include <vector>

static std::vector<uint32_t> sweep(const uint8_t *ref, uint32_t n_, const uint8_t *qry, uint32_t m_, const aln_rule_params &p, int32_t *score,
                                   uint64_t *cells)
{
    const int32_t n = (int32_t)n_, m = (int32_t)m_;
    int32_t lo, hi;
    aln_band(n_, m_, p.band_pad, lo, hi);
    const uint32_t width = aln_row_width(m_, lo, hi);
    std::vector<uint8_t> dir((uint64_t)n * width, 0xFF);
    std::vector<int32_t> s_h(m + 1, 12345), s_e(m + 1, 12345);   // (stale words: only cells the strip above wrote may be read)
    *cells = 0;
    *score = ALN_NEG;
    for (int32_t i0 = 1; i0 <= n; i0 += 64) {
        const int32_t last_row = i0 + 63 < n ? i0 + 63 : n;
        const int32_t j_lo = i0 + lo > 1 ? i0 + lo : 1, j_hi = last_row + hi < m ? last_row + hi : m;
        const int32_t steps = j_hi - j_lo + 64;
        int32_t h_left[64], f_left[64], h_diag[64], h_out[64], e_out[64];
        uint32_t q_out[64], q_block[64];
        for (int l = 0; l < 64; l++) { h_left[l] = f_left[l] = h_diag[l] = h_out[l] = e_out[l] = ALN_NEG; q_out[l] = q_block[l] = 4; }
        for (int32_t t = 0; t < steps; t++) {
            if ((t & 63) == 0)
                for (int l = 0; l < 64; l++) {
                    const int32_t col = j_lo + t + l;
                    q_block[l] = col <= m ? qry[col - 1] : 4;
                }
            int32_t h_new[64], e_new[64];
            uint32_t q_new[64];
            for (int l = 0; l < 64; l++) {
                const int32_t i = i0 + l, j = j_lo + t - l;
                const bool row = i <= n;
                const int32_t my_first = i + lo > 1 ? i + lo : 1, my_last = i + hi < m ? i + hi : m;
                int32_t h_up = l ? h_out[l - 1] : ALN_NEG, e_up = l ? e_out[l - 1] : ALN_NEG;
                uint32_t q_code = l ? q_out[l - 1] : 4;
                if (l == 0) {
                    q_code = q_block[t & 63];
                    const bool above = j <= m && aln_in_band(i0 - 1, j, lo, hi), above_left = j - 1 <= m && aln_in_band(i0 - 1, j - 1, lo, hi);
                    if (i0 == 1) {
                        h_up = j <= m ? aln_border_h(0, j, lo, hi, p.q, p.e) : ALN_NEG;
                        e_up = ALN_NEG;
                        h_diag[0] = aln_border_h(0, j - 1, lo, hi, p.q, p.e);
                    } else {
                        h_up = above ? s_h[j] : ALN_NEG;
                        e_up = above ? s_e[j] : ALN_NEG;
                        h_diag[0] = j == 1 ? aln_border_h(i0 - 1, 0, lo, hi, p.q, p.e) : above_left ? s_h[j - 1] : ALN_NEG;
                    }
                }
                const bool active = row && j >= my_first && j <= my_last;
                h_new[l] = e_new[l] = ALN_NEG;
                if (active) {
                    if (j == 1) {
                        h_left[l] = aln_border_h(i, 0, lo, hi, p.q, p.e);
                        f_left[l] = ALN_NEG;
                        if (l != 0) h_diag[l] = aln_border_h(i - 1, 0, lo, hi, p.q, p.e);
                    }
                    int32_t h, ee, f;
                    const uint32_t d = aln_cell(h_diag[l], h_up, e_up, h_left[l], f_left[l], aln_match(ref[i - 1], q_code), p.a, p.b, p.q, p.e, h, ee, f);
                    dir[aln_dir_at(i, j, m_, lo, width)] = (uint8_t)d;
                    ++*cells;
                    h_left[l] = h; f_left[l] = f; h_new[l] = h; e_new[l] = ee;
                    if (i == n && j == m) *score = h;
                } else {
                    h_left[l] = f_left[l] = ALN_NEG;
                }
                h_diag[l] = h_up;
                q_new[l] = q_code;
            }
            // (lane 63 writes the row for the strip below behind lane 0's reads of this step, as in the kernel)
            {
                const int32_t j = j_lo + t - 63, i = i0 + 63;
                if (i <= n && j >= (i + lo > 1 ? i + lo : 1) && j <= (i + hi < m ? i + hi : m)) { s_h[j] = h_new[63]; s_e[j] = e_new[63]; }
            }
            memcpy(h_out, h_new, sizeof h_out); memcpy(e_out, e_new, sizeof e_out); memcpy(q_out, q_new, sizeof q_out);
        }
    }
    std::vector<uint32_t> runs(n_ + m_);
    runs.resize(aln_trace(dir.data(), n_, m_, lo, hi, width, runs.data()));
    return std::vector<uint32_t>(runs.rbegin(), runs.rend());
}

int main(int argc, char **argv)
{
    if (argc != 2) return 2;
    const bool by_sweep = !strcmp(argv[1], "sweep");
    if (!by_sweep && strcmp(argv[1], "segment")) return 2;
    aln_rule_params p = {};
    uint32_t n, m;
    while (std::cin >> p.a >> p.b >> p.q >> p.e >> p.band_pad >> n >> m) {
        std::vector<uint8_t> ref(n), qry(m);
        for (auto *v : {&ref, &qry})
            for (auto &c : *v) { unsigned x; std::cin >> x; c = (uint8_t)x; }
        int32_t score;
        uint64_t cells;
        const std::vector<uint32_t> runs = (by_sweep ? sweep : aln_segment_host)(ref.data(), n, qry.data(), m, p, &score, &cells);
        printf("%d %llu %zu", score, (unsigned long long)cells, runs.size());
        for (uint32_t r : runs) printf(" %u", r);
        printf("\n");
    }
    // the codes, the complement and the query of the reverse strand
    if (aln_code('a') != 0 || aln_code('C') != 1 || aln_code('g') != 2 || aln_code('T') != 3 || aln_code('u') != 3 || aln_code('U') != 3) return 1;
    if (aln_code('N') != 4 || aln_code('\n') != 4 || aln_code(0) != 4 || aln_code(0xE1) != 4 || aln_comp(4) != 4 || aln_comp(0) != 3 || aln_comp(2) != 1) return 1;
    const uint8_t read[] = "ACGNT";
    const uint32_t reverse[] = {0, 4, 1, 2, 3}, forward[] = {0, 1, 2, 4, 3};
    for (uint64_t x = 0; x < 5; x++)
        if (aln_query_code(read, 5, 1, x) != reverse[x] || aln_query_code(read, 5, 0, x) != forward[x]) return 1;
    if (aln_record_len(5, 5) != 0 || aln_record_len(5, 6) != 0 || aln_record_len(5, 9) != 3) return 1;
    return 0;
}
