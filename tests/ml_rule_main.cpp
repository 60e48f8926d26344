// The rule of the minimizer-list library (needletail_amd/csrc/ntk_ml_rule.hpp) on the CPU, step by step as ml_select_kernel and
// ml_scatter_kernel of ntk_minimizer_list.hip take it: the window ends are cut into tiles, a tile is staged with the w ends in front of
// it as (key, slot) pairs, doubled level by level (every slot's new pair is computed before any is written, as the kernel's registers
// hold them across the barrier), every window taken as two overlapping ranges, and the word of every end written; the span of an opening
// end is then read from the words behind it.  tests/test_ml_rule.py holds what it prints to a model written from the definition; the
// same program is built with -fsanitize=address,undefined.
//
//   ml_rule sweep TILE     every array of length 1..9 over the keys 0, 1, 2 and "not valid", for w = 1..9, in the order
//                          w, length, code (symbol i of an array = (code >> 2 i) & 3, 3 = not valid); per window end two bytes,
//                          little endian: the end's word | span << 12 (span 0 where no entry opens)
//   ml_rule                cases on stdin, "order w tile n" and then n tokens (a hex VALUE, or - for an end that is not valid); per
//                          case one line of n hex numbers: word | span << 16
#include "../needletail_amd/csrc/ntk_ml_rule.hpp"

#include <cinttypes>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

// the words of n window ends (the chunk's base is end 0, its limit n)
static void select(const std::vector<uint64_t> &key, const std::vector<char> &valid, uint32_t w, uint32_t tile, std::vector<uint32_t> &sel)
{
    const uint64_t n_ends = key.size();
    const uint32_t top = ml_top_q(w);
    std::vector<MlPair> m(w + tile), next(w + tile), win(w + tile);
    auto range = [&](uint32_t i) { return m[i]; };
    for (uint64_t t0 = 0; t0 < n_ends; t0 += tile) {
        const uint32_t own = n_ends - t0 < tile ? (uint32_t)(n_ends - t0) : tile, n = w + own;
        for (uint32_t i = 0; i < n; i++) {
            const bool behind = t0 + i >= w;
            const uint64_t at = behind ? t0 + i - w : 0;
            const bool ok = behind && valid[at];
            m[i] = ml_pair(ok ? key[at] : 0, i, ok);
        }
        for (uint32_t q = 1; q < top; q *= 2) {
            for (uint32_t i = 0; i < n; i++) next[i] = ml_double_at(range, i, q);
            for (uint32_t i = 0; i < n; i++) m[i] = next[i];
        }
        for (uint32_t i = 0; i < n; i++)
            if (i + 1 >= w) win[i] = MlPair{0, ml_window_at(range, i, w, top).pos};
        for (uint32_t i = w; i < n; i++) sel[t0 + i - w] = ml_sel_word(i, win[i - 1], win[i]);
    }
}

static uint32_t span_at(const std::vector<uint32_t> &sel, uint64_t x, uint32_t w)
{
    if (!(sel[x] & ML_SEL_OPEN)) return 0;
    return ml_span([&](uint64_t y) { return sel[y]; }, x, sel.size(), w);
}

static int sweep(uint32_t tile)
{
    std::vector<unsigned char> out;
    for (uint32_t w = 1; w <= 9; w++)
        for (uint32_t len = 1; len <= 9; len++) {
            std::vector<uint64_t> key(len);
            std::vector<char> valid(len);
            std::vector<uint32_t> sel(len);
            out.clear();
            for (uint32_t code = 0; code < (1u << 2 * len); code++) {
                for (uint32_t i = 0; i < len; i++) {
                    const uint32_t s = (code >> 2 * i) & 3;
                    valid[i] = s != 3;
                    key[i] = s == 3 ? 0 : s;
                }
                select(key, valid, w, tile, sel);
                for (uint32_t i = 0; i < len; i++) {
                    const uint32_t v = sel[i] | span_at(sel, i, w) << 12;
                    out.push_back((unsigned char)(v & 0xFF));
                    out.push_back((unsigned char)(v >> 8));
                }
            }
            if (fwrite(out.data(), 1, out.size(), stdout) != out.size()) return 2;
        }
    return 0;
}

int main(int argc, char **argv)
{
    if (argc == 3 && strcmp(argv[1], "sweep") == 0) return sweep((uint32_t)atoi(argv[2]));
    uint32_t order, w, tile;
    uint64_t n;
    while (scanf("%u %u %u %" SCNu64, &order, &w, &tile, &n) == 4) {
        if (w < 1 || w > ML_W_MAX || tile < 1 || tile > ML_TILE) return 2;
        std::vector<uint64_t> key(n);
        std::vector<char> valid(n);
        for (uint64_t i = 0; i < n; i++) {
            char tok[64];
            if (scanf("%63s", tok) != 1) return 2;
            valid[i] = strcmp(tok, "-") != 0;
            key[i] = valid[i] ? ml_key(order, strtoull(tok, nullptr, 16)) : 0;
        }
        std::vector<uint32_t> sel(n);
        select(key, valid, w, tile, sel);
        for (uint64_t i = 0; i < n; i++) printf("%s%" PRIx32, i ? " " : "", sel[i] | span_at(sel, i, w) << 16);
        printf("\n");
    }
    return 0;
}
