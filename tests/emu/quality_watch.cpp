// quality_watch.cpp — TEST-ONLY host build of the quality mask and of the speculative kernels' bit-5 watch on masked bytes
// (needletail_amd/csrc/ntk_tile.hpp: quality_cut, quality_break16, lower_watch_or, lower_watch16, or_of_input_bytes), the same source the
// HIP kernels compile.  tests/test_quality_watch.py runs it and checks every (byte, quality) pair at every cutoff against a Python model.
//
// Output on stdout, per cutoff 1..255, in that order:
//   65536 bytes  quality_break16 of the pairs in the order of perm() (byte = pair >> 8, quality = pair & 255), 16 bytes per line
//   65536 bytes  lower_watch16 of those lines (bit 5 of a byte: the byte is watched)
//    4096 bytes  per 16-byte line: 1 if lower_watch_or over its four dwords left bit 5 set in some byte, else 0
//    4096 bytes  per 16-byte line: 1 if or_of_input_bytes(lower_watch16(line), line % 17) has bit 5 set in some byte, else 0
#include <cstdint>
#include <cstdio>
#include <vector>

#include "../../needletail_amd/csrc/ntk_tile.hpp"

using namespace ntk;

// a permutation of the 65536 pairs, so that the bytes sharing a dword are unrelated pairs
static uint32_t perm(uint32_t i) { return (i * 40503u + 12345u) & 0xFFFFu; }

int main()
{
    std::vector<uint8_t> seq(65536), qual(65536), out(65536 * 2 + 4096 * 2);
    for (uint32_t i = 0; i < 65536; i++) { seq[i] = (uint8_t)(perm(i) >> 8); qual[i] = (uint8_t)perm(i); }
    auto word = [](const uint8_t *p) { return (uint32_t)p[0] | (uint32_t)p[1] << 8 | (uint32_t)p[2] << 16 | (uint32_t)p[3] << 24; };
    auto put = [](uint8_t *p, uint32_t w) { for (int b = 0; b < 4; b++) p[b] = (uint8_t)(w >> (8 * b)); };
    for (uint32_t cutoff = 1; cutoff <= 255; cutoff++) {
        const QualityCut qc = quality_cut(cutoff);
        for (uint32_t line = 0; line < 4096; line++) {
            const uint8_t *s = &seq[16 * line], *q = &qual[16 * line];
            const Raw16 m = quality_break16(Raw16{word(s), word(s + 4), word(s + 8), word(s + 12)},
                                            Raw16{word(q), word(q + 4), word(q + 8), word(q + 12)}, qc.add, qc.sel);
            const Raw16 w = lower_watch16(m);
            put(&out[16 * line], m.x); put(&out[16 * line + 4], m.y); put(&out[16 * line + 8], m.z); put(&out[16 * line + 12], m.w);
            put(&out[65536 + 16 * line], w.x); put(&out[65536 + 16 * line + 4], w.y);
            put(&out[65536 + 16 * line + 8], w.z); put(&out[65536 + 16 * line + 12], w.w);
            const uint32_t lc = lower_watch_or(lower_watch_or(lower_watch_or(lower_watch_or(0u, m.x), m.y), m.z), m.w);
            out[131072 + line] = (lc & 0x20202020u) != 0u;
            out[131072 + 4096 + line] = (or_of_input_bytes(w, (int64_t)(line % 17)) & 0x20202020u) != 0u;
        }
        if (fwrite(out.data(), 1, out.size(), stdout) != out.size()) return 1;
    }
    return 0;
}
