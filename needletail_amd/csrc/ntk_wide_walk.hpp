// The byte walk of two-word keys (k = 33..63), for libraries that hand every canonical key of a device batch to a functor.
//
// This is wt_count_kernel's walk (ntk_wide_count.hip): the same lane geometry and the same base, break and quality rules.  That kernel
// keeps its own inline copy - sharing the walker changed its schedule, and the kernel set of its library is
// pinned - so there is one header, and wt_count_kernel's own: the sketch (ntk_sketch.hip) and the MinHash library (ntk_minhash.hip)
// include this one, and tests/test_minhash_abi.py holds its constants and per-byte rules to ntk_wide_count.hip.
#pragma once

#include <hip/hip_runtime.h>

#include <cstdint>

namespace {

constexpr uint32_t kKMax = 63;
constexpr uint32_t kLaneRun = 64;                        // window ends per lane, as wt_count_kernel
constexpr uint32_t kPrime = 64;                          // bytes each lane reads before its first end (>= kKMax - 1, a multiple of 16)

static_assert(kPrime >= kKMax - 1 && kPrime % 16 == 0 && kLaneRun % 16 == 0, "lane geometry");

// The lane owns the window ends [first_end, first_end + kRun): it reads the kLead bytes before its first end (kLead >= k - 1, a
// multiple of 16) and its own kRun bytes in 16-byte loads, rolls the forward and reverse-complement words (two u64 each: hi = the
// first k - 32 bases, lo = the last 32) over all of them, and calls emit(hi, lo) with min(forward, reverse complement) of every window
// that ends in its run after k base bytes in a row.  Bases are ACGTacgtUu with a quality byte >= cutoff (qual == nullptr: no mask).
// A load is issued only for a 16-byte block that starts in [0, n_bytes) (the layout makes round_up(n_bytes, 16) readable), and a byte
// at or past n_bytes is a break.
template <uint32_t kRun, uint32_t kLead, class Emit>
__device__ __forceinline__ void walk_lane_run(const uint8_t *seq, const uint8_t *qual, uint64_t n_bytes, uint32_t k, uint32_t cutoff,
                                              uint64_t first_end, Emit emit)
{
    static_assert(kLead % 16 == 0 && kRun % 16 == 0, "lane geometry");
    const uint32_t hi_bits = 2 * k - 64, rc_shift = 2 * k - 66;
    const uint64_t hi_mask = ((uint64_t)1 << hi_bits) - 1;
    uint64_t fh = 0, fl = 0, rh = 0, rl = 0;
    uint32_t run = 0;
#pragma unroll 1
    for (uint32_t blk = 0; blk < (kLead + kRun) / 16; blk++) {
        // 16 bytes starting at first_end - kLead + 16 * blk (before 0 or at / past n_bytes: breaks)
        const uint64_t at = first_end + 16 * blk;   // = the block's start + kLead
        uint4 s = make_uint4(0, 0, 0, 0), q = make_uint4(~0u, ~0u, ~0u, ~0u);
        if (at >= kLead && at - kLead < n_bytes) {
            s = *reinterpret_cast<const uint4 *>(seq + (at - kLead));
            if (qual) q = *reinterpret_cast<const uint4 *>(qual + (at - kLead));
        }
#pragma unroll 1
        for (uint32_t j = 0; j < 16; j++) {
            const uint32_t b = s.x & 0xFF, qb = q.x & 0xFF;
            s.x = (s.x >> 8) | (s.y << 24); s.y = (s.y >> 8) | (s.z << 24); s.z = (s.z >> 8) | (s.w << 24); s.w >>= 8;
            q.x = (q.x >> 8) | (q.y << 24); q.y = (q.y >> 8) | (q.z << 24); q.z = (q.z >> 8) | (q.w << 24); q.w >>= 8;
            const uint64_t pos_plus = at + j;   // the byte's position + kLead
            const uint32_t l = b | 0x20;        // ACGTU / acgtu -> lower case
            const bool base = (l == 'a' || l == 'c' || l == 'g' || l == 't' || l == 'u') && qb >= cutoff && pos_plus - kLead < n_bytes;
            const uint64_t c = ((b >> 1) ^ (b >> 2)) & 3;   // A 0, C 1, G 2, T / U 3 in either case
            fh = ((fh << 2) | (fl >> 62)) & hi_mask;
            fl = (fl << 2) | c;
            rl = (rl >> 2) | (rh << 62);
            rh = (rh >> 2) | ((3 - c) << rc_shift);
            run = base ? run + 1 : 0;
            if (run >= k && pos_plus >= first_end + kLead) {
                const bool fwd = fh < rh || (fh == rh && fl <= rl);
                emit(fwd ? fh : rh, fwd ? fl : rl);
            }
        }
    }
}

}  // namespace
