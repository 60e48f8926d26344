// The chunk cut of the batched Sequence-trait calls (run_banked of ntk_api.hip walks it) and the constants of their pipeline.  Plain C++
// without any device call, so that it also compiles with g++: the CPU suite sweeps the cutter against a restatement
// (tests/test_compat_plan.py).
#pragma once

#include <stdint.h>

namespace {

constexpr uint64_t kCompatChunkBytes = (uint64_t)16 << 20;   // NTK_OPT_COMPAT_CHUNK_BYTES by default: bytes per chunk
constexpr uint64_t kCompatChunkMin = 64;                     // ... and the least it is set to (a stray 1 would cost a launch and an event wait per record)
constexpr int kCompatBanks = 3;                              // chunks in flight
constexpr uint64_t kLongRecord = (uint64_t)1 << 16;          // ntk_minimizer_batch: longer records go to the one-block kernel

// records [r0, r1) of a batch and the bytes they cost
struct CompatCut {
    uint64_t r0, r1, bytes;
    uint64_t nrec() const { return r1 - r0; }
};

// The chunk that starts at record r0 < n_records: as many records as fit chunk_bytes, and one at the least.  A record costs its own bytes
// plus per_record: 1 where the records are packed with a break byte behind each (the item arrays), 0 where they are uploaded as they lie.
inline CompatCut compat_cut(const uint64_t *offsets, uint64_t n_records, uint64_t r0, uint64_t chunk_bytes, uint64_t per_record)
{
    uint64_t r1 = r0 + 1;
    while (r1 < n_records && offsets[r1 + 1] - offsets[r0] + per_record * (r1 + 1 - r0) <= chunk_bytes) r1++;
    return CompatCut{r0, r1, offsets[r1] - offsets[r0] + per_record * (r1 - r0)};
}

}  // namespace
