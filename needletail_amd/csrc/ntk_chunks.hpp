// The chunk geometry of a batch that is materialised piece by piece (for_each_chunk of ntk_consumer.hpp walks it).  Plain C++ without
// any device call, so that it also compiles with g++: the CPU suite sweeps it against a restatement (tests/test_chunks.py).
//
// A batch of n_bytes is taken in chunks of kChunkBases.  Each chunk after the first is materialised from `halo` bytes before its start
// (a multiple of 16: d_seq stays aligned; >= k - 1: every window that ends in the chunk is whole), and only what ends at or after the
// start is taken: a window counts once, and the halo's partial windows never replace a good word of the chunk before.
#pragma once

#include <stdint.h>

namespace {

constexpr uint64_t kChunkBases = (uint64_t)64 << 20;     // bases materialised per pass (scratch: 10 B per base)

struct Chunk {
    uint64_t start, end;   // the window ends [start, end) are this chunk's
    uint64_t base;         // materialised from here: 0, or start - halo
    uint64_t len() const { return end - base; }      // bytes materialised
    uint64_t skip() const { return start - base; }   // of which the halo
};

inline uint64_t chunk_halo(uint32_t k) { return ((uint64_t)k - 1 + 15) & ~(uint64_t)15; }

// the window ends of the longest chunk
inline uint64_t chunk_bases(uint64_t n_bytes) { return n_bytes < kChunkBases ? n_bytes : kChunkBases; }

// the bytes materialised for the longest chunk: what the scratch must hold
inline uint64_t chunk_scratch_bases(uint64_t n_bytes, uint32_t k) { return chunk_bases(n_bytes) + (n_bytes > kChunkBases ? chunk_halo(k) : 0); }

// the chunk that starts at `start` (a multiple of kChunkBases below n_bytes)
inline Chunk chunk_at(uint64_t n_bytes, uint32_t k, uint64_t start)
{
    const uint64_t end = n_bytes - start > kChunkBases ? start + kChunkBases : n_bytes;
    return Chunk{start, end, start ? start - chunk_halo(k) : 0};
}

}  // namespace
