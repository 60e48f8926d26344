// ntk_plan.hpp — the launch arithmetic of a tile scan (ntk_api.hip launch_tile_scan), host only and free of HIP so that a CPU test can
// include it (tests/emu/emu_exact.cpp).  A scan covers the window ends [0, n) with tiles of `stride` bytes - tile t owns the ends in
// [t stride, (t + 1) stride); the stride is the kernel build's own (ntk_tile.hpp: Sv2Geom<..>::kStride for the scan2 builds, kTileStride for
// scan_kernel, (64 - min_halo_lanes) * 16 for minimizer_scan_kernel) - in launches of at most kMaxTilesPerLaunch tiles.
#pragma once
#include <stdint.h>

namespace ntk {

constexpr int kMaxShards = 256;      // work counters: the pull atomics of > 6000 waves on 8 counters were the bottleneck (profiles/r02)
// a launch of a tile scan covers at most this many tiles, a shard <= 2^22 of them, so that the per-block u32 histogram cells (a block can at
// most drain its whole shard: 2^22 * 1008 windows), the u32 work counters and 32-bit buffer offsets cannot overflow
constexpr uint64_t kMaxTilesPerLaunch = (uint64_t)8 << 22;

inline uint64_t tile_count(uint64_t n, uint64_t stride) { return (n + stride - 1) / stride; }

struct LaunchPlan {
    uint64_t tile_begin, tile_end;   // the launch covers tiles [tile_begin, tile_end)
    uint32_t chunk_tiles;            // tiles per pull
    uint32_t blocks;                 // grid
    uint32_t n_shards;               // work counters in use: block b pulls from shard b % n_shards
    uint32_t tiles_per_shard;
    uint32_t tail_tile_rel;          // first tile, relative to tile_begin, that touches byte n or later; 0xFFFFFFFF: none in this launch
};

// The launch that starts at tile `tile_begin` (a multiple of kMaxTilesPerLaunch below tile_count(n, stride)).  blocks_max: the blocks that are
// resident at once (work is pulled: more only write empty histograms); max_chunk: cap on the tiles per pull.
inline LaunchPlan plan_launch(uint64_t n, uint64_t stride, uint64_t tile_begin, uint64_t blocks_max, uint64_t waves_per_block, uint64_t max_chunk)
{
    LaunchPlan p;
    const uint64_t n_tiles = tile_count(n, stride);
    p.tile_begin = tile_begin;
    p.tile_end = tile_begin + kMaxTilesPerLaunch < n_tiles ? tile_begin + kMaxTilesPerLaunch : n_tiles;
    const uint64_t tiles = p.tile_end - p.tile_begin;
    uint64_t chunk = tiles / (blocks_max * waves_per_block * 4);  // >= ~4 pulls per wave, <= max_chunk tiles each (8..32 are within 1 %: profiles/r02c)
    chunk = chunk < 1 ? 1 : (chunk > max_chunk ? max_chunk : chunk);
    const uint64_t want_blocks = (tiles + chunk * waves_per_block - 1) / (chunk * waves_per_block);
    p.blocks = (uint32_t)(want_blocks < blocks_max ? want_blocks : blocks_max);
    p.chunk_tiles = (uint32_t)chunk;
    p.n_shards = p.blocks < (uint32_t)kMaxShards ? (p.blocks ? p.blocks : 1u) : (uint32_t)kMaxShards;   // (no blocks: n = 0, nothing is launched)
    p.tiles_per_shard = (uint32_t)((tiles + p.n_shards - 1) / p.n_shards);
    const uint64_t first_tail = n / stride;   // tiles t with (t + 1) * stride > n touch the end of the input
    p.tail_tile_rel = first_tail < tile_begin ? 0u : (first_tail - tile_begin > 0xFFFFFFFEull ? 0xFFFFFFFFu : (uint32_t)(first_tail - tile_begin));
    return p;
}

}  // namespace ntk
