// emu_exact.cpp — TEST-ONLY: the lock-step wave emulation of emu_scan.cpp run in the tile geometry the k-mer builds of scan2_kernel use
// (ntk_tile.hpp Sv2Geom<K, true>: a tile advances by every byte whose windows lie inside it) and over the tiles the host planner hands out
// (csrc/ntk_plan.hpp), plus the planner itself for the CPU test of its arithmetic.  emu_scan.cpp's own run_sv2 keeps the whole-halo-lane
// geometry, which the fused-minimizer builds still have.
#include "emu_scan.cpp"
#include "../../needletail_amd/csrc/ntk_plan.hpp"

namespace {

// scan2_kernel<K, TIE_RC, ACCEPT_U, QM, HB, 0, FWD> tile by tile: tile t of the launch plan loads the bytes [t kStride - kHaloBytes, + 1024)
// and is a tail tile from the plan's tail_tile_rel on.  Quality builds: g_qual / g_qc as in emu_scan.cpp.
template <bool TIE_RC, bool ACCEPT_U, int K, int HB, bool FWD>
void run_sv2_exact(const uint8_t *buf, uint64_t n, uint64_t n_padded, HostStats *st)
{
    using Geo = Sv2Geom<K, true>;
    const uint64_t n_tiles = tile_count(n, Geo::kStride);
    EmuMP2<K, HB> mp;
    EmuNoSink sink;
    for (uint64_t tb = 0; tb < n_tiles; tb += kMaxTilesPerLaunch) {
        const LaunchPlan lp = plan_launch(n, Geo::kStride, tb, 512, 12, 24);
        for (uint64_t t = lp.tile_begin; t < lp.tile_end; t++) {
            const bool tail = t - lp.tile_begin >= lp.tail_tile_rel;
            EncSV2 en[64];
            uint64_t G[16] = {0};
            for (int l = 0; l < 64; l++) {
                const int64_t lane_base = (int64_t)(t * Geo::kStride) - Geo::kHaloBytes + l * 16;
                en[l] = encode16_sv2<ACCEPT_U>(load16q(buf, n_padded, lane_base));
                for (int i = 0; i < 16; i++) {
                    bool good = !sv2_base_is_break(en[l], i);
                    if (tail && lane_base + i >= (int64_t)n) good = false;
                    if (good) G[i] |= 1ull << l;
                }
            }
            window_masks_ab_any<K, true>(G, mp.VA, mp.VB);
            mp.tie_rc = TIE_RC;
            EmuXL xl;
            for (int l = 0; l < 64; l++) {
                xl.next_lane(l == 0);
                mp.lane = l;
                if constexpr (K <= 16) lane_tile_sv2w<TIE_RC, K, FWD>(sink, xl, mp, en[l].code, en[l].rcode);
                else if constexpr (FWD) lane_tile_sv2_fwd<K>(sink, xl, mp, en[l].code);
                else lane_tile_sv2<TIE_RC, K>(sink, xl, mp, en[l].code, en[l].rcode);
            }
        }
    }
    mp.finish(st);
}

template <int K>
void run_exact_k(const uint8_t *buf, uint64_t n, uint64_t n_padded, int canon, int tie_rc, int accept_u, HostStats *st)
{
    constexpr int HB = 14;   // the shipped histogram (ntk_scan2.hip kScan2HistBits)
    if (!canon) { if (accept_u) run_sv2_exact<false, true, K, HB, true>(buf, n, n_padded, st); else run_sv2_exact<false, false, K, HB, true>(buf, n, n_padded, st); }
    else if (tie_rc) { if (accept_u) run_sv2_exact<true, true, K, HB, false>(buf, n, n_padded, st); else run_sv2_exact<true, false, K, HB, false>(buf, n, n_padded, st); }
    else { if (accept_u) run_sv2_exact<false, true, K, HB, false>(buf, n, n_padded, st); else run_sv2_exact<false, false, K, HB, false>(buf, n, n_padded, st); }
}

}  // namespace

extern "C" {

// The tile stride of the k-mer build of k, 0 on bad k.
uint32_t emu_exact_stride(uint32_t k) { return k >= 1 && k <= 32 ? (uint32_t)sv2_stride_bytes((int)k, true) : 0u; }

// out: [n_total, n_fwd, sum, xor, hist[4096]] of scan2_kernel's k-mer build for (k, canon, tie_rc, accept_u); qual != null: the quality build
// with bases below `cutoff` (1..255) masked.  Returns 0, -1 on a bad argument.
int emu_scan_exact(const uint8_t *buf, const uint8_t *qual, uint32_t cutoff, uint64_t n, uint64_t n_padded, uint32_t k, int canon, int tie_rc,
                   int accept_u, uint64_t *out)
{
    if (k < 1 || k > 32 || (qual && (cutoff < 1 || cutoff > 255))) return -1;
    HostStats *st = new HostStats();
    if (qual) { g_qual = qual; g_qc = quality_cut(cutoff); }
    switch (k) {
#define EMU_XK(KF) case KF: run_exact_k<KF>(buf, n, n_padded, canon, tie_rc, accept_u, st); break;
    EMU_XK(1) EMU_XK(2) EMU_XK(3) EMU_XK(4) EMU_XK(5) EMU_XK(6) EMU_XK(7) EMU_XK(8) EMU_XK(9) EMU_XK(10) EMU_XK(11) EMU_XK(12) EMU_XK(13)
    EMU_XK(14) EMU_XK(15) EMU_XK(16) EMU_XK(17) EMU_XK(18) EMU_XK(19) EMU_XK(20) EMU_XK(21) EMU_XK(22) EMU_XK(23) EMU_XK(24) EMU_XK(25)
    EMU_XK(26) EMU_XK(27) EMU_XK(28) EMU_XK(29) EMU_XK(30) EMU_XK(31) EMU_XK(32)
#undef EMU_XK
    }
    g_qual = nullptr;
    out[0] = st->n_total; out[1] = st->n_fwd; out[2] = st->sum; out[3] = st->xr;
    memcpy(out + 4, st->hist, sizeof(st->hist));
    delete st;
    return 0;
}

// plan_launch (csrc/ntk_plan.hpp) as the library calls it.  out: [tile_count, tile_begin, tile_end, chunk_tiles, blocks, n_shards,
// tiles_per_shard, tail_tile_rel, kMaxTilesPerLaunch, kMaxShards].
void emu_plan_launch(uint64_t n, uint64_t stride, uint64_t tile_begin, uint64_t blocks_max, uint64_t waves_per_block, uint64_t max_chunk, uint64_t *out)
{
    const LaunchPlan p = plan_launch(n, stride, tile_begin, blocks_max, waves_per_block, max_chunk);
    out[0] = tile_count(n, stride); out[1] = p.tile_begin; out[2] = p.tile_end; out[3] = p.chunk_tiles; out[4] = p.blocks; out[5] = p.n_shards;
    out[6] = p.tiles_per_shard; out[7] = p.tail_tile_rel; out[8] = kMaxTilesPerLaunch; out[9] = (uint64_t)kMaxShards;
}

// Which window ends the tile-local masks let a tile of the k-mer build of k emit when every byte is a base: emits[p] = 1 for tile byte
// p = 16 lane + j.  A tile must emit exactly its last kStride bytes.  Returns 0, -1 on bad k.
int emu_exact_emits(uint32_t k, uint8_t *emits)
{
    uint64_t G[16], A[16], B[16];
    for (int i = 0; i < 16; i++) G[i] = ~0ull;
    switch (k) {
#define EMU_XE(KF) case KF: window_masks_ab_any<KF, true>(G, A, B); break;
    EMU_XE(1) EMU_XE(2) EMU_XE(3) EMU_XE(4) EMU_XE(5) EMU_XE(6) EMU_XE(7) EMU_XE(8) EMU_XE(9) EMU_XE(10) EMU_XE(11) EMU_XE(12) EMU_XE(13)
    EMU_XE(14) EMU_XE(15) EMU_XE(16) EMU_XE(17) EMU_XE(18) EMU_XE(19) EMU_XE(20) EMU_XE(21) EMU_XE(22) EMU_XE(23) EMU_XE(24) EMU_XE(25)
    EMU_XE(26) EMU_XE(27) EMU_XE(28) EMU_XE(29) EMU_XE(30) EMU_XE(31) EMU_XE(32)
#undef EMU_XE
    default: return -1;
    }
    for (int l = 0; l < 64; l++)
        for (int j = 0; j < 16; j++) emits[16 * l + j] = (uint8_t)(((A[j] & B[j]) >> l) & 1);
    return 0;
}

}  // extern "C"
