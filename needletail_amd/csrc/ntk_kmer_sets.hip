// Exact set algebra and joint spectra of two k-mer lists (include/needletail_amd_kmer_sets.h).  A consumer of the core's public ABI like
// the other libraries (it takes the context's device and stream and nothing else), and of no other library: it works on the format the
// count tables' extract writes and never touches a table.
//
// Both calls are one streaming merge-join (ntk_kset_rule.hpp has the rule and every per-element step).  ks_split_kernel cuts the merged
// order into tiles of kTileOf<KW> elements, one binary search per tile boundary.  ks_join_kernel's blocks take tiles grid-stride: a block
// stages the tile's keys of both lists with one look-behind and one look-ahead element in LDS (the loads coalesced and all issued
// before the first is used), and every element takes its bounded search there.  Counts are read from global memory by index, and only
// where the output needs them.  COMPARE adds into the block's LDS bins and keeps the sums in registers; at the end of the block's last
// tile the sums go through wave_sum and LDS, and every sum and every non-zero bin is flushed with one agent-scope add.  COUNT writes the
// number of kept elements per tile; after rocPRIM's exclusive scan WRITE parks each kept element at its merged slot in LDS and stores
// the slots in order: a slot's rank is a ballot's popcount prefix within the wave plus the wave's carry.  DESIGN.md section 19.
#include "../../include/needletail_amd_kmer_sets.h"
#include "ntk_consumer.hpp"
#include "ntk_kset_rule.hpp"

#include <rocprim/device/device_scan.hpp>

#include <cstring>
#include <new>

namespace {

constexpr uint32_t kTileWords = 2048;                  // key words of a tile: 16 KiB of LDS whatever the key width
template <int KW>
constexpr uint32_t kTileOf = kTileWords / KW;          // merged elements of a tile: 2048 narrow keys, 1024 wide ones
constexpr uint32_t kWaves = kThreads / 64;
constexpr uint32_t kBinsSmall = 4096, kBinsBig = 16384;   // the two builds of COMPARE: 16 KiB and 64 KiB of LDS bins
constexpr uint64_t kMaxTilesPerBlock = (uint64_t)1 << 20; // at most 2^31 elements per block: a block's u32 bins cannot overflow
constexpr unsigned kBlocksPerCu = 4;
constexpr uint64_t kMinTilesPerBlock = 2;                 // a block's fixed cost (zeroing and flushing its bins) is shared by two tiles or more
constexpr uint32_t kSumWords = 8;                      // the sums of compare (KS_N_SUMS, padded) in front of the device bins
constexpr uint16_t kNoSlot = 0xFFFF;

enum { kCompare = 0, kCount = 1, kWrite = 2 };

static_assert(kTileWords == NTK_KSET_TILE_WORDS && kBinsBig == NTK_KSET_MAX_BINS, "the header states the tile and the bin limit");
static_assert(kTileOf<2> % kThreads == 0 && kTileOf<1> + 2 < kNoSlot, "whole rounds of the store pass; a staged key index fits a slot's u16");
static_assert(KS_N_SUMS <= kSumWords, "the sums fit their words");
static_assert(KS_INTERSECT == NTK_KSET_INTERSECT && KS_UNION == NTK_KSET_UNION && KS_SUBTRACT == NTK_KSET_SUBTRACT &&
              KS_COUNTERS_SUBTRACT == NTK_KSET_COUNTERS_SUBTRACT, "the rule's ops are the header's");
static_assert(KS_MIN == NTK_KSET_MIN && KS_MAX == NTK_KSET_MAX && KS_SUM == NTK_KSET_SUM && KS_LEFT == NTK_KSET_LEFT &&
              KS_RIGHT == NTK_KSET_RIGHT, "the rule's rules are the header's");
static_assert(sizeof(ntk_kmer_sets_totals) == 13 * sizeof(uint64_t), "ks_totals fills thirteen words");

struct JoinArgs {
    const uint64_t *a_keys, *a_counts, *b_keys, *b_counts;
    uint64_t n_a, n_b, n_tiles;
    const uint64_t *splits;       // n_tiles + 1: split(min(t * kTileOf<KW>, n_a + n_b))
    uint32_t op, rule;            // COUNT, WRITE
    uint32_t n_bins_a, n_bins_b;  // COMPARE
    uint64_t *sums, *hist;        // COMPARE: KS_N_SUMS words and n_bins_a * n_bins_b words, zeroed
    uint64_t *tile_counts;        // COUNT: n_tiles
    const uint64_t *bases;        // WRITE: n_tiles + 1, the exclusive scan of tile_counts
    uint64_t *out_keys, *out_counts;
};

// one thread per tile boundary
template <int KW>
__global__ __launch_bounds__(kThreads) void ks_split_kernel(const uint64_t *a, uint64_t n_a, const uint64_t *b, uint64_t n_b, uint64_t n_tiles,
                                                            uint64_t *splits)
{
    const uint64_t t = (uint64_t)blockIdx.x * kThreads + threadIdx.x;
    if (t > n_tiles) return;
    const uint64_t n = n_a + n_b, d = t * kTileOf<KW> < n ? t * kTileOf<KW> : n;
    splits[t] = ks_split<KW>(a, n_a, b, n_b, d);
}

// adjacent pairs that do not ascend strictly
template <int KW>
__global__ __launch_bounds__(kThreads) void ks_validate_kernel(const uint64_t *keys, uint64_t n, uint64_t *n_violations)
{
    const uint64_t stride = (uint64_t)gridDim.x * kThreads;
    uint64_t bad = 0;
    for (uint64_t i = (uint64_t)blockIdx.x * kThreads + threadIdx.x; i + 1 < n; i += stride)
        bad += ks_less<KW>(keys + i * KW, keys + (i + 1) * KW) ? 0 : 1;
    bad = wave_sum(bad);
    if ((threadIdx.x & 63) == 0 && bad) add_agent(n_violations, bad);
}

template <int KW, int MODE, uint32_t BINS>
__global__ __launch_bounds__(kThreads) void ks_join_kernel(JoinArgs g)
{
    constexpr uint32_t kTile = kTileOf<KW>;
    constexpr uint32_t kStageKeys = kTile + 2;        // with the look-behind and the look-ahead element
    constexpr uint32_t kRounds = kTile / kThreads;    // slots per thread of the store pass
    __shared__ uint64_t stage[kStageKeys * KW];
    __shared__ uint32_t bins[MODE == kCompare ? BINS : 1];
    __shared__ uint64_t slot_count[MODE == kWrite ? kTile : 1];
    __shared__ uint16_t slot_src[MODE == kWrite ? kTile : 2];
    __shared__ uint64_t wave_part[kWaves][kSumWords];
    __shared__ uint32_t red[kWaves];

    const uint32_t tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const uint64_t n = g.n_a + g.n_b;
    const uint32_t n_bins = g.n_bins_a * g.n_bins_b;   // at most BINS (the host picks the build)
    KsSums acc;
    if (MODE == kCompare)
        for (uint32_t b = tid; b < n_bins; b += kThreads) bins[b] = 0;

    for (uint64_t t = blockIdx.x; t < g.n_tiles; t += gridDim.x) {
        const uint64_t d0 = t * kTile, d1 = d0 + kTile < n ? d0 + kTile : n;
        const KsView v = ks_view(g.splits[t], g.splits[t + 1], d0, d1, g.n_b);
        // stage A[sa0, sa0 + na) and behind it B[j0, j0 + nb), word by word: every load is issued before the first store
        const uint32_t words_a = v.na * KW, words = (v.na + v.nb) * KW;   // at most kStageKeys * KW
        const uint64_t *src_a = g.a_keys + v.sa0 * KW, *src_b = g.b_keys + v.j0 * KW;
        constexpr uint32_t kLoads = (kStageKeys * KW + kThreads - 1) / kThreads;
        uint64_t held[kLoads];
#pragma unroll
        for (uint32_t u = 0; u < kLoads; u++) {
            const uint32_t w = tid + u * kThreads;
            held[u] = w < words_a ? src_a[w] : w < words ? src_b[w - words_a] : 0;
        }
        __syncthreads();   // the tile before is done with the stage and the slots
#pragma unroll
        for (uint32_t u = 0; u < kLoads; u++) {
            const uint32_t w = tid + u * kThreads;
            if (w < words) stage[w] = held[u];
        }
        if (MODE == kWrite)
            for (uint32_t m = tid; m < kTile; m += kThreads) slot_src[m] = kNoSlot;
        __syncthreads();

        const uint64_t *sa = stage, *sb = stage + words_a;
        const uint32_t len = v.la + v.lb;
        const bool with_counts = MODE == kWrite || g.op == KS_COUNTERS_SUBTRACT;   // COUNT: only where a count decides
        uint32_t kept = 0;
        for (uint32_t e = tid; e < len; e += kThreads) {
            if (e < v.la) {
                const KsHit hit = ks_probe_a<KW>(v, sa, sb, e);
                const uint64_t i = v.i0 + e, j = v.j0 + hit.twin;   // j < n_b where shared
                if (MODE == kCompare) {
                    const uint64_t ca = g.a_counts[i], cb = hit.shared ? g.b_counts[j] : 0;
                    atomicAdd(&bins[ks_compare_a(acc, hit.shared, ca, cb, g.n_bins_a, g.n_bins_b)], 1u);
                } else {
                    const uint64_t ca = with_counts && ks_a_needs_a(g.op, hit.shared) ? g.a_counts[i] : 0;
                    const uint64_t cb = with_counts && ks_a_needs_b(g.op, hit.shared) ? g.b_counts[j] : 0;
                    uint64_t count = 0;
                    if (ks_out_a(g.op, g.rule, hit.shared, ca, cb, count)) {
                        kept++;
                        if (MODE == kWrite) {
                            slot_src[hit.slot] = (uint16_t)(v.a_first + e);
                            slot_count[hit.slot] = count;
                        }
                    }
                }
            } else {
                const uint32_t y = e - v.la;
                const KsHit hit = ks_probe_b<KW>(v, sa, sb, y);
                const uint64_t j = v.j0 + y;
                if (MODE == kCompare) {
                    if (!hit.shared) atomicAdd(&bins[ks_compare_b(acc, g.b_counts[j], g.n_bins_b)], 1u);
                } else if (ks_out_b(g.op, hit.shared)) {
                    kept++;
                    if (MODE == kWrite) {
                        slot_src[hit.slot] = (uint16_t)(v.na + y);
                        slot_count[hit.slot] = g.b_counts[j];
                    }
                }
            }
        }

        if (MODE == kCount) {
            const uint32_t total = block_sum_u32(kept, red);
            if (tid == 0) g.tile_counts[t] = total;
        }
        if (MODE == kWrite) {
            __syncthreads();
            // wave w stores the slots [w * kTile / kWaves, (w + 1) * kTile / kWaves) in rounds of 64
            uint64_t ballot[kRounds];
            uint16_t src[kRounds];
            uint32_t mine = 0;
#pragma unroll
            for (uint32_t r = 0; r < kRounds; r++) {
                src[r] = slot_src[wave * (kTile / kWaves) + r * 64 + lane];
                ballot[r] = __ballot(src[r] != kNoSlot);
                mine += (uint32_t)__popcll(ballot[r]);
            }
            if (lane == 0) red[wave] = mine;
            __syncthreads();
            uint32_t carry = 0;   // kept slots before this round (wave-uniform)
            for (uint32_t w = 0; w < wave; w++) carry += red[w];
            // never past what COUNT saw of the tile (they differ only on input that does not ascend)
            const uint64_t base = g.bases[t], limit = g.bases[t + 1] - base;
#pragma unroll
            for (uint32_t r = 0; r < kRounds; r++) {
                const uint32_t rank = carry + (uint32_t)__popcll(ballot[r] & (((uint64_t)1 << lane) - 1));
                if (src[r] != kNoSlot && rank < limit) {
                    const uint64_t out = base + rank;
                    for (int q = 0; q < KW; q++) g.out_keys[out * KW + q] = stage[(uint32_t)src[r] * KW + q];
                    g.out_counts[out] = slot_count[wave * (kTile / kWaves) + r * 64 + lane];
                }
                carry += (uint32_t)__popcll(ballot[r]);
            }
        }
    }

    if (MODE == kCompare) {
        const uint64_t sums[KS_N_SUMS] = {acc.n_shared, acc.sum_a, acc.sum_a_shared, acc.sum_b_shared, acc.sum_b_only, acc.sum_min};
#pragma unroll
        for (int q = 0; q < KS_N_SUMS; q++) {
            const uint64_t s = wave_sum(sums[q]);
            if (lane == 0) wave_part[wave][q] = s;
        }
        __syncthreads();   // also: every add into the bins is done
        if (tid < KS_N_SUMS) {
            uint64_t s = 0;
            for (uint32_t w = 0; w < kWaves; w++) s += wave_part[w][tid];
            if (s) add_agent(g.sums + tid, s);
        }
        for (uint32_t b = tid; b < n_bins; b += kThreads)
            if (bins[b]) add_agent(g.hist + b, bins[b]);
    }
}

// two byte ranges share a byte (by differences, so that no end address is formed and nothing can wrap)
bool overlaps(const void *p, uint64_t p_bytes, const void *q, uint64_t q_bytes)
{
    const uintptr_t a = (uintptr_t)p, b = (uintptr_t)q;
    if (!p_bytes || !q_bytes) return false;
    return a <= b ? b - a < p_bytes : a - b < q_bytes;
}

}  // namespace

struct ntk_kmer_sets : Consumer {
    uint32_t kw = 1;
    DeviceArray<uint64_t> d_splits, d_tile_counts, d_bases;   // one word more than the tiles they hold, each
    DeviceArray<char> d_scan_tmp;          // rocPRIM's temporary storage of the scan over the tile counts
    DeviceArray<uint64_t> d_bins;          // kSumWords + kBinsBig words
    Pinned<uint64_t> h_stage;              // likewise
    uint64_t n_launches = 0, n_calls = 0;

    void release_scratch() { d_splits.release(); d_tile_counts.release(); d_bases.release(); d_scan_tmp.release(); }
};

namespace {

// the exclusive scan of the tile counts into the bases; item n_tiles is the total
hipError_t scan_tiles(ntk_kmer_sets *h, void *tmp, size_t &tmp_bytes, uint64_t n_tiles)
{
    return rocprim::exclusive_scan(tmp, tmp_bytes, h->d_tile_counts.p, h->d_bases.p, (uint64_t)0, (size_t)(n_tiles + 1),
                                   rocprim::plus<uint64_t>(), h->stream);
}

// room for the arrays of n_tiles tiles: a number of tiles that doubles from 1024, and one word more
int ensure_tiles(ntk_kmer_sets *h, uint64_t n_tiles)
{
    const uint64_t words = grow_doubling(0, n_tiles) + 1;
    int rc = h->d_splits.ensure(h->stream, words, grow_exact);
    if (!rc) rc = h->d_tile_counts.ensure(h->stream, words, grow_exact);
    if (!rc) rc = h->d_bases.ensure(h->stream, words, grow_exact);
    return rc;
}

int check_list(const uint64_t *keys, const uint64_t *counts, uint64_t n)
{
    if (n && (!keys || !counts)) return NTK_ERR_BAD_ARG;
    if (((uintptr_t)keys & 7) || ((uintptr_t)counts & 7)) return NTK_ERR_BAD_ARG;
    return n >= ((uint64_t)1 << 58) ? NTK_ERR_BAD_ARG : NTK_OK;   // n_a + n_b and every byte count (16 B per key at most) stay 64-bit
}

// the tiles of a join of n > 0 merged elements: the scratch and the splits; *blocks = the join's grid
int prepare(ntk_kmer_sets *h, JoinArgs &g, unsigned *blocks)
{
    CT_HIPCHK(hipSetDevice(h->device));
    const uint64_t n = g.n_a + g.n_b;
    const uint64_t tile = kTileWords / h->kw;
    g.n_tiles = (n + tile - 1) / tile;
    const uint64_t floor_blocks = (g.n_tiles + kMaxTilesPerBlock - 1) / kMaxTilesPerBlock;
    if (floor_blocks > 0x7FFFFFFFull) return NTK_ERR_UNSUPPORTED;
    const int rc = ensure_tiles(h, g.n_tiles);
    if (rc) return rc;
    g.splits = h->d_splits.p; g.tile_counts = h->d_tile_counts.p; g.bases = h->d_bases.p;
    const unsigned fill = grid_for(g.n_tiles, kMinTilesPerBlock, (unsigned)h->n_cu * kBlocksPerCu);
    *blocks = fill < floor_blocks ? (unsigned)floor_blocks : fill;
    const unsigned split_blocks = grid_for(g.n_tiles + 1, kThreads, 0x7FFFFFFFu);
    if (h->kw == 1)
        hipLaunchKernelGGL(ks_split_kernel<1>, dim3(split_blocks), dim3(kThreads), 0, h->stream, g.a_keys, g.n_a, g.b_keys, g.n_b, g.n_tiles,
                           h->d_splits.p);
    else
        hipLaunchKernelGGL(ks_split_kernel<2>, dim3(split_blocks), dim3(kThreads), 0, h->stream, g.a_keys, g.n_a, g.b_keys, g.n_b, g.n_tiles,
                           h->d_splits.p);
    CT_HIPCHK(hipGetLastError());
    h->n_launches++;
    return NTK_OK;
}

template <int MODE, uint32_t BINS>
int launch_join(ntk_kmer_sets *h, const JoinArgs &g, unsigned blocks)
{
    if (h->kw == 1) hipLaunchKernelGGL((ks_join_kernel<1, MODE, BINS>), dim3(blocks), dim3(kThreads), 0, h->stream, g);
    else hipLaunchKernelGGL((ks_join_kernel<2, MODE, BINS>), dim3(blocks), dim3(kThreads), 0, h->stream, g);
    CT_HIPCHK(hipGetLastError());
    h->n_launches++;
    return NTK_OK;
}

}  // namespace

extern "C" {

int ntk_kmer_sets_create(ntk_ctx *ctx, uint32_t key_words, ntk_kmer_sets **out)
{
    if (!ctx || !out) return NTK_ERR_BAD_ARG;
    *out = nullptr;
    if (key_words != 1 && key_words != 2) return NTK_ERR_BAD_ARG;
    ntk_kmer_sets *h = new (std::nothrow) ntk_kmer_sets();
    if (!h) return NTK_ERR_NOMEM;
    int rc = h->bind(ctx, 0, 0);
    if (rc) { delete h; return rc; }
    h->kw = key_words;
    if ((rc = h->d_bins.ensure(h->stream, kSumWords + kBinsBig, grow_exact)) || (rc = h->h_stage.alloc(kSumWords + kBinsBig))) {
        ntk_kmer_sets_destroy(h);
        return rc;
    }
    *out = h;
    return NTK_OK;
}

void ntk_kmer_sets_destroy(ntk_kmer_sets *h)
{
    if (!h) return;
    (void)hipSetDevice(h->device);
    (void)hipStreamSynchronize(h->stream);
    h->release_scratch();
    h->d_bins.release();
    h->h_stage.release();
    (void)hipGetLastError();
    delete h;
}

int ntk_kmer_sets_release(ntk_kmer_sets *h)
{
    if (!h) return NTK_ERR_BAD_ARG;
    CT_HIPCHK(hipSetDevice(h->device));
    CT_HIPCHK(hipStreamSynchronize(h->stream));
    h->release_scratch();
    return NTK_OK;
}

int ntk_kmer_sets_stats(ntk_kmer_sets *h, struct ntk_kmer_sets_stats *out)
{
    if (!h || !out) return NTK_ERR_BAD_ARG;
    out->key_words = h->kw;
    out->device_bytes = h->d_bins.bytes() + h->d_splits.bytes() + h->d_tile_counts.bytes() + h->d_bases.bytes() + h->d_scan_tmp.bytes();
    out->n_launches = h->n_launches;
    out->n_calls = h->n_calls;
    return NTK_OK;
}

int ntk_kmer_sets_validate_device(ntk_kmer_sets *h, const uint64_t *d_keys, uint64_t n, uint64_t *n_violations)
{
    if (!h || !n_violations || (n && !d_keys) || ((uintptr_t)d_keys & 7) || n >= ((uint64_t)1 << 58)) return NTK_ERR_BAD_ARG;
    *n_violations = 0;
    if (n < 2) return NTK_OK;
    CT_HIPCHK(hipSetDevice(h->device));
    CT_HIPCHK(hipMemsetAsync(h->d_bins.p, 0, sizeof(uint64_t), h->stream));
    const unsigned blocks = grid_for(n - 1, kThreads, (unsigned)h->n_cu * 8);
    if (h->kw == 1) hipLaunchKernelGGL(ks_validate_kernel<1>, dim3(blocks), dim3(kThreads), 0, h->stream, d_keys, n, h->d_bins.p);
    else hipLaunchKernelGGL(ks_validate_kernel<2>, dim3(blocks), dim3(kThreads), 0, h->stream, d_keys, n, h->d_bins.p);
    CT_HIPCHK(hipGetLastError());
    h->n_launches++; h->n_calls++;
    const int rc = h->h_stage.read(h->stream, h->d_bins.p, 1);
    if (!rc) *n_violations = h->h_stage.p[0];
    return rc;
}

int ntk_kmer_sets_compare_device(ntk_kmer_sets *h, const uint64_t *d_a_keys, const uint64_t *d_a_counts, uint64_t n_a,
                                 const uint64_t *d_b_keys, const uint64_t *d_b_counts, uint64_t n_b, uint32_t n_bins_a, uint32_t n_bins_b,
                                 uint64_t *hist, struct ntk_kmer_sets_totals *totals)
{
    if (!h || n_bins_a < 2 || n_bins_b < 2 || (uint64_t)n_bins_a * n_bins_b > kBinsBig) return NTK_ERR_BAD_ARG;
    int rc = check_list(d_a_keys, d_a_counts, n_a);
    if (!rc) rc = check_list(d_b_keys, d_b_counts, n_b);
    if (rc) return rc;
    const uint32_t n_bins = n_bins_a * n_bins_b;
    uint64_t *sums = h->h_stage.p;
    if (n_a + n_b == 0) {
        memset(h->h_stage.p, 0, (kSumWords + n_bins) * sizeof(uint64_t));
    } else {
        JoinArgs g = {};
        g.a_keys = d_a_keys; g.a_counts = d_a_counts; g.n_a = n_a;
        g.b_keys = d_b_keys; g.b_counts = d_b_counts; g.n_b = n_b;
        g.n_bins_a = n_bins_a; g.n_bins_b = n_bins_b;
        g.sums = h->d_bins.p; g.hist = h->d_bins.p + kSumWords;
        unsigned blocks = 0;
        if ((rc = prepare(h, g, &blocks))) return rc;
        CT_HIPCHK(hipMemsetAsync(h->d_bins.p, 0, (kSumWords + n_bins) * sizeof(uint64_t), h->stream));
        rc = n_bins <= kBinsSmall ? launch_join<kCompare, kBinsSmall>(h, g, blocks) : launch_join<kCompare, kBinsBig>(h, g, blocks);
        if (rc) return rc;
        h->n_calls++;
        if ((rc = h->h_stage.read(h->stream, h->d_bins.p, kSumWords + n_bins))) return rc;
    }
    if (totals) ks_totals(sums, n_a, n_b, &totals->n_a);
    if (hist) memcpy(hist, h->h_stage.p + kSumWords, n_bins * sizeof(uint64_t));
    return NTK_OK;
}

int ntk_kmer_sets_apply_device(ntk_kmer_sets *h, uint32_t op, uint32_t rule, const uint64_t *d_a_keys, const uint64_t *d_a_counts, uint64_t n_a,
                               const uint64_t *d_b_keys, const uint64_t *d_b_counts, uint64_t n_b, uint64_t *d_out_keys,
                               uint64_t *d_out_counts, uint64_t cap, uint64_t *n)
{
    if (!h || !n || !ks_op_ok(op, rule)) return NTK_ERR_BAD_ARG;
    int rc = check_list(d_a_keys, d_a_counts, n_a);
    if (!rc) rc = check_list(d_b_keys, d_b_counts, n_b);
    if (!rc) rc = check_list(d_out_keys, d_out_counts, cap);
    if (rc) return rc;
    const uint64_t key_bytes = h->kw * sizeof(uint64_t);
    const struct { const void *p; uint64_t bytes; } in[4] = {{d_a_keys, n_a * key_bytes}, {d_a_counts, n_a * sizeof(uint64_t)},
                                                            {d_b_keys, n_b * key_bytes}, {d_b_counts, n_b * sizeof(uint64_t)}};
    for (const auto &r : in)
        if (overlaps(d_out_keys, cap * key_bytes, r.p, r.bytes) || overlaps(d_out_counts, cap * sizeof(uint64_t), r.p, r.bytes))
            return NTK_ERR_BAD_ARG;
    if (overlaps(d_out_keys, cap * key_bytes, d_out_counts, cap * sizeof(uint64_t))) return NTK_ERR_BAD_ARG;
    *n = 0;
    if (n_a + n_b == 0) return NTK_OK;

    JoinArgs g = {};
    g.a_keys = d_a_keys; g.a_counts = d_a_counts; g.n_a = n_a;
    g.b_keys = d_b_keys; g.b_counts = d_b_counts; g.n_b = n_b;
    g.op = op; g.rule = rule;
    g.out_keys = d_out_keys; g.out_counts = d_out_counts;
    unsigned blocks = 0;
    if ((rc = prepare(h, g, &blocks))) return rc;
    h->n_calls++;
    if ((rc = launch_join<kCount, 1>(h, g, blocks))) return rc;
    CT_HIPCHK(hipMemsetAsync(h->d_tile_counts.p + g.n_tiles, 0, sizeof(uint64_t), h->stream));   // the scan's last output is the total
    rc = with_tmp(h->d_scan_tmp, h->stream, grow_exact,
                  [&](void *tmp, size_t &tmp_bytes) { return scan_tiles(h, tmp, tmp_bytes, g.n_tiles); });
    if (rc || (rc = h->h_stage.read(h->stream, h->d_bases.p + g.n_tiles, 1))) return rc;
    const uint64_t total = h->h_stage.p[0];
    *n = total;
    if (total > cap) return NTK_ERR_CAPACITY;
    if (total == 0) return NTK_OK;
    if ((rc = launch_join<kWrite, 1>(h, g, blocks))) return rc;
    CT_HIPCHK(hipStreamSynchronize(h->stream));
    return NTK_OK;
}

}  // extern "C"
