// A coloured k-mer index on the device and the read screen against it (include/needletail_amd_colors.h): k-mer -> the set of references
// that hold it, one bit each, and one pass over a batch that writes per record how many of its k-mers every colour holds.  A consumer
// of the core's public ABI: the k-mers are the values ntk_materialize_device_quality emits, chunk by chunk.
//
// The index is the count table's scheme with a mask where the count was (ntk_colors_rule.hpp states it, and the CPU suite runs it):
// keys are write-once (EMPTY -> key, claimed by an agent-scope CAS), masks change only through agent-scope atomic ORs.
//
// The screen: a record's candidate windows are the window ends [offsets[r] + k - 1, offsets[r + 1] - 1); the valid plane says which of
// them were emitted.  Per chunk, kc_wave_kernel gives a wave to a record (grid-stride over the records): in rounds of 64 window ends a
// lane reads the chunk's value, probes the index, and the wave counts by one ballot and one population count per colour, lane c
// keeping column c, so the row goes out coalesced.  Only the window ends of the chunk are taken (a window counts where it ends), and
// the wave adds its share to the zeroed outputs by a plain read-add-write: chunks are stream-ordered and the wave owns the record.
// A record of more than kLongRecord windows goes to a device-built list and is taken by the whole grid of kc_long_kernel, round by
// round, whose waves add with agent-scope atomics.  After the last chunk kc_best_kernel reads the finished matrix.  Nothing here is
// proportional to the bases of the batch.  DESIGN.md section 21.
#include "../../include/needletail_amd_colors.h"
#include "ntk_consumer.hpp"
#include "ntk_colors_rule.hpp"

#include <cstring>
#include <new>

namespace {

static_assert(NTK_COLORS_MAX == KC_COLORS_MAX && NTK_COLORS_NONE == KC_NONE, "the rule header restates the public header");

constexpr int kWaveThreads = 256;                        // kc_wave_kernel: four records per block at a time
constexpr int kLongThreads = 256;                        // kc_long_kernel: four rounds of a long record per block at a time
constexpr uint64_t kLongRecord = 16384;                  // records with more candidate windows go to kc_long_kernel
// stats words on the device, then the per-colour census
constexpr int kStKeys = 0, kStDropped = 1, kStMasked = 2, kStSide = 3, kStWords = 4, kStAll = kStWords + (int)KC_COLORS_MAX;

using Row = ntk_kmer_colors_row;
static_assert(sizeof(Row) == 40, "the header states the row");
static_assert(sizeof(struct ntk_kmer_colors_stats) == 576, "the header states the stats");

// the index as the rule reads it ...
struct ReadMem {
    const uint64_t *keys, *masks;
    __device__ uint64_t key(uint64_t slot) const { return keys[slot]; }
    __device__ uint64_t mask(uint64_t slot) const { return masks[slot]; }
};

// ... and as it writes it
struct WriteMem {
    uint64_t *keys, *masks;
    __device__ uint64_t key(uint64_t slot) const { return keys[slot]; }
    __device__ uint64_t claim(uint64_t slot, uint64_t key)
    {
        uint64_t expected = KC_EMPTY;
        (void)__hip_atomic_compare_exchange_strong(&keys[slot], &expected, key, __ATOMIC_RELAXED, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        return expected;
    }
    __device__ void or_mask(uint64_t slot, uint64_t m)
    {
        (void)__hip_atomic_fetch_or(&masks[slot], m, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    }
};

struct AddArgs {
    const uint64_t *keys, *key_masks;   // key_masks == nullptr: `mask` for every key
    uint64_t mask, n;
    WriteMem table;
    uint64_t slots, bits;               // bits: kc_color_bits(n_colors)
    uint32_t probe_max;
    uint64_t *stats;
};

// One key per lane, grid-stride; every lane of a wave runs the same number of iterations, so the counters are summed across the wave
// once at the end and added by one lane.
__global__ __launch_bounds__(kThreads) void kc_add_kernel(AddArgs a)
{
    uint64_t fresh = 0, dropped = 0, masked = 0;
    const uint64_t stride = (uint64_t)gridDim.x * blockDim.x, rounds = (a.n + stride - 1) / stride;
    uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    for (uint64_t r = 0; r < rounds; r++, i += stride) {
        if (i >= a.n) continue;
        uint64_t m = a.key_masks ? a.key_masks[i] : a.mask;
        masked += __popcll(m & ~a.bits);
        m &= a.bits;
        if (m == 0) continue;
        const uint64_t key = a.keys[i];
        if (key == KC_EMPTY) {
            (void)__hip_atomic_fetch_or(a.stats + kStSide, m, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
            continue;
        }
        const int got = kc_insert_or(a.table, a.slots, a.probe_max, key, m);
        fresh += got == KC_INSERTED;
        dropped += got == KC_DROPPED;
    }
    fresh = wave_sum(fresh); dropped = wave_sum(dropped); masked = wave_sum(masked);
    if ((threadIdx.x & 63) == 0) {
        if (fresh) add_agent(a.stats + kStKeys, fresh);
        if (dropped) add_agent(a.stats + kStDropped, dropped);
        if (masked) add_agent(a.stats + kStMasked, masked);
    }
}

struct LookupArgs {
    ReadMem table;
    uint64_t slots, side;
    uint32_t probe_max;
    const uint64_t *queries;
    uint64_t n;
    uint64_t *out;
};

__global__ __launch_bounds__(kThreads) void kc_lookup_kernel(LookupArgs a)
{
    const uint64_t stride = (uint64_t)gridDim.x * blockDim.x;
    for (uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; i < a.n; i += stride)
        a.out[i] = kc_lookup(a.table, a.slots, a.probe_max, a.side, a.queries[i]);
}

struct CensusArgs {
    ReadMem table;
    uint64_t slots;
    uint64_t *per_color;   // KC_COLORS_MAX words, zeroed
};

// keys per bit: block-private LDS counters over a grid-stride share of the slots, then one atomic per non-zero counter per block
__global__ __launch_bounds__(kThreads) void kc_census_kernel(CensusArgs a)
{
    __shared__ uint32_t bins[KC_COLORS_MAX];
    if (threadIdx.x < KC_COLORS_MAX) bins[threadIdx.x] = 0;
    __syncthreads();
    const uint64_t stride = (uint64_t)gridDim.x * blockDim.x;
    for (uint64_t s = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; s < a.slots; s += stride) {
        if (a.table.key(s) == KC_EMPTY) continue;
        for (uint64_t m = a.table.mask(s); m; m &= m - 1) atomicAdd(&bins[__builtin_ctzll(m)], 1u);
    }
    __syncthreads();
    if (threadIdx.x < KC_COLORS_MAX && bins[threadIdx.x]) add_agent(a.per_color + threadIdx.x, bins[threadIdx.x]);
}

struct ScreenArgs {
    const uint64_t *values;    // the chunk's materialised values, indexed by window end - base
    const uint16_t *valid16;   // bit (15 - i % 16) of word i / 16: the window that ends at base + i is emitted
    uint64_t base, start, end; // the chunk: materialised from `base`, its window ends are [start, end)
    ReadMem table;
    uint64_t slots, side;
    uint32_t probe_max, k, n_colors;
    const uint64_t *offsets;   // n_records + 1 record starts
    uint64_t n_bytes, n_records;
    uint64_t *n_long;          // records of this chunk handed to kc_long_kernel ...
    uint64_t *long_list;       // ... and their indices, at most long_cap
    uint64_t long_cap;
    Row *rows;
    uint64_t *hits, *single;   // single may be nullptr
};

// what a wave has counted of a record: lane c holds column c of the two matrix rows, the three scalars are wave-uniform
struct Acc {
    uint64_t hits = 0, single = 0, n_kmers = 0, n_hit = 0, n_single = 0;
};

// Rounds first, first + stride, ... of 64 window ends of [lo, hi), all within the chunk: lane l takes window end lo + 64 * round + l.
__device__ inline void screen_rounds(const ScreenArgs &a, uint64_t lo, uint64_t hi, uint64_t first, uint64_t stride, uint32_t lane, Acc &acc)
{
    for (uint64_t e0 = lo + first * 64; e0 < hi; e0 += stride * 64) {
        const uint64_t e = e0 + lane;
        uint64_t m = 0;
        bool ok = false;
        if (e < hi) {
            const uint64_t at = e - a.base;
            ok = (a.valid16[at >> 4] >> (15 - (at & 15))) & 1u;
            if (ok) m = kc_lookup(a.table, a.slots, a.probe_max, a.side, a.values[at]);
        }
        acc.n_kmers += __popcll(__ballot(ok));
        const uint64_t any = __ballot(m != 0);
        if (!any) continue;
        acc.n_hit += __popcll(any);
        const bool one = kc_is_single(m);
        const uint64_t singles = __ballot(one);
        acc.n_single += __popcll(singles);
        for (uint32_t c = 0; c < a.n_colors; c++) {
            const uint64_t n = __popcll(__ballot(kc_has(m, c)));
            if (lane == c) acc.hits += n;
        }
        if (singles && a.single) {
            for (uint32_t c = 0; c < a.n_colors; c++) {
                const uint64_t n = __popcll(__ballot(one && kc_has(m, c)));
                if (lane == c) acc.single += n;
            }
        }
    }
}

// record r's window ends in this chunk, [lo, hi) (empty: lo >= hi), and whether the whole record is a long one
__device__ inline bool chunk_share(const ScreenArgs &a, uint64_t r, uint64_t &lo, uint64_t &hi)
{
    record_span(a.offsets, a.n_bytes, a.k, r, lo, hi);
    lo = uniform(lo); hi = uniform(hi);
    const bool is_long = hi - lo > kLongRecord;
    if (lo < a.start) lo = a.start;
    if (hi > a.end) hi = a.end;
    return is_long;
}

// One wave per record, grid-stride over the records.  A long record with a share in this chunk is appended to the list (one atomic)
// and left to kc_long_kernel.
__global__ __launch_bounds__(kWaveThreads) void kc_wave_kernel(ScreenArgs a)
{
    const uint32_t lane = threadIdx.x & 63;
    const uint64_t waves = (uint64_t)gridDim.x * (kWaveThreads / 64);
    const uint64_t first = (uint64_t)blockIdx.x * (kWaveThreads / 64) + __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    for (uint64_t r = first; r < a.n_records; r += waves) {
        uint64_t lo, hi;
        const bool is_long = chunk_share(a, r, lo, hi);
        if (lo >= hi) continue;
        if (is_long) {
            if (lane == 0) {
                const uint64_t at = __hip_atomic_fetch_add(a.n_long, (uint64_t)1, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
                if (at < a.long_cap) a.long_list[at] = r;
            }
            continue;
        }
        Acc acc;
        screen_rounds(a, lo, hi, 0, 1, lane, acc);
        // the wave owns the record, and the chunk before is done: a plain read-add-write
        if (lane < a.n_colors) {
            const uint64_t at = r * a.n_colors + lane;
            if (acc.hits) a.hits[at] += acc.hits;
            if (acc.single) a.single[at] += acc.single;
        }
        if (lane == 0 && acc.n_kmers) {
            Row *row = a.rows + r;
            row->n_kmers += acc.n_kmers;
            row->n_hit += acc.n_hit;
            row->n_single += acc.n_single;
        }
    }
}

// The long records of the chunk, each taken by every wave of the grid, round by round; the waves share the row, so they add atomically.
__global__ __launch_bounds__(kLongThreads) void kc_long_kernel(ScreenArgs a)
{
    const uint32_t lane = threadIdx.x & 63;
    const uint64_t waves = (uint64_t)gridDim.x * (kLongThreads / 64);
    const uint64_t first = (uint64_t)blockIdx.x * (kLongThreads / 64) + __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    uint64_t n_long = *a.n_long;
    if (n_long > a.long_cap) n_long = a.long_cap;
    for (uint64_t i = 0; i < n_long; i++) {
        const uint64_t r = a.long_list[i];
        uint64_t lo, hi;
        (void)chunk_share(a, r, lo, hi);
        if (lo >= hi) continue;
        Acc acc;
        screen_rounds(a, lo, hi, first, waves, lane, acc);
        if (lane < a.n_colors) {
            const uint64_t at = r * a.n_colors + lane;
            if (acc.hits) add_agent(a.hits + at, acc.hits);
            if (acc.single) add_agent(a.single + at, acc.single);
        }
        if (lane == 0 && acc.n_kmers) {
            Row *row = a.rows + r;
            add_agent(&row->n_kmers, acc.n_kmers);
            if (acc.n_hit) add_agent(&row->n_hit, acc.n_hit);
            if (acc.n_single) add_agent(&row->n_single, acc.n_single);
        }
    }
}

struct BestArgs {
    const uint64_t *hits;
    Row *rows;
    uint64_t n_records;
    uint32_t n_colors;
};

// best and second of every record from the finished matrix, one record per thread
__global__ __launch_bounds__(kThreads) void kc_best_kernel(BestArgs a)
{
    const uint64_t stride = (uint64_t)gridDim.x * blockDim.x;
    for (uint64_t r = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; r < a.n_records; r += stride) {
        const KcBest b = kc_best(a.hits + r * a.n_colors, a.n_colors);
        a.rows[r].best = b.best;
        a.rows[r].second = b.second;
    }
}

}  // namespace

struct ntk_kmer_colors : Consumer {
    uint32_t n_colors = 0, probe_max = 0;
    uint64_t slots = 0, n_launches = 0;
    // the index, from create to destroy
    DeviceArray<uint64_t> d_keys, d_masks;   // 16 B per slot
    DeviceArray<uint64_t> d_stats;           // kStAll words
    Pinned<uint64_t> h_stage;                // stats read-backs
    // run_device's, grown on demand
    MaterialiseScratch scratch;              // of one chunk
    DeviceArray<uint64_t> d_long;            // [0]: the number of long records, then their indices (one per kLongRecord bases at most)

    uint64_t long_cap() const { return d_long.cap - 1; }

    uint64_t device_bytes() const
    {
        return d_keys.bytes() + d_masks.bytes() + d_stats.bytes() + scratch.device_bytes() + d_long.bytes();
    }

    void release_scratch() { scratch.release(); d_long.release(); }

    ReadMem read_mem() const { return ReadMem{d_keys.p, d_masks.p}; }

    // the stats words on the host (synchronises)
    int read_stats(uint64_t *w)
    {
        CT_HIPCHK(hipSetDevice(device));
        const int rc = h_stage.read(stream, d_stats.p, kStWords);
        if (!rc) memcpy(w, h_stage.p, kStWords * sizeof(uint64_t));
        return rc;
    }

    // read_stats for the read side, which refuses an incomplete index
    int read_complete(uint64_t *w)
    {
        const int rc = read_stats(w);
        return rc ? rc : w[kStDropped] ? NTK_ERR_CAPACITY : NTK_OK;
    }
};

extern "C" {

int ntk_kmer_colors_create(ntk_ctx *ctx, uint32_t k, uint32_t path, uint32_t n_colors, uint64_t capacity, ntk_kmer_colors **out)
{
    if (!ctx || !out) return NTK_ERR_BAD_ARG;
    *out = nullptr;
    if (k < 1 || k > 32) return NTK_ERR_BAD_K;
    if (path > NTK_PATH_BITS_CANONICAL || n_colors < 1 || n_colors > NTK_COLORS_MAX || capacity == 0 || capacity > ((uint64_t)3 << 38))
        return NTK_ERR_BAD_ARG;
    ntk_kmer_colors *h = new (std::nothrow) ntk_kmer_colors();
    if (!h) return NTK_ERR_NOMEM;
    h->n_colors = n_colors;
    h->slots = kc_slots(capacity);
    h->probe_max = kc_probe_bound(h->slots);
    int rc = h->bind(ctx, k, path);
    if (!rc) rc = h->d_keys.ensure(h->stream, h->slots, grow_exact);
    if (!rc) rc = h->d_masks.ensure(h->stream, h->slots, grow_exact);
    if (!rc) rc = h->d_stats.ensure(h->stream, kStAll, grow_exact);
    if (!rc) rc = h->h_stage.alloc(kStAll);
    if (!rc) rc = ntk_kmer_colors_reset(h);
    if (rc) { ntk_kmer_colors_destroy(h); return rc; }
    *out = h;
    return NTK_OK;
}

int ntk_kmer_colors_release(ntk_kmer_colors *h)
{
    if (!h) return NTK_ERR_BAD_ARG;
    CT_HIPCHK(hipSetDevice(h->device));
    CT_HIPCHK(hipStreamSynchronize(h->stream));
    h->release_scratch();
    (void)hipGetLastError();
    return NTK_OK;
}

void ntk_kmer_colors_destroy(ntk_kmer_colors *h)
{
    if (!h) return;
    if (h->stream || h->d_keys.p) {
        (void)hipSetDevice(h->device);
        (void)hipStreamSynchronize(h->stream);
    }
    h->release_scratch();
    h->d_keys.release(); h->d_masks.release(); h->d_stats.release();
    h->h_stage.release();
    (void)hipGetLastError();
    delete h;
}

int ntk_kmer_colors_reset(ntk_kmer_colors *h)
{
    if (!h) return NTK_ERR_BAD_ARG;
    CT_HIPCHK(hipSetDevice(h->device));
    CT_HIPCHK(hipMemsetAsync(h->d_keys.p, 0xFF, h->slots * sizeof(uint64_t), h->stream));
    CT_HIPCHK(hipMemsetAsync(h->d_masks.p, 0, h->slots * sizeof(uint64_t), h->stream));
    CT_HIPCHK(hipMemsetAsync(h->d_stats.p, 0, kStAll * sizeof(uint64_t), h->stream));
    return NTK_OK;
}

int ntk_kmer_colors_add_device(ntk_kmer_colors *h, const uint64_t *d_keys, const uint64_t *d_masks, uint64_t mask, uint64_t n)
{
    if (!h) return NTK_ERR_BAD_ARG;
    const uint64_t bits = kc_color_bits(h->n_colors);
    if (!d_masks && (mask & ~bits)) return NTK_ERR_BAD_ARG;
    if (n == 0) return NTK_OK;
    if (!d_keys || ((uintptr_t)d_keys & 7) || ((uintptr_t)d_masks & 7)) return NTK_ERR_BAD_ARG;
    CT_HIPCHK(hipSetDevice(h->device));
    AddArgs a;
    a.keys = d_keys; a.key_masks = d_masks; a.mask = mask; a.n = n;
    a.table = WriteMem{h->d_keys.p, h->d_masks.p};
    a.slots = h->slots; a.bits = bits; a.probe_max = h->probe_max; a.stats = h->d_stats.p;
    hipLaunchKernelGGL(kc_add_kernel, dim3(grid_for(n, kThreads, (unsigned)h->n_cu * 8)), dim3(kThreads), 0, h->stream, a);
    CT_HIPCHK(hipGetLastError());
    h->n_launches++;
    return NTK_OK;
}

int ntk_kmer_colors_stats(ntk_kmer_colors *h, struct ntk_kmer_colors_stats *out)
{
    if (!h || !out) return NTK_ERR_BAD_ARG;
    CT_HIPCHK(hipSetDevice(h->device));
    CT_HIPCHK(hipMemsetAsync(h->d_stats.p + kStWords, 0, KC_COLORS_MAX * sizeof(uint64_t), h->stream));
    CensusArgs c;
    c.table = h->read_mem(); c.slots = h->slots; c.per_color = h->d_stats.p + kStWords;
    hipLaunchKernelGGL(kc_census_kernel, dim3(grid_for(h->slots, kThreads, (unsigned)h->n_cu * 2)), dim3(kThreads), 0, h->stream, c);
    CT_HIPCHK(hipGetLastError());
    h->n_launches++;
    const int rc = h->h_stage.read(h->stream, h->d_stats.p, kStAll);
    if (rc) return rc;
    const uint64_t *w = h->h_stage.p;
    memset(out, 0, sizeof *out);
    out->n_keys = w[kStKeys] + (w[kStSide] ? 1 : 0);
    out->n_dropped = w[kStDropped];
    out->n_masked_bits = w[kStMasked];
    out->slots = h->slots;
    out->device_bytes = h->device_bytes();
    out->n_launches = h->n_launches;
    for (uint32_t b = 0; b < KC_COLORS_MAX; b++) out->per_color[b] = w[kStWords + b] + ((w[kStSide] >> b) & 1u);
    out->n_colors = h->n_colors; out->k = h->k; out->path = h->path;
    return NTK_OK;
}

int ntk_kmer_colors_lookup_device(ntk_kmer_colors *h, const uint64_t *d_queries, uint64_t n, uint64_t *d_masks)
{
    if (!h || ((!d_queries || !d_masks) && n) || ((uintptr_t)d_queries & 7) || ((uintptr_t)d_masks & 7)) return NTK_ERR_BAD_ARG;
    uint64_t w[kStWords];
    const int rc = h->read_complete(w);
    if (rc) return rc;
    if (n == 0) return NTK_OK;
    LookupArgs a;
    a.table = h->read_mem(); a.slots = h->slots; a.side = w[kStSide]; a.probe_max = h->probe_max;
    a.queries = d_queries; a.n = n; a.out = d_masks;
    hipLaunchKernelGGL(kc_lookup_kernel, dim3(grid_for(n, kThreads, (unsigned)h->n_cu * 8)), dim3(kThreads), 0, h->stream, a);
    CT_HIPCHK(hipGetLastError());
    h->n_launches++;
    CT_HIPCHK(hipStreamSynchronize(h->stream));
    return NTK_OK;
}

int ntk_kmer_colors_run_device(ntk_kmer_colors *h, const uint8_t *d_seq, const uint8_t *d_qual, uint64_t n_bytes,
                               const uint64_t *d_offsets, uint64_t n_records, const ntk_params *p,
                               struct ntk_kmer_colors_row *d_rows, uint64_t *d_hits, uint64_t *d_single)
{
    int rc = check_batch_params(h, p);
    if (rc || n_records == 0 || n_bytes == 0) return rc;
    if ((rc = check_batch_pointers(d_seq, d_qual))) return rc;
    if (!d_offsets || !d_rows || !d_hits || ((uintptr_t)d_offsets & 7) || ((uintptr_t)d_rows & 7) || ((uintptr_t)d_hits & 7) ||
        ((uintptr_t)d_single & 7))
        return NTK_ERR_BAD_ARG;
    uint64_t w[kStWords];
    if ((rc = h->read_complete(w))) return rc;   // an incomplete index fails here, before anything is written
    const bool may_be_long = n_bytes > kLongRecord;   // only then can a record be long; whether one is, the device alone knows
    if ((rc = h->d_long.ensure(h->stream, n_bytes / kLongRecord + 2, grow_exact))) return rc;
    const uint64_t cells = n_records * h->n_colors;
    CT_HIPCHK(hipMemsetAsync(d_rows, 0, n_records * sizeof(Row), h->stream));
    CT_HIPCHK(hipMemsetAsync(d_hits, 0, cells * sizeof(uint64_t), h->stream));
    if (d_single) CT_HIPCHK(hipMemsetAsync(d_single, 0, cells * sizeof(uint64_t), h->stream));
    ScreenArgs g;
    g.table = h->read_mem(); g.slots = h->slots; g.side = w[kStSide];
    g.probe_max = h->probe_max; g.k = h->k; g.n_colors = h->n_colors;
    g.offsets = d_offsets; g.n_bytes = n_bytes; g.n_records = n_records;
    g.n_long = h->d_long.p; g.long_list = h->d_long.p + 1; g.long_cap = h->long_cap();
    g.rows = d_rows; g.hits = d_hits; g.single = d_single;
    // every chunk adds the share of the windows that end in it
    rc = for_each_chunk(*h, h->scratch, d_seq, d_qual, n_bytes, p, [&](const Chunk &c) -> int {
        g.values = h->scratch.d_values.p; g.valid16 = h->scratch.d_valid16.p;
        g.base = c.base; g.start = c.start; g.end = c.end;
        CT_HIPCHK(hipMemsetAsync(h->d_long.p, 0, sizeof(uint64_t), h->stream));
        hipLaunchKernelGGL(kc_wave_kernel, dim3(grid_for(n_records, kWaveThreads / 64, (unsigned)h->n_cu * 8)), dim3(kWaveThreads), 0,
                           h->stream, g);
        CT_HIPCHK(hipGetLastError());
        h->n_launches++;
        if (may_be_long) {
            hipLaunchKernelGGL(kc_long_kernel, dim3((unsigned)h->n_cu * 4), dim3(kLongThreads), 0, h->stream, g);
            CT_HIPCHK(hipGetLastError());
            h->n_launches++;
        }
        return NTK_OK;
    });
    if (rc) return rc;
    BestArgs b;
    b.hits = d_hits; b.rows = d_rows; b.n_records = n_records; b.n_colors = h->n_colors;
    hipLaunchKernelGGL(kc_best_kernel, dim3(grid_for(n_records, kThreads, (unsigned)h->n_cu * 8)), dim3(kThreads), 0, h->stream, b);
    CT_HIPCHK(hipGetLastError());
    h->n_launches++;
    CT_HIPCHK(hipStreamSynchronize(h->stream));
    return NTK_OK;
}

}  // extern "C"
