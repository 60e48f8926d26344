// Per-read k-mer abundance against a count table (include/needletail_amd_abundance.h): one row per record with the number of k-mers,
// how many the table holds, and the min / median / max / sum of their counts.  A consumer of the public ABIs like the sketch: the
// k-mers are the values ntk_materialize_device_quality emits, their counts are ntk_kmer_table_lookup_device's, chunk by chunk into a
// batch-long count array and valid plane; then one reduction pass over the batch, which is this file's own device code.
//
// The reduction: a record's candidate windows are the window ends [offsets[r] + k - 1, offsets[r + 1] - 1) (a window never spans a break
// byte, and the record's last byte is its break byte); the valid plane says which of them were emitted.  ra_wave_kernel gives a wave
// to a record (grid-stride over the records), ra_block_kernel a 1024-thread block to each record of more than kLongRecord windows,
// which the wave kernel hands over through a device list.  Both fold n_kmers, n_present, min, max and sum in one pass, then SELECT the
// median rather than sort: with rank = n_kmers / 2, the median is the largest m with |{c < m}| <= rank, built bit by bit below the
// common prefix of min and max (a bit stays set when the count of values below the candidate does not exceed the rank).  That is one
// counting pass per bit in which min and max differ - a handful for real spectra, never more than 64 - over counts the wave holds in
// registers (up to kRegWindows windows) or re-reads through the caches.  DESIGN.md section 13.
#include "../../include/needletail_amd_abundance.h"
#include "ntk_consumer.hpp"

#include <new>

namespace {

constexpr int kWaveThreads = 256;                        // ra_wave_kernel: four records per block at a time
constexpr int kBlockThreads = 1024;                      // ra_block_kernel: one long record per block at a time
constexpr uint32_t kRegRounds = 3;                       // rounds of 64 windows a wave holds in registers
constexpr uint32_t kRegWindows = 64 * kRegRounds;        // 192: records up to here are read once
constexpr uint64_t kLongRecord = 65536;                  // records with more candidate windows go to ra_block_kernel
// Window ends a thread takes per round of a streaming pass.  A wave shares its CU with 31 others, which hide the latency of its loads: it
// skips a window end past the record (a conditional load, which the compiler completes before it issues the next).  A block streaming a
// long record has its CU alone, and bytes in flight are all that bounds it: it clamps such an end to the record's last one, so that its
// 16 loads go out back to back (a 75.5 M-base record: 138 ms against 375 ms with four conditional loads; the wave kernel is 10 - 28 %
// slower with clamped loads: profiles/abundance/README.md).
constexpr uint32_t kWaveInFlight = 4, kBlockInFlight = 16;

using Row = ntk_read_abundance_row;
static_assert(sizeof(Row) == 48, "the header states the row");

struct RaArgs {
    const uint64_t *counts;    // table count of the value at every window end of the batch (undefined where the plane says invalid)
    const uint16_t *plane;     // bit (15 - e % 16) of word e / 16: window e is emitted
    const uint64_t *offsets;   // n_records + 1 record starts
    uint64_t n_bytes, n_records;
    uint64_t min_count;        // >= 1
    uint32_t k;
    uint64_t *n_long;          // records handed to ra_block_kernel ...
    uint64_t *long_list;       // ... and their indices, at most long_cap
    uint64_t long_cap;
    Row *rows;
};

struct MinOp { __device__ uint64_t operator()(uint64_t x, uint64_t y) const { return x < y ? x : y; } };
struct MaxOp { __device__ uint64_t operator()(uint64_t x, uint64_t y) const { return x > y ? x : y; } };
struct AddOp { __device__ uint64_t operator()(uint64_t x, uint64_t y) const { return x + y; } };

template <class Op>
__device__ inline uint64_t wave_fold(uint64_t v, Op op)
{
    for (int off = 32; off > 0; off >>= 1) v = op(v, __shfl_xor(v, off, 64));
    return v;
}

// the threads that share a record: a wave ...
struct WaveGroup {
    static constexpr uint32_t kStride = 64, kInFlight = kWaveInFlight;
    static constexpr bool kClamp = false;
    uint32_t tid;
    template <class Op> __device__ uint64_t fold(uint64_t v, Op op) const { return uniform(wave_fold(v, op)); }
};

// ... or a block (every thread of the block calls fold)
struct BlockGroup {
    static constexpr uint32_t kStride = kBlockThreads, kInFlight = kBlockInFlight;
    static constexpr bool kClamp = true;
    uint32_t tid;
    uint64_t *lds;   // kBlockThreads / 64 words
    template <class Op> __device__ uint64_t fold(uint64_t v, Op op) const
    {
        v = wave_fold(v, op);
        __syncthreads();   // the words are free again
        if ((tid & 63) == 0) lds[tid >> 6] = v;
        __syncthreads();
        uint64_t s = lds[0];
        for (int w = 1; w < kBlockThreads / 64; w++) s = op(s, lds[w]);
        return uniform(s);
    }
};

// the bits in which min and max differ decide the median; the prefix above them is common to every count
__device__ inline int select_start(uint64_t mn, uint64_t mx, uint64_t &prefix)
{
    const int top = 63 - __builtin_clzll(mn ^ mx);   // mn != mx
    prefix = top == 63 ? 0 : (mx >> (top + 1)) << (top + 1);
    return top;
}

__device__ inline bool plane_bit(uint16_t word, uint64_t e) { return (word >> (15 - (e & 15))) & 1u; }

// f(count) for every emitted window of [lo, hi), lo < hi, that falls to this thread of the group: kInFlight window ends per round, each a
// coalesced 8-byte load across the wave with its plane word (kClamp: above).
template <class G, class F>
__device__ inline void for_windows(const RaArgs &a, uint64_t lo, uint64_t hi, const G &g, F f)
{
    constexpr uint32_t kInFlight = G::kInFlight;
    for (uint64_t e0 = lo + g.tid; e0 < hi; e0 += (uint64_t)G::kStride * kInFlight) {
        uint64_t v[kInFlight];
        bool ok[kInFlight];
        if constexpr (G::kClamp) {
            uint16_t w[kInFlight];
#pragma unroll
            for (uint32_t u = 0; u < kInFlight; u++) {
                const uint64_t e = e0 + (uint64_t)u * G::kStride, at = e < hi ? e : hi - 1;
                v[u] = a.counts[at];
                w[u] = a.plane[at >> 4];
            }
#pragma unroll
            for (uint32_t u = 0; u < kInFlight; u++) {
                const uint64_t e = e0 + (uint64_t)u * G::kStride;
                ok[u] = e < hi && plane_bit(w[u], e);
            }
        } else {
#pragma unroll
            for (uint32_t u = 0; u < kInFlight; u++) {
                const uint64_t e = e0 + (uint64_t)u * G::kStride;
                ok[u] = e < hi;
                v[u] = ok[u] ? a.counts[e] : 0;
                ok[u] = ok[u] && plane_bit(a.plane[e >> 4], e);
            }
        }
#pragma unroll
        for (uint32_t u = 0; u < kInFlight; u++)
            if (ok[u]) f(v[u]);
    }
}

// A record streamed by the group's threads: one pass for the five folds, then one per undecided bit of the median.
template <class G>
__device__ inline Row stream_row(const RaArgs &a, uint64_t lo, uint64_t hi, const G &g)
{
    Row row;
    row.n_kmers = row.n_present = row.min = row.median = row.max = row.sum = 0;
    if (lo == hi) return row;
    uint64_t n = 0, present = 0, mn = ~(uint64_t)0, mx = 0, sum = 0;
    for_windows(a, lo, hi, g, [&](uint64_t v) __attribute__((always_inline)) {
        n++;
        present += v >= a.min_count;
        mn = v < mn ? v : mn;
        mx = v > mx ? v : mx;
        sum += v;
    });
    row.n_kmers = g.fold(n, AddOp());
    row.n_present = g.fold(present, AddOp());
    row.min = g.fold(mn, MinOp());
    row.max = g.fold(mx, MaxOp());
    row.sum = g.fold(sum, AddOp());
    if (row.n_kmers == 0) { row.min = 0; row.median = 0; return row; }
    row.median = row.min;
    if (row.min == row.max) return row;
    const uint64_t rank = row.n_kmers / 2;
    uint64_t ans;
    for (int b = select_start(row.min, row.max, ans); b >= 0; b--) {
        const uint64_t cand = ans | ((uint64_t)1 << b);
        uint64_t below = 0;
        for_windows(a, lo, hi, g, [&](uint64_t v) __attribute__((always_inline)) { below += v < cand; });
        if (g.fold(below, AddOp()) <= rank) ans = cand;
    }
    row.median = ans;
    return row;
}

// A record of at most kRegWindows candidate windows, read once by a wave: lane l holds windows l, l + 64, l + 128.  The counts of
// windows and of values below a candidate are ballots, so the selection costs a compare and a scalar popcount per round and bit.
__device__ inline Row register_row(const RaArgs &a, uint64_t lo, uint64_t hi, uint32_t lane)
{
    Row row;
    row.n_kmers = row.n_present = row.min = row.median = row.max = row.sum = 0;
    uint64_t v[kRegRounds];
    bool ok[kRegRounds];
#pragma unroll
    for (uint32_t u = 0; u < kRegRounds; u++) {
        const uint64_t e = lo + u * 64 + lane;
        ok[u] = e < hi;
        v[u] = ok[u] ? a.counts[e] : 0;
        ok[u] = ok[u] && plane_bit(a.plane[e >> 4], e);
    }
    uint64_t n = 0, present = 0, mn = ~(uint64_t)0, mx = 0, sum = 0;
#pragma unroll
    for (uint32_t u = 0; u < kRegRounds; u++) {
        n += __popcll(__ballot(ok[u]));
        present += __popcll(__ballot(ok[u] && v[u] >= a.min_count));
        if (ok[u]) {
            mn = v[u] < mn ? v[u] : mn;
            mx = v[u] > mx ? v[u] : mx;
            sum += v[u];
        }
    }
    row.n_kmers = n;
    row.n_present = present;
    if (n == 0) return row;
    row.min = uniform(wave_fold(mn, MinOp()));
    row.max = uniform(wave_fold(mx, MaxOp()));
    row.sum = uniform(wave_fold(sum, AddOp()));
    row.median = row.min;
    if (row.min == row.max) return row;
    const uint64_t rank = n / 2;
    uint64_t ans;
    for (int b = select_start(row.min, row.max, ans); b >= 0; b--) {
        const uint64_t cand = ans | ((uint64_t)1 << b);
        uint64_t below = 0;
#pragma unroll
        for (uint32_t u = 0; u < kRegRounds; u++) below += __popcll(__ballot(ok[u] && v[u] < cand));
        if (below <= rank) ans = cand;
    }
    row.median = ans;
    return row;
}

// One wave per record, grid-stride over the records.  A record of more than kLongRecord candidate windows is appended to the long list
// (one atomic) and left to ra_block_kernel.
__global__ __launch_bounds__(kWaveThreads) void ra_wave_kernel(RaArgs a)
{
    const uint32_t lane = threadIdx.x & 63;
    const uint64_t waves = (uint64_t)gridDim.x * (kWaveThreads / 64);
    const uint64_t first = (uint64_t)blockIdx.x * (kWaveThreads / 64) + __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    for (uint64_t r = first; r < a.n_records; r += waves) {
        uint64_t lo, hi;
        record_span(a.offsets, a.n_bytes, a.k, r, lo, hi);
        const uint64_t span = hi - lo;
        if (span > kLongRecord) {
            if (lane == 0) {
                const uint64_t at = __hip_atomic_fetch_add(a.n_long, (uint64_t)1, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
                if (at < a.long_cap) a.long_list[at] = r;
            }
            continue;
        }
        const Row row = span <= kRegWindows ? register_row(a, lo, hi, lane) : stream_row(a, lo, hi, WaveGroup{lane});
        if (lane == 0) a.rows[r] = row;
    }
}

// One block per long record, a fixed grid walking the list ra_wave_kernel left (its length is read here, on the device).
__global__ __launch_bounds__(kBlockThreads) void ra_block_kernel(RaArgs a)
{
    __shared__ uint64_t lds[kBlockThreads / 64];
    uint64_t n_long = *a.n_long;
    if (n_long > a.long_cap) n_long = a.long_cap;
    for (uint64_t i = blockIdx.x; i < n_long; i += gridDim.x) {
        const uint64_t r = a.long_list[i];
        uint64_t lo, hi;
        record_span(a.offsets, a.n_bytes, a.k, r, lo, hi);
        const Row row = stream_row(a, lo, hi, BlockGroup{threadIdx.x, lds});
        if (threadIdx.x == 0) a.rows[r] = row;
    }
}

}  // namespace

struct ntk_read_abundance : Consumer {   // k and path: the table's
    ntk_kmer_table *table = nullptr;   // borrowed
    MaterialiseScratch scratch;        // of one chunk
    // batch-long, grown on demand
    DeviceArray<uint64_t> d_counts;    // 8 B per base
    DeviceArray<uint16_t> d_plane;     // 1/8 B per base
    DeviceArray<uint64_t> d_long;      // [0]: the number of long records, then their indices (one per kLongRecord bases at most)

    uint64_t long_cap() const { return d_long.cap - 1; }

    void release_batch() { d_counts.release(); d_plane.release(); d_long.release(); }

    int ensure_batch(uint64_t n_bytes)
    {
        const uint64_t need = (n_bytes + 15) & ~(uint64_t)15;   // bases (a multiple of 16)
        int rc = d_counts.ensure(stream, need, grow_exact);
        if (!rc) rc = d_plane.ensure(stream, need / 16, grow_exact);
        if (!rc) rc = d_long.ensure(stream, (need >> 16) + 2, grow_exact);
        return rc;
    }
};

extern "C" {

int ntk_read_abundance_create(ntk_ctx *ctx, ntk_kmer_table *table, ntk_read_abundance **out)
{
    if (!ctx || !table || !out) return NTK_ERR_BAD_ARG;
    *out = nullptr;
    ntk_read_abundance *a = new (std::nothrow) ntk_read_abundance();
    if (!a) return NTK_ERR_NOMEM;
    struct ntk_kmer_table_stats st;
    int rc = ntk_kmer_table_stats(table, &st);
    if (!rc) rc = a->bind(ctx, st.k, st.path);
    if (rc) { delete a; return rc; }
    a->table = table;
    *out = a;
    return NTK_OK;
}

int ntk_read_abundance_trim(ntk_read_abundance *a)
{
    if (!a) return NTK_ERR_BAD_ARG;
    CT_HIPCHK(hipSetDevice(a->device));
    CT_HIPCHK(hipStreamSynchronize(a->stream));
    a->scratch.release();
    a->release_batch();
    (void)hipGetLastError();
    return NTK_OK;
}

void ntk_read_abundance_destroy(ntk_read_abundance *a)
{
    if (!a) return;
    (void)ntk_read_abundance_trim(a);
    delete a;
}

int ntk_read_abundance_run_device(ntk_read_abundance *a, const uint8_t *d_seq, const uint8_t *d_qual, uint64_t n_bytes,
                                  const uint64_t *d_offsets, uint64_t n_records, const ntk_params *p, uint64_t min_count,
                                  struct ntk_read_abundance_row *d_rows)
{
    int rc = check_batch_params(a, p);
    if (rc || n_records == 0 || n_bytes == 0) return rc;
    if ((rc = check_batch_pointers(d_seq, d_qual))) return rc;
    if (!d_offsets || !d_rows || ((uintptr_t)d_offsets & 7) || ((uintptr_t)d_rows & 7)) return NTK_ERR_BAD_ARG;
    CT_HIPCHK(hipSetDevice(a->device));
    if ((rc = a->ensure_batch(n_bytes))) return rc;
    // Of every chunk only the values and the plane words from its start on are taken, so the halo's partial windows never replace a good
    // word of the chunk before.
    rc = for_each_chunk(*a, a->scratch, d_seq, d_qual, n_bytes, p, [&](const Chunk &c) -> int {
        // values at invalid positions are undefined: looking them up is a bounded read-only probe, and the plane drops their counts.
        // An incomplete table fails here, on the first chunk, before any row is written.  Synchronises.
        const int rc = ntk_kmer_table_lookup_device(a->table, a->scratch.d_values.p + c.skip(), c.end - c.start, a->d_counts.p + c.start);
        if (rc) return rc;
        CT_HIPCHK(hipSetDevice(a->device));
        CT_HIPCHK(hipMemcpyAsync(a->d_plane.p + c.start / 16, a->scratch.d_valid16.p + c.skip() / 16,
                                 (c.end - c.start + 15) / 16 * sizeof(uint16_t), hipMemcpyDeviceToDevice, a->stream));
        return NTK_OK;
    });
    if (rc) return rc;
    RaArgs g;
    g.counts = a->d_counts.p; g.plane = a->d_plane.p; g.offsets = d_offsets;
    g.n_bytes = n_bytes; g.n_records = n_records;
    g.min_count = min_count ? min_count : 1;
    g.k = a->k;
    g.n_long = a->d_long.p; g.long_list = a->d_long.p + 1; g.long_cap = a->long_cap();
    g.rows = d_rows;
    CT_HIPCHK(hipMemsetAsync(a->d_long.p, 0, sizeof(uint64_t), a->stream));
    hipLaunchKernelGGL(ra_wave_kernel, dim3(grid_for(n_records, kWaveThreads / 64, (unsigned)a->n_cu * 8)), dim3(kWaveThreads), 0,
                       a->stream, g);
    CT_HIPCHK(hipGetLastError());
    if (n_bytes > kLongRecord) {   // only then can a record be long; whether one is, the device alone knows
        hipLaunchKernelGGL(ra_block_kernel, dim3((unsigned)a->n_cu), dim3(kBlockThreads), 0, a->stream, g);
        CT_HIPCHK(hipGetLastError());
    }
    CT_HIPCHK(hipStreamSynchronize(a->stream));
    return NTK_OK;
}

}  // extern "C"
