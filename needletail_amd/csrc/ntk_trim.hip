// Trimming reads by k-mer abundance and writing the kept reads out as a batch (include/needletail_amd_trim.h).  A consumer of the
// public ABIs like the abundance library: per chunk of the batch (for_each_chunk of ntk_consumer.hpp, taking only what ends at or after
// the chunk's start) the k-mers are the values ntk_materialize_device_quality emits and their counts are
// ntk_kmer_table_lookup_device's, into a CHUNK-long count array.  This file's own device code:
//
//   rt_solid_kernel     one lane per window end of the chunk: ballot(valid && count >= min_count) is one 64-bit word of the batch-long
//                       solid plane per wave round, ballot(valid) one word of the valid plane.  The counts are read once and never kept.
//   rt_interval_kernel  a record's bit range of the planes -> its row.  The run search is the monoid of ntk_trim_runs.hpp over 64-bit
//                       words: folded across the kGroup lanes that share a short record by shuffles, or across a whole wave, round
//                       after round with a carry, for a long one (the same streaming code at both widths).
//   rt_copy_kernel      after an exclusive scan over the records (rocPRIM) of the bytes and records they write: moves the kept bytes,
//                       16 lanes per record, one 16-byte piece of the DESTINATION per lane and step: an aligned 16-byte store from an
//                       unaligned 16-byte load; the pieces at a record's two ends, which it shares with its neighbours, byte by byte.
//   rt_copy_long_kernel the records of more than kLongPieces pieces, which rt_copy_kernel lists: the whole grid on each.
//
// Plane layout: bit e % 64 of word e / 64 is the window that ends at batch byte e.  DESIGN.md section 14.
#include "../../include/needletail_amd_trim.h"
#include "ntk_consumer.hpp"
#include "ntk_trim_runs.hpp"

#include <new>
#include <rocprim/device/device_scan.hpp>
#include <rocprim/iterator/counting_iterator.hpp>
#include <rocprim/iterator/transform_iterator.hpp>

namespace {

constexpr int kSolidThreads = 256;                       // rt_solid_kernel: a wave takes kSolidRounds * 64 window ends at a time
constexpr uint32_t kSolidRounds = 4;                     // 8-byte count loads a lane has in flight
constexpr int kIntervalThreads = 256;
constexpr uint32_t kGroup = 8;                           // lanes that share a short record in rt_interval_kernel
constexpr uint32_t kGroupRounds = 4;                     // a record of more than kGroup * kGroupRounds plane words goes to the whole wave
constexpr int kCopyThreads = 256;
constexpr uint32_t kCopyGroup = 16;                      // lanes that share a record in rt_copy_kernel
constexpr uint64_t kLongPieces = 2048;                   // a record of more 16-byte pieces goes to rt_copy_long_kernel

using Row = ntk_read_trim_row;
static_assert(sizeof(Row) == 32, "the header states the row");

// ---- the solid and valid planes of one chunk -------------------------------------------------------------------------------------------

struct SolidArgs {
    const uint64_t *counts;    // table count of the value at window end i of the chunk (undefined where invalid)
    const uint16_t *valid16;   // the materialise face's plane from the chunk's start: bit (15 - i % 16) of word i / 16
    uint64_t n;                // window ends of the chunk, > 0
    uint64_t min_count;        // >= 1
    uint64_t *solid, *valid;   // the planes' words from the chunk's start: (n + 63) / 64 each
};

// A window end past the chunk is clamped to its last one, so that a lane's loads go out back to back (a conditional load is completed
// before the next is issued: DESIGN.md section 13), and masked out of the ballots.
__global__ __launch_bounds__(kSolidThreads) void rt_solid_kernel(SolidArgs a)
{
    const uint32_t lane = threadIdx.x & 63;
    constexpr uint64_t kTile = 64 * kSolidRounds;
    const uint64_t tiles = (a.n + kTile - 1) / kTile, words = (a.n + 63) / 64;
    const uint64_t stride = (uint64_t)gridDim.x * (kSolidThreads / 64);
    for (uint64_t tile = (uint64_t)blockIdx.x * (kSolidThreads / 64) + __builtin_amdgcn_readfirstlane(threadIdx.x >> 6); tile < tiles;
         tile += stride) {
        uint64_t c[kSolidRounds];
        uint16_t w[kSolidRounds];
#pragma unroll
        for (uint32_t u = 0; u < kSolidRounds; u++) {
            const uint64_t i = tile * kTile + u * 64 + lane, at = i < a.n ? i : a.n - 1;
            c[u] = a.counts[at];
            w[u] = a.valid16[at >> 4];
        }
        uint64_t sw = 0, vw = 0;   // lane u keeps the words of round u
#pragma unroll
        for (uint32_t u = 0; u < kSolidRounds; u++) {
            const uint64_t i = tile * kTile + u * 64 + lane;
            const bool ok = i < a.n && ((w[u] >> (15 - (i & 15))) & 1u);
            const uint64_t v = __ballot(ok), s = __ballot(ok && c[u] >= a.min_count);
            if (lane == u) { vw = v; sw = s; }
        }
        const uint64_t word = tile * kSolidRounds + lane;
        if (lane < kSolidRounds && word < words) {
            a.solid[word] = sw;
            a.valid[word] = vw;
        }
    }
}

// ---- a record's row from its bit range of the planes ------------------------------------------------------------------------------------

struct IntervalArgs {
    const uint64_t *solid, *valid;   // batch-long planes
    const uint64_t *offsets;         // n_records + 1 record starts
    uint64_t n_bytes, n_records;
    uint64_t min_length;
    uint32_t k, prefix;
    Row *rows;
};

template <uint32_t G>
__device__ inline RtRuns shuffle_down(const RtRuns &v, uint32_t off)
{
    RtRuns o;
    o.len = __shfl_down(v.len, off, G);
    o.lead = __shfl_down(v.lead, off, G);
    o.trail = __shfl_down(v.trail, off, G);
    o.best = __shfl_down(v.best, off, G);
    o.best_pos = __shfl_down(v.best_pos, off, G);
    return o;
}

// The row of the bit range [lo, hi), by the G lanes (`sub` = 0 .. G - 1 among them) that share it: lane sub takes plane word
// first + sub of every round of G words; the words' summaries are folded in order towards lane 0 (lane i combines its own with that of
// lane i + off, off = 1, 2, 4 ..: a lane without a partner takes the identity) and appended to the carry of the rounds before.  Every
// lane of the group returns, lane 0 with the row.
template <uint32_t G>
__device__ inline Row range_row(const IntervalArgs &a, uint64_t lo, uint64_t hi, uint32_t sub)
{
    RtRuns carry;
    uint64_t n_valid = 0, n_solid = 0;
    if (lo < hi) {
        const uint64_t w_end = ((hi - 1) >> 6) + 1;
        for (uint64_t w0 = lo >> 6; w0 < w_end; w0 += G) {
            const uint64_t w = w0 + sub;
            RtRuns e;
            if (w < w_end) {
                const uint64_t first = w * 64 > lo ? w * 64 : lo, end = w * 64 + 64 < hi ? w * 64 + 64 : hi;
                const uint32_t n = (uint32_t)(end - first);
                const uint64_t mask = n < 64 ? (((uint64_t)1 << n) - 1) : ~(uint64_t)0;
                const uint64_t s = (a.solid[w] >> (first - w * 64)) & mask, v = (a.valid[w] >> (first - w * 64)) & mask;
                n_solid += __popcll(s);
                n_valid += __popcll(v);
                e = rt_word_runs(s, n);
            }
#pragma unroll
            for (uint32_t off = 1; off < G; off <<= 1) {
                RtRuns o = shuffle_down<G>(e, off);
                if (sub + off >= G) o = RtRuns();
                e = rt_combine(e, o);
            }
            carry = rt_combine(carry, e);
        }
    }
#pragma unroll
    for (uint32_t off = G / 2; off > 0; off >>= 1) {
        n_valid += __shfl_xor(n_valid, off, G);
        n_solid += __shfl_xor(n_solid, off, G);
    }
    Row row;
    rt_interval(carry, a.prefix != 0, a.k, a.min_length, row.start, row.length);
    row.n_kmers = n_valid;
    row.n_solid = n_solid;
    return row;
}

// kGroup lanes per record, 64 / kGroup records per wave and step, grid-stride over the records.  The records of a step that are too
// long for a group are then taken one after the other by the whole wave.
__global__ __launch_bounds__(kIntervalThreads) void rt_interval_kernel(IntervalArgs a)
{
    constexpr uint32_t kPerWave = 64 / kGroup;
    const uint32_t lane = threadIdx.x & 63, sub = lane % kGroup, grp = lane / kGroup;
    const uint64_t waves = (uint64_t)gridDim.x * (kIntervalThreads / 64);
    const uint64_t first = (uint64_t)blockIdx.x * (kIntervalThreads / 64) + __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    for (uint64_t r0 = first * kPerWave; r0 < a.n_records; r0 += waves * kPerWave) {
        const uint64_t r = r0 + grp;
        const bool have = r < a.n_records;
        uint64_t lo = 0, hi = 0;
        if (have) record_span(a.offsets, a.n_bytes, a.k, r, lo, hi);
        const uint64_t words = lo < hi ? ((hi - 1) >> 6) - (lo >> 6) + 1 : 0;
        const bool is_long = words > kGroup * kGroupRounds;
        if (have && !is_long) {
            const Row row = range_row<kGroup>(a, lo, hi, sub);
            if (sub == 0) a.rows[r] = row;
        }
        uint64_t todo = __ballot(have && is_long && sub == 0);
        while (todo) {
            const uint32_t src = (uint32_t)__builtin_ctzll(todo);
            todo &= todo - 1;
            const uint64_t l_lo = uniform(__shfl(lo, src, 64)), l_hi = uniform(__shfl(hi, src, 64));
            const Row row = range_row<64>(a, l_lo, l_hi, lane);
            if (lane == 0) a.rows[r0 + src / kGroup] = row;
        }
    }
}

// ---- the compaction --------------------------------------------------------------------------------------------------------------------

struct ScanItem {
    uint64_t bytes, records;   // written before this record
};

struct ScanAdd {
    __host__ __device__ ScanItem operator()(const ScanItem &x, const ScanItem &y) const
    {
        return ScanItem{x.bytes + y.bytes, x.records + y.records};
    }
};

struct Batch {
    const uint64_t *offsets;
    const Row *rows;
    uint64_t n_bytes, n_records;
};

// The kept bytes of record r: [at, at + len) of the batch; brk = the record's break byte.  A row that reaches beyond the record's L
// bytes is clamped: start to L, then length to L - start.
__device__ inline void kept_span(const Batch &b, uint64_t r, uint64_t &at, uint64_t &len, uint64_t &brk)
{
    uint64_t s = b.offsets[r], e = b.offsets[r + 1];
    if (e > b.n_bytes) e = b.n_bytes;
    if (s > e) s = e;
    const uint64_t L = e > s ? e - s - 1 : 0;
    const Row row = b.rows[r];
    const uint64_t start = row.start < L ? row.start : L;
    len = row.length < L - start ? row.length : L - start;
    at = s + start;
    brk = s + L;
}

// what record r writes; nothing for r = n_records, whose scanned item is the total
struct KeptItem {
    Batch b;
    __device__ ScanItem operator()(uint64_t r) const
    {
        if (r >= b.n_records) return ScanItem{0, 0};
        uint64_t at, len, brk;
        kept_span(b, r, at, len, brk);
        return len ? ScanItem{len + 1, 1} : ScanItem{0, 0};
    }
};

struct CopyArgs {
    Batch b;
    const ScanItem *scan;      // n_records + 1
    const uint8_t *src;        // d_seq, or d_aux
    uint8_t *dst;
    uint64_t src_readable;     // round_up(n_bytes, 16)
    uint32_t aux;              // the break byte is copied from the source record's, not written as '\n'
    uint32_t first;            // the launch for d_seq: it writes the offsets and sources and makes the list, which stands for d_aux
    uint64_t *out_offsets, *out_source;
    uint64_t total_bytes, total_records;
    uint64_t *n_long;          // records left to rt_copy_long_kernel ...
    uint64_t *long_list;       // ... and their indices, at most long_cap
    uint64_t long_cap;
};

struct Span {
    uint64_t at, len, brk;   // kept_span
    uint64_t d0;             // the first byte written
    uint64_t pieces;         // 16-byte pieces of the destination that [d0, d0 + len] touches
};

__device__ inline Span output_span(const CopyArgs &a, uint64_t r)
{
    Span s;
    kept_span(a.b, r, s.at, s.len, s.brk);
    s.d0 = a.scan[r].bytes;
    s.pieces = s.len ? ((s.d0 + s.len) >> 4) - (s.d0 >> 4) + 1 : 0;
    return s;
}

__device__ inline uint4 load16_unaligned(const uint8_t *p)
{
    uint4 v;
    __builtin_memcpy(&v, p, 16);
    return v;
}

// Piece p of a record's output: the 16 destination bytes from P = (d0 & ~15) + 16 p.  Wholly inside the kept bytes: one unaligned
// 16-byte load and one aligned 16-byte store.  Otherwise (the record's first or last piece, which the neighbours write too): the
// bytes that are this record's, from one 16-byte load where the source is readable that far, and the break byte.
__device__ inline void copy_piece(const CopyArgs &a, const Span &s, uint64_t p)
{
    const uint64_t P = (s.d0 & ~(uint64_t)15) + 16 * p, end = s.d0 + s.len;   // end: where the break byte goes
    const uint64_t lo = P > s.d0 ? P : s.d0, hi = P + 16 < end ? P + 16 : end;
    if (lo == P && hi == P + 16) {
        *reinterpret_cast<uint4 *>(a.dst + P) = load16_unaligned(a.src + s.at + (P - s.d0));
        return;
    }
    if (lo < hi) {
        const uint32_t cnt = (uint32_t)(hi - lo);
        const uint64_t from = s.at + (lo - s.d0);
        if (from + 16 <= a.src_readable) {
            const uint4 v = load16_unaligned(a.src + from);
            const uint32_t w[4] = {v.x, v.y, v.z, v.w};
#pragma unroll
            for (uint32_t j = 0; j < 15; j++)
                if (j < cnt) a.dst[lo + j] = (uint8_t)(w[j >> 2] >> (8 * (j & 3)));
        } else {
            for (uint32_t j = 0; j < cnt; j++) a.dst[lo + j] = a.src[from + j];
        }
    }
    if (end >= P && end < P + 16) a.dst[end] = a.aux ? a.src[s.brk] : (uint8_t)'\n';
}

// kCopyGroup lanes per kept record, grid-stride over the records; also the output's offsets and sources, its last offset and its
// padding.  A record of more than kLongPieces pieces is listed for rt_copy_long_kernel.
__global__ __launch_bounds__(kCopyThreads) void rt_copy_kernel(CopyArgs a)
{
    constexpr uint32_t kPerBlock = kCopyThreads / kCopyGroup;
    const uint32_t sub = threadIdx.x % kCopyGroup, grp = threadIdx.x / kCopyGroup;
    if (blockIdx.x == 0) {
        if (threadIdx.x == 0 && a.first) a.out_offsets[a.total_records] = a.total_bytes;
        if (threadIdx.x < 16 && a.total_bytes + threadIdx.x < ((a.total_bytes + 15) & ~(uint64_t)15))
            a.dst[a.total_bytes + threadIdx.x] = (uint8_t)'\n';
    }
    for (uint64_t r = (uint64_t)blockIdx.x * kPerBlock + grp; r < a.b.n_records; r += (uint64_t)gridDim.x * kPerBlock) {
        const Span s = output_span(a, r);
        if (s.len == 0) continue;
        if (sub == 0 && a.first) {
            const uint64_t i = a.scan[r].records;
            a.out_offsets[i] = s.d0;
            a.out_source[i] = r;
        }
        if (s.pieces > kLongPieces) {
            if (sub == 0 && a.first) {
                const uint64_t at = __hip_atomic_fetch_add(a.n_long, (uint64_t)1, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
                if (at < a.long_cap) a.long_list[at] = r;
            }
            continue;
        }
        for (uint64_t p = sub; p < s.pieces; p += kCopyGroup) copy_piece(a, s, p);
    }
}

// every listed record by the whole grid, consecutive threads on consecutive pieces (the list's length is read here, on the device)
__global__ __launch_bounds__(kCopyThreads) void rt_copy_long_kernel(CopyArgs a)
{
    uint64_t n_long = *a.n_long;
    if (n_long > a.long_cap) n_long = a.long_cap;
    const uint64_t stride = (uint64_t)gridDim.x * kCopyThreads;
    for (uint64_t i = 0; i < n_long; i++) {
        const Span s = output_span(a, a.long_list[i]);
        for (uint64_t p = (uint64_t)blockIdx.x * kCopyThreads + threadIdx.x; p < s.pieces; p += stride) copy_piece(a, s, p);
    }
}

}  // namespace

struct ntk_read_trim : Consumer {        // k and path: the table's
    ntk_kmer_table *table = nullptr;   // borrowed
    MaterialiseScratch scratch;        // of one chunk
    DeviceArray<uint64_t> d_counts;    // 8 B per base of one chunk (a multiple of 16 bases, at most kChunkBases)
    DeviceArray<uint64_t> d_solid, d_valid;   // the planes: one word per 64 bases of the batch each
    // the compaction's
    DeviceArray<ScanItem> d_scan;
    DeviceArray<char> d_scan_tmp;
    DeviceArray<uint64_t> d_long;      // [0]: the number of long records, then their indices

    void release_all()
    {
        scratch.release();
        d_counts.release(); d_solid.release(); d_valid.release();
        d_scan.release(); d_scan_tmp.release(); d_long.release();
    }
};

namespace {

uint64_t planes_words(uint64_t n_bytes) { return (n_bytes + 63) / 64 + 1; }

}  // namespace

extern "C" {

int ntk_read_trim_create(ntk_ctx *ctx, ntk_kmer_table *table, ntk_read_trim **out)
{
    if (!ctx || !table || !out) return NTK_ERR_BAD_ARG;
    *out = nullptr;
    ntk_read_trim *t = new (std::nothrow) ntk_read_trim();
    if (!t) return NTK_ERR_NOMEM;
    struct ntk_kmer_table_stats st;
    int rc = ntk_kmer_table_stats(table, &st);
    if (!rc) rc = t->bind(ctx, st.k, st.path);
    if (rc) { delete t; return rc; }
    t->table = table;
    *out = t;
    return NTK_OK;
}

int ntk_read_trim_release(ntk_read_trim *t)
{
    if (!t) return NTK_ERR_BAD_ARG;
    CT_HIPCHK(hipSetDevice(t->device));
    CT_HIPCHK(hipStreamSynchronize(t->stream));
    t->release_all();
    (void)hipGetLastError();
    return NTK_OK;
}

void ntk_read_trim_destroy(ntk_read_trim *t)
{
    if (!t) return;
    (void)ntk_read_trim_release(t);
    delete t;
}

int ntk_read_trim_run_device(ntk_read_trim *t, const uint8_t *d_seq, const uint8_t *d_qual, uint64_t n_bytes,
                             const uint64_t *d_offsets, uint64_t n_records, const ntk_params *p, uint64_t min_count, uint32_t mode,
                             uint64_t min_length, struct ntk_read_trim_row *d_rows)
{
    if (mode != NTK_TRIM_PREFIX && mode != NTK_TRIM_LONGEST) return NTK_ERR_BAD_ARG;
    int rc = check_batch_params(t, p);
    if (rc || n_records == 0 || n_bytes == 0) return rc;
    if ((rc = check_batch_pointers(d_seq, d_qual))) return rc;
    if (!d_offsets || !d_rows || ((uintptr_t)d_offsets & 7) || ((uintptr_t)d_rows & 7)) return NTK_ERR_BAD_ARG;
    CT_HIPCHK(hipSetDevice(t->device));
    if ((rc = t->d_counts.ensure(t->stream, (chunk_bases(n_bytes) + 15) & ~(uint64_t)15, grow_exact)) ||
        (rc = t->d_solid.ensure(t->stream, planes_words(n_bytes), grow_exact)) ||
        (rc = t->d_valid.ensure(t->stream, planes_words(n_bytes), grow_exact)))
        return rc;
    // the counts of a chunk are turned into plane words before the next chunk's replace them
    rc = for_each_chunk(*t, t->scratch, d_seq, d_qual, n_bytes, p, [&](const Chunk &c) -> int {
        // values at invalid positions are undefined: looking them up is a bounded read-only probe, and the valid bit drops their counts.
        // An incomplete table fails here, on the first chunk, before any row is written.  Synchronises.
        const int rc = ntk_kmer_table_lookup_device(t->table, t->scratch.d_values.p + c.skip(), c.end - c.start, t->d_counts.p);
        if (rc) return rc;
        CT_HIPCHK(hipSetDevice(t->device));
        SolidArgs g;
        g.counts = t->d_counts.p; g.valid16 = t->scratch.d_valid16.p + c.skip() / 16;
        g.n = c.end - c.start; g.min_count = min_count ? min_count : 1;
        g.solid = t->d_solid.p + c.start / 64; g.valid = t->d_valid.p + c.start / 64;
        hipLaunchKernelGGL(rt_solid_kernel, dim3(grid_for(g.n, 64 * kSolidRounds * (kSolidThreads / 64), (unsigned)t->n_cu * 8)),
                           dim3(kSolidThreads), 0, t->stream, g);
        CT_HIPCHK(hipGetLastError());
        return NTK_OK;
    });
    if (rc) return rc;
    IntervalArgs g;
    g.solid = t->d_solid.p; g.valid = t->d_valid.p; g.offsets = d_offsets;
    g.n_bytes = n_bytes; g.n_records = n_records; g.min_length = min_length;
    g.k = t->k; g.prefix = mode == NTK_TRIM_PREFIX;
    g.rows = d_rows;
    hipLaunchKernelGGL(rt_interval_kernel, dim3(grid_for(n_records, (64 / kGroup) * (kIntervalThreads / 64), (unsigned)t->n_cu * 8)),
                       dim3(kIntervalThreads), 0, t->stream, g);
    CT_HIPCHK(hipGetLastError());
    CT_HIPCHK(hipStreamSynchronize(t->stream));
    return NTK_OK;
}

int ntk_read_trim_compact_device(ntk_read_trim *t, const uint8_t *d_seq, const uint8_t *d_aux, uint64_t n_bytes,
                                 const uint64_t *d_offsets, uint64_t n_records, const struct ntk_read_trim_row *d_rows,
                                 uint8_t *d_out_seq, uint8_t *d_out_aux, uint64_t out_cap_bytes, uint64_t *d_out_offsets,
                                 uint64_t *d_out_source, uint64_t out_cap_records, uint64_t *out_n_bytes, uint64_t *out_n_records)
{
    if (!t || !out_n_bytes || !out_n_records) return NTK_ERR_BAD_ARG;
    *out_n_bytes = 0;
    *out_n_records = 0;
    if (out_cap_bytes && !d_aux != !d_out_aux) return NTK_ERR_BAD_ARG;
    if (((uintptr_t)d_seq & 15) || ((uintptr_t)d_aux & 15) || ((uintptr_t)d_out_seq & 15) || ((uintptr_t)d_out_aux & 15) ||
        ((uintptr_t)d_offsets & 7) || ((uintptr_t)d_rows & 7) || ((uintptr_t)d_out_offsets & 7) || ((uintptr_t)d_out_source & 7))
        return NTK_ERR_BAD_ARG;
    if ((out_cap_bytes && !d_out_seq) || (out_cap_records && (!d_out_offsets || !d_out_source))) return NTK_ERR_BAD_ARG;
    CT_HIPCHK(hipSetDevice(t->device));
    if (n_records == 0 || n_bytes == 0) {
        if (d_out_offsets) CT_HIPCHK(hipMemsetAsync(d_out_offsets, 0, sizeof(uint64_t), t->stream));
        CT_HIPCHK(hipStreamSynchronize(t->stream));
        return NTK_OK;
    }
    if (!d_seq || !d_offsets || !d_rows) return NTK_ERR_BAD_ARG;
    // the exclusive scan of what every record writes; item n_records is the total
    const Batch b{d_offsets, d_rows, n_bytes, n_records};
    auto items = rocprim::make_transform_iterator(rocprim::counting_iterator<uint64_t>(0), KeptItem{b});
    int rc = t->d_scan.ensure(t->stream, n_records + 1, grow_exact);
    if (!rc) rc = t->d_long.ensure(t->stream, (n_bytes >> 14) + 2, grow_exact);
    if (!rc) rc = with_tmp(t->d_scan_tmp, t->stream, grow_exact, [&](void *tmp, size_t &tmp_bytes) {
        return rocprim::exclusive_scan(tmp, tmp_bytes, items, t->d_scan.p, ScanItem{0, 0}, n_records + 1, ScanAdd(), t->stream);
    });
    if (rc) return rc;
    ScanItem total{0, 0};
    CT_HIPCHK(hipMemcpyAsync(&total, t->d_scan.p + n_records, sizeof total, hipMemcpyDeviceToHost, t->stream));
    CT_HIPCHK(hipStreamSynchronize(t->stream));
    *out_n_bytes = total.bytes;
    *out_n_records = total.records;
    if (((total.bytes + 15) & ~(uint64_t)15) > out_cap_bytes || total.records > out_cap_records)
        return NTK_ERR_CAPACITY;
    if (total.records == 0) {
        if (d_out_offsets) CT_HIPCHK(hipMemsetAsync(d_out_offsets, 0, sizeof(uint64_t), t->stream));
        CT_HIPCHK(hipStreamSynchronize(t->stream));
        return NTK_OK;
    }
    if (!d_out_seq || !d_out_offsets || !d_out_source) return NTK_ERR_BAD_ARG;   // a capacity without its array
    CopyArgs g;
    g.b = b; g.scan = t->d_scan.p;
    g.src_readable = (n_bytes + 15) & ~(uint64_t)15;
    g.out_offsets = d_out_offsets; g.out_source = d_out_source;
    g.total_bytes = total.bytes; g.total_records = total.records;
    g.n_long = t->d_long.p; g.long_list = t->d_long.p + 1; g.long_cap = t->d_long.cap - 1;
    CT_HIPCHK(hipMemsetAsync(t->d_long.p, 0, sizeof(uint64_t), t->stream));
    for (int aux = 0; aux < (d_aux ? 2 : 1); aux++) {
        g.src = aux ? d_aux : d_seq; g.dst = aux ? d_out_aux : d_out_seq;
        g.aux = (uint32_t)aux; g.first = !aux;
        hipLaunchKernelGGL(rt_copy_kernel, dim3(grid_for(n_records, kCopyThreads / kCopyGroup, (unsigned)t->n_cu * 8)), dim3(kCopyThreads),
                           0, t->stream, g);
        CT_HIPCHK(hipGetLastError());
        if (total.bytes > kLongPieces * 16 - 16) {   // only then can a record be long; whether one is, the device alone knows
            hipLaunchKernelGGL(rt_copy_long_kernel, dim3((unsigned)t->n_cu * 4), dim3(kCopyThreads), 0, t->stream, g);
            CT_HIPCHK(hipGetLastError());
        }
    }
    CT_HIPCHK(hipStreamSynchronize(t->stream));
    return NTK_OK;
}

}  // extern "C"
