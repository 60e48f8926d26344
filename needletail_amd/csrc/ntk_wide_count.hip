// Exact count table of canonical k-mers, k = 33..63, on the device (include/needletail_amd_wide_count.h).  Uses only the core's public
// ABI (ntk_ctx_stream: the device and the stream); the keys come from its own fused kernel, which reads the batch bytes and inserts.
//
// Table: structure of arrays hi[slots], lo[slots] (EMPTY = ~0) and counts[slots], 24 B per slot; slot = fmix64(lo ^ fmix64(hi)) &
// (slots - 1), then linear probing, at most kProbeMax slots.  Both key words are write-once (EMPTY -> word, each claimed by an
// agent-scope CAS), counts change only through agent-scope atomics.  No canonical key at k = 33..63 has a word equal to EMPTY: hi has
// 2k - 64 <= 62 bits, and lo == ~0 (the key ends in 32 T) would make the reverse complement start with 32 A, smaller than the key unless
// the key also starts with 32 A, and for k <= 63 those two runs overlap.  At k = 64 the palindromes T^32 A^32 and A^32 T^32 break this,
// which is why the table stops at 63.  DESIGN.md section 11 has the claim protocol and why it is exact; ntk_count_common.hpp holds what
// the narrow table shares.
#include "../../include/needletail_amd_wide_count.h"
#include "ntk_count_common.hpp"

#include <new>
#include <rocprim/device/device_radix_sort.hpp>

namespace {

constexpr uint32_t kKMin = 33, kKMax = 63;
constexpr uint32_t kLaneRun = 64;                        // window ends per lane of the count kernel
constexpr uint32_t kPrime = 64;                          // bytes each lane reads before its first end (>= kKMax - 1, a multiple of 16)
// stats words on the device: the shared ones only (no key needs a side word)
constexpr int kStWords = 3;

static_assert(kPrime >= kKMax - 1 && kPrime % 16 == 0 && kLaneRun % 16 == 0, "lane geometry");

__device__ inline uint64_t home_slot(uint64_t hi, uint64_t lo, uint64_t mask) { return fmix64(lo ^ fmix64(hi)) & mask; }

// the word's value after an agent-scope claim of an EMPTY word: `want` if this lane wrote it, else the word another lane wrote first
__device__ inline uint64_t claim(uint64_t *w, uint64_t want, bool &won)
{
    uint64_t expected = kEmpty;
    won = __hip_atomic_compare_exchange_strong(w, &expected, want, __ATOMIC_RELAXED, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    return won ? want : expected;
}

struct Table {
    uint64_t *hi, *lo, *counts;
    uint64_t mask;
    uint32_t probe_max;
};

struct CountArgs {
    const uint8_t *seq, *qual;   // qual: nullptr = no mask
    uint64_t n_bytes;            // windows ending in [0, n_bytes) count; no byte at or past it is a base
    uint32_t k, cutoff;
    Table t;
    uint64_t *stats;
};

// Count one occurrence of the key (x, y).  Per probe step: the hi word, then the lo word, each a plain load that sees EMPTY or the final
// word (write-once), and on EMPTY an agent-scope CAS whose returned value decides.  The slot is skipped only when one of its final words
// is not the key's, so a key never lands in two slots; no lane waits for another.  A won lo claim makes a new key (whoever claimed
// the hi word).  Returns 1 on a new key, 0 on a repeat, -1 when the probe bound is reached (dropped).
__device__ inline int insert(const Table &t, uint64_t x, uint64_t y)
{
    uint64_t slot = home_slot(x, y, t.mask);
    for (uint32_t p = 0; p < t.probe_max; p++, slot = (slot + 1) & t.mask) {
        bool won_hi = false, won_lo = false;
        uint64_t h = t.hi[slot];
        if (h == kEmpty) h = claim(&t.hi[slot], x, won_hi);
        if (h != x) continue;
        uint64_t l = t.lo[slot];
        if (l == kEmpty) l = claim(&t.lo[slot], y, won_lo);
        if (l != y) continue;
        add_agent(&t.counts[slot], 1);
        return won_lo ? 1 : 0;
    }
    return -1;
}

// The fused count kernel.  Lane r (grid-stride) owns the window ends [r * kLaneRun, (r + 1) * kLaneRun): it reads the kPrime bytes
// before its first end and its own kLaneRun bytes in 16-byte loads, rolls the forward and reverse-complement words (two u64 each) over
// all of them, and inserts min(forward, reverse complement) of every window that ends in its run after k base bytes in a row.  A load
// is issued only for a 16-byte block that starts in [0, n_bytes) (the layout makes round_up(n_bytes, 16) readable), and a byte at or
// past n_bytes is a break.  The counters are summed per lane, then across the wave, and added once per wave.
__global__ __launch_bounds__(kThreads) void wt_count_kernel(CountArgs a)
{
    uint64_t distinct = 0, total = 0, dropped = 0;
    const uint32_t k = a.k, hi_bits = 2 * k - 64, rc_shift = 2 * k - 66;
    const uint64_t hi_mask = ((uint64_t)1 << hi_bits) - 1;
    const uint64_t n_runs = (a.n_bytes + kLaneRun - 1) / kLaneRun, stride = (uint64_t)gridDim.x * blockDim.x;
    for (uint64_t r = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; r < n_runs; r += stride) {
        const uint64_t first_end = r * kLaneRun;
        uint64_t fh = 0, fl = 0, rh = 0, rl = 0;
        uint32_t run = 0;
#pragma unroll 1
        for (uint32_t blk = 0; blk < (kPrime + kLaneRun) / 16; blk++) {
            // 16 bytes starting at first_end - kPrime + 16 * blk (before 0 or at / past n_bytes: breaks)
            const uint64_t at = first_end + 16 * blk;   // = the block's start + kPrime
            uint4 s = make_uint4(0, 0, 0, 0), q = make_uint4(~0u, ~0u, ~0u, ~0u);
            if (at >= kPrime && at - kPrime < a.n_bytes) {
                s = *reinterpret_cast<const uint4 *>(a.seq + (at - kPrime));
                if (a.qual) q = *reinterpret_cast<const uint4 *>(a.qual + (at - kPrime));
            }
#pragma unroll 1
            for (uint32_t j = 0; j < 16; j++) {
                const uint32_t b = s.x & 0xFF, qb = q.x & 0xFF;
                s.x = (s.x >> 8) | (s.y << 24); s.y = (s.y >> 8) | (s.z << 24); s.z = (s.z >> 8) | (s.w << 24); s.w >>= 8;
                q.x = (q.x >> 8) | (q.y << 24); q.y = (q.y >> 8) | (q.z << 24); q.z = (q.z >> 8) | (q.w << 24); q.w >>= 8;
                const uint64_t pos_plus = at + j;   // the byte's position + kPrime
                const uint32_t l = b | 0x20;        // ACGTU / acgtu -> lower case
                const bool base = (l == 'a' || l == 'c' || l == 'g' || l == 't' || l == 'u') && qb >= a.cutoff &&
                                  pos_plus - kPrime < a.n_bytes;
                const uint64_t c = ((b >> 1) ^ (b >> 2)) & 3;   // A 0, C 1, G 2, T / U 3 in either case
                fh = ((fh << 2) | (fl >> 62)) & hi_mask;
                fl = (fl << 2) | c;
                rl = (rl >> 2) | (rh << 62);
                rh = (rh >> 2) | ((3 - c) << rc_shift);
                run = base ? run + 1 : 0;
                if (run >= k && pos_plus >= first_end + kPrime) {
                    const bool fwd = fh < rh || (fh == rh && fl <= rl);
                    const int got = insert(a.t, fwd ? fh : rh, fwd ? fl : rl);
                    if (got < 0) {
                        dropped++;
                    } else {
                        total++;
                        distinct += (uint64_t)got;
                    }
                }
            }
        }
    }
    distinct = wave_sum(distinct); total = wave_sum(total); dropped = wave_sum(dropped);
    if ((threadIdx.x & 63) == 0) {
        if (distinct) add_agent(a.stats + kStDistinct, distinct);
        if (total) add_agent(a.stats + kStTotal, total);
        if (dropped) add_agent(a.stats + kStDropped, dropped);
    }
}

// a key row as extract writes it, and the decomposer that makes the radix sort see hi * 2^64 + lo
struct WideKey {
    uint64_t hi, lo;
};
struct WideKeyDecomposer {
    __host__ __device__ rocprim::tuple<uint64_t &, uint64_t &> operator()(WideKey &key) const
    {
        return rocprim::tuple<uint64_t &, uint64_t &>(key.hi, key.lo);
    }
};

// extract, step 3: scatter the pairs of each block to its offset (order inside a block is arbitrary: the sort follows)
__global__ __launch_bounds__(kThreads) void wt_extract_scatter_kernel(const uint64_t *hi, const uint64_t *lo, const uint64_t *counts,
                                                                      uint64_t slots, uint64_t min_count, const uint64_t *offsets,
                                                                      WideKey *out_keys, uint64_t *out_counts)
{
    __shared__ uint32_t fill;
    if (threadIdx.x == 0) fill = 0;
    __syncthreads();
    const uint64_t base = (uint64_t)blockIdx.x * kExtractPerBlock, at = offsets[blockIdx.x];
    for (uint32_t j = 0; j < kExtractPerThread; j++) {
        const uint64_t s = base + (uint64_t)j * kThreads + threadIdx.x;
        if (s >= slots) continue;
        const uint64_t h = hi[s], c = counts[s];
        if (h != kEmpty && c >= min_count) {
            const uint32_t pos = atomicAdd(&fill, 1u);
            out_keys[at + pos] = WideKey{h, lo[s]};
            out_counts[at + pos] = c;
        }
    }
}

// reverse complement of 32 bases in one word (complement = 3 - code = code ^ 3; reverse the 2-bit groups)
__device__ inline uint64_t revcomp32(uint64_t x)
{
    x = ~x;
    x = ((x >> 2) & 0x3333333333333333ull) | ((x & 0x3333333333333333ull) << 2);
    x = ((x >> 4) & 0x0F0F0F0F0F0F0F0Full) | ((x & 0x0F0F0F0F0F0F0F0Full) << 4);
    return __builtin_bswap64(x);
}

// lookup: canonicalise the query, then a read-only probe that stops at an EMPTY hi word
__global__ __launch_bounds__(kThreads) void wt_lookup_kernel(Table t, uint32_t k, const uint64_t *queries, uint64_t n, uint64_t *out)
{
    const uint32_t hi_bits = 2 * k - 64, s = 128 - 2 * k;   // s = 2..62
    const uint64_t stride = (uint64_t)gridDim.x * blockDim.x;
    for (uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += stride) {
        const uint64_t qh = queries[2 * i], ql = queries[2 * i + 1];
        uint64_t c = 0;
        if ((qh >> hi_bits) == 0) {
            // the 128-bit reverse complement of the whole word pair, shifted down to 2k bits
            const uint64_t top = revcomp32(ql), bottom = revcomp32(qh);
            const uint64_t rh = top >> s, rl = (bottom >> s) | (top << (64 - s));
            const bool fwd = qh < rh || (qh == rh && ql <= rl);
            const uint64_t x = fwd ? qh : rh, y = fwd ? ql : rl;
            uint64_t slot = home_slot(x, y, t.mask);
            for (uint32_t p = 0; p < t.probe_max; p++, slot = (slot + 1) & t.mask) {
                const uint64_t h = t.hi[slot];
                if (h == kEmpty) break;
                if (h == x && t.lo[slot] == y) { c = t.counts[slot]; break; }
            }
        }
        out[i] = c;
    }
}

}  // namespace

struct ntk_wide_table : TableCore {
    DeviceArray<uint64_t> d_hi, d_lo;
};

namespace {

Table table_of(const ntk_wide_table *t) { return Table{t->d_hi.p, t->d_lo.p, t->d_counts.p, t->slots - 1, t->probe_max}; }

}  // namespace

extern "C" {

int ntk_wide_table_create(ntk_ctx *ctx, uint32_t k, uint32_t path, uint64_t capacity, ntk_wide_table **out)
{
    if (!ctx || !out) return NTK_ERR_BAD_ARG;
    *out = nullptr;
    if (k < kKMin || k > kKMax) return NTK_ERR_BAD_K;
    if (path == NTK_PATH_BITS || path == NTK_PATH_BITS_CANONICAL) return NTK_ERR_BAD_K;   // the 2-bit iterator stops at k = 32
    if (path != NTK_PATH_BYTES_CANONICAL || capacity == 0 || capacity > ((uint64_t)3 << 38)) return NTK_ERR_BAD_ARG;
    ntk_wide_table *t = new (std::nothrow) ntk_wide_table();
    if (!t) return NTK_ERR_NOMEM;
    int rc = t->init(ctx, k, path, capacity);
    if (rc) { delete t; return rc; }
    rc = t->alloc({&t->d_hi, &t->d_lo}, kStWords);
    if (!rc) rc = ntk_wide_table_reset(t);
    if (rc) { ntk_wide_table_destroy(t); return rc; }
    *out = t;
    return NTK_OK;
}

void ntk_wide_table_destroy(ntk_wide_table *t)
{
    if (!t) return;
    t->release({&t->d_hi, &t->d_lo});
    delete t;
}

int ntk_wide_table_reset(ntk_wide_table *t)
{
    if (!t) return NTK_ERR_BAD_ARG;
    return t->reset({&t->d_hi, &t->d_lo}, kStWords);
}

int ntk_wide_table_count_device(ntk_wide_table *t, const uint8_t *d_seq, const uint8_t *d_qual, uint64_t n_bytes, const ntk_params *p)
{
    int rc = check_batch_params(t, p);   // the table's path is the byte path: it needs NORMALIZE
    if (rc || n_bytes == 0) return rc;
    if ((rc = check_batch_pointers(d_seq, d_qual))) return rc;
    CT_HIPCHK(hipSetDevice(t->device));
    CountArgs a;
    a.seq = d_seq; a.n_bytes = n_bytes; a.k = t->k;
    set_quality(a, p, d_qual);
    a.t = table_of(t); a.stats = t->d_stats.p;
    const uint64_t runs = (n_bytes + kLaneRun - 1) / kLaneRun;
    hipLaunchKernelGGL(wt_count_kernel, dim3(grid_for(runs, kThreads, (unsigned)t->n_cu * 8)), dim3(kThreads), 0, t->stream, a);
    CT_HIPCHK(hipGetLastError());
    return NTK_OK;
}

int ntk_wide_table_stats(ntk_wide_table *t, struct ntk_kmer_table_stats *out)
{
    if (!t || !out) return NTK_ERR_BAD_ARG;
    uint64_t w[kStWords];
    int rc = t->read_stats(w, kStWords);
    if (rc) return rc;
    out->n_distinct = w[kStDistinct];
    out->n_total = w[kStTotal];
    out->n_dropped = w[kStDropped];
    out->slots = t->slots; out->k = t->k; out->path = t->path;
    return NTK_OK;
}

int ntk_wide_table_extract_device(ntk_wide_table *t, uint64_t min_count, uint64_t *d_keys, uint64_t *d_counts, uint64_t cap, uint64_t *n)
{
    if (!t || !n) return NTK_ERR_BAD_ARG;
    *n = 0;
    uint64_t w[kStWords], need = 0;
    int rc = t->read_complete(w, kStWords);
    if (rc) return rc;
    if (min_count == 0) min_count = 1;
    rc = t->extract_offsets(t->d_hi.p, min_count, &need);
    if (rc) return rc;
    *n = need;
    if (need > cap) return NTK_ERR_CAPACITY;
    if (need == 0) return NTK_OK;
    if (!d_keys || !d_counts) return NTK_ERR_BAD_ARG;
    WideKey *out_keys = reinterpret_cast<WideKey *>(d_keys);
    return t->scatter_sort<WideKey>(
        need,
        [&](WideKey *tk, uint64_t *tc) {
            hipLaunchKernelGGL(wt_extract_scatter_kernel, dim3((unsigned)t->extract_blocks()), dim3(kThreads), 0, t->stream, t->d_hi.p,
                               t->d_lo.p, t->d_counts.p, t->slots, min_count, t->d_offsets.p, tk, tc);
        },
        // the keys are < 2^(2k) as hi * 2^64 + lo: a radix sort on the low 2k bits of the pair orders them
        [&](void *tmp, size_t &tmp_bytes, WideKey *tk, uint64_t *tc) {
            return rocprim::radix_sort_pairs(tmp, tmp_bytes, tk, out_keys, tc, d_counts, need, WideKeyDecomposer{}, 0u, 2 * t->k,
                                             t->stream);
        });
}

int ntk_wide_table_spectrum(ntk_wide_table *t, uint64_t *hist, uint32_t n_bins)
{
    if (!t || !hist || n_bins < 2 || n_bins > kMaxBins) return NTK_ERR_BAD_ARG;
    uint64_t w[kStWords];
    const int rc = t->read_complete(w, kStWords);
    return rc ? rc : t->spectrum(t->d_hi.p, hist, n_bins);
}

int ntk_wide_table_lookup_device(ntk_wide_table *t, const uint64_t *d_queries, uint64_t n, uint64_t *d_counts)
{
    if (!t || ((!d_queries || !d_counts) && n)) return NTK_ERR_BAD_ARG;
    uint64_t w[kStWords];
    int rc = t->read_complete(w, kStWords);
    if (rc) return rc;
    if (n == 0) return NTK_OK;
    hipLaunchKernelGGL(wt_lookup_kernel, dim3(grid_for(n, kThreads, (unsigned)t->n_cu * 8)), dim3(kThreads), 0, t->stream, table_of(t),
                       t->k, d_queries, n, d_counts);
    CT_HIPCHK(hipGetLastError());
    CT_HIPCHK(hipStreamSynchronize(t->stream));
    return NTK_OK;
}

}  // extern "C"
