// Exact k-mer count table on the device (include/needletail_amd_count.h).  A consumer of the core's public ABI: the keys are the values
// ntk_materialize_device_quality emits, so every path's canonical form and tie rule are the core's by construction.
//
// Table: structure of arrays, keys[slots] (EMPTY = ~0) and counts[slots], 16 B per slot; slot = fmix64(key) & (slots - 1), then
// linear probing, at most kProbeMax slots.  Keys are write-once (EMPTY -> key, claimed by an agent-scope CAS), counts change only
// through agent-scope atomics.  The one key that equals EMPTY (NTK_PATH_BITS, k = 32, TTT...T) is counted in a side word.
// DESIGN.md section 10 has the layout and the coherence argument, section 16 the chunking; ntk_count_common.hpp holds what the wide table
// shares.
#include "../../include/needletail_amd_count.h"
#include "ntk_count_common.hpp"

#include <new>
#include <rocprim/device/device_radix_sort.hpp>

namespace {

// stats words on the device: the shared ones, then the side word of the all-ones key
constexpr int kStOnes = 3, kStWords = 4;

struct InsertArgs {
    const uint64_t *values;    // materialised values, indexed by window end
    const uint16_t *valid16;   // bit (15 - e % 16) of word e / 16: window e is emitted
    uint64_t first, n;         // windows ending in [first, n) are inserted (first: the chunk's halo)
    uint64_t *keys, *counts, *stats;
    uint64_t mask;
    uint32_t probe_max;
};

// One window end per lane, grid-stride; every lane of a wave runs the same number of iterations (the bound is rounded up to the
// grid), so the counters are summed across the wave once at the end and added by one lane.
__global__ __launch_bounds__(kThreads) void kt_insert_kernel(InsertArgs a)
{
    uint64_t distinct = 0, total = 0, dropped = 0, ones = 0;
    const uint64_t stride = (uint64_t)gridDim.x * blockDim.x, span = a.n - a.first;
    const uint64_t rounds = (span + stride - 1) / stride;
    uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    for (uint64_t r = 0; r < rounds; r++, i += stride) {
        if (i >= span) continue;
        const uint64_t e = a.first + i;
        if (!((a.valid16[e >> 4] >> (15 - (e & 15))) & 1u)) continue;
        const uint64_t key = a.values[e];
        if (key == kEmpty) { ones++; total++; continue; }
        uint64_t slot = fmix64(key) & a.mask;
        uint32_t p = 0;
        for (; p < a.probe_max; p++, slot = (slot + 1) & a.mask) {
            // a plain load sees EMPTY or the slot's final key (write-once); EMPTY may be stale in this XCD's L2, so only the CAS's
            // returned value decides whether the slot is ours, already this key, or another key's
            uint64_t cur = a.keys[slot];
            if (cur == kEmpty) {
                uint64_t expected = kEmpty;
                if (__hip_atomic_compare_exchange_strong(&a.keys[slot], &expected, key, __ATOMIC_RELAXED, __ATOMIC_RELAXED,
                                                         __HIP_MEMORY_SCOPE_AGENT)) {
                    distinct++;
                    cur = key;
                } else {
                    cur = expected;
                }
            }
            if (cur == key) {
                add_agent(&a.counts[slot], 1);
                total++;
                break;
            }
        }
        if (p == a.probe_max) dropped++;
    }
    distinct = wave_sum(distinct); total = wave_sum(total); dropped = wave_sum(dropped); ones = wave_sum(ones);
    if ((threadIdx.x & 63) == 0) {
        if (distinct) add_agent(a.stats + kStDistinct, distinct);
        if (total) add_agent(a.stats + kStTotal, total);
        if (dropped) add_agent(a.stats + kStDropped, dropped);
        if (ones) add_agent(a.stats + kStOnes, ones);
    }
}

// extract, step 3: scatter the pairs of each block to its offset (order inside a block is arbitrary: the sort follows)
__global__ __launch_bounds__(kThreads) void kt_extract_scatter_kernel(const uint64_t *keys, const uint64_t *counts, uint64_t slots,
                                                                      uint64_t min_count, const uint64_t *offsets, uint64_t *out_keys,
                                                                      uint64_t *out_counts)
{
    __shared__ uint32_t fill;
    if (threadIdx.x == 0) fill = 0;
    __syncthreads();
    const uint64_t base = (uint64_t)blockIdx.x * kExtractPerBlock, at = offsets[blockIdx.x];
    for (uint32_t j = 0; j < kExtractPerThread; j++) {
        const uint64_t s = base + (uint64_t)j * kThreads + threadIdx.x;
        if (s >= slots) continue;
        const uint64_t key = keys[s], c = counts[s];
        if (key != kEmpty && c >= min_count) {
            const uint32_t pos = atomicAdd(&fill, 1u);
            out_keys[at + pos] = key;
            out_counts[at + pos] = c;
        }
    }
}

// lookup: read-only probe; the EMPTY key reads the side word
__global__ __launch_bounds__(kThreads) void kt_lookup_kernel(const uint64_t *keys, const uint64_t *counts, uint64_t mask,
                                                             uint32_t probe_max, uint64_t ones, const uint64_t *queries, uint64_t n,
                                                             uint64_t *out)
{
    const uint64_t stride = (uint64_t)gridDim.x * blockDim.x;
    for (uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += stride) {
        const uint64_t q = queries[i];
        uint64_t c = 0;
        if (q == kEmpty) {
            c = ones;
        } else {
            uint64_t slot = fmix64(q) & mask;
            for (uint32_t p = 0; p < probe_max; p++, slot = (slot + 1) & mask) {
                const uint64_t cur = keys[slot];
                if (cur == q) { c = counts[slot]; break; }
                if (cur == kEmpty) break;
            }
        }
        out[i] = c;
    }
}

}  // namespace

struct ntk_kmer_table : TableCore {
    DeviceArray<uint64_t> d_keys;
    MaterialiseScratch scratch;   // of one chunk (grown on demand)
};

extern "C" {

int ntk_kmer_table_create(ntk_ctx *ctx, uint32_t k, uint32_t path, uint64_t capacity, ntk_kmer_table **out)
{
    if (!ctx || !out) return NTK_ERR_BAD_ARG;
    *out = nullptr;
    if (k < 1 || k > 32) return NTK_ERR_BAD_K;
    if (path > NTK_PATH_BITS_CANONICAL || capacity == 0 || capacity > ((uint64_t)3 << 38)) return NTK_ERR_BAD_ARG;
    ntk_kmer_table *t = new (std::nothrow) ntk_kmer_table();
    if (!t) return NTK_ERR_NOMEM;
    int rc = t->init(ctx, k, path, capacity);
    if (rc) { delete t; return rc; }
    rc = t->alloc({&t->d_keys}, kStWords);
    if (!rc) rc = ntk_kmer_table_reset(t);
    if (rc) { ntk_kmer_table_destroy(t); return rc; }
    *out = t;
    return NTK_OK;
}

void ntk_kmer_table_destroy(ntk_kmer_table *t)
{
    if (!t) return;
    t->release({&t->d_keys});
    t->scratch.release();
    delete t;
}

int ntk_kmer_table_reset(ntk_kmer_table *t)
{
    if (!t) return NTK_ERR_BAD_ARG;
    return t->reset({&t->d_keys}, kStWords);
}

int ntk_kmer_table_count_device(ntk_kmer_table *t, const uint8_t *d_seq, const uint8_t *d_qual, uint64_t n_bytes, const ntk_params *p)
{
    int rc = check_batch_params(t, p);
    if (rc || n_bytes == 0) return rc;
    if ((rc = check_batch_pointers(d_seq, d_qual))) return rc;
    CT_HIPCHK(hipSetDevice(t->device));
    // of every chunk only the windows ending at or after its start count
    return for_each_chunk(*t, t->scratch, d_seq, d_qual, n_bytes, p, [&](const Chunk &c) -> int {
        InsertArgs a;
        a.values = t->scratch.d_values.p; a.valid16 = t->scratch.d_valid16.p;
        a.first = c.skip(); a.n = c.len();
        a.keys = t->d_keys.p; a.counts = t->d_counts.p; a.stats = t->d_stats.p;
        a.mask = t->slots - 1; a.probe_max = t->probe_max;
        hipLaunchKernelGGL(kt_insert_kernel, dim3(grid_for(a.n - a.first, kThreads, (unsigned)t->n_cu * 8)), dim3(kThreads), 0,
                           t->stream, a);
        CT_HIPCHK(hipGetLastError());
        return NTK_OK;
    });
}

int ntk_kmer_table_stats(ntk_kmer_table *t, struct ntk_kmer_table_stats *out)
{
    if (!t || !out) return NTK_ERR_BAD_ARG;
    uint64_t w[kStWords];
    int rc = t->read_stats(w, kStWords);
    if (rc) return rc;
    out->n_distinct = w[kStDistinct] + (w[kStOnes] ? 1 : 0);
    out->n_total = w[kStTotal];
    out->n_dropped = w[kStDropped];
    out->slots = t->slots; out->k = t->k; out->path = t->path;
    return NTK_OK;
}

int ntk_kmer_table_extract_device(ntk_kmer_table *t, uint64_t min_count, uint64_t *d_keys, uint64_t *d_counts, uint64_t cap, uint64_t *n)
{
    if (!t || !n) return NTK_ERR_BAD_ARG;
    *n = 0;
    uint64_t w[kStWords], in_table = 0;
    int rc = t->read_complete(w, kStWords);
    if (rc) return rc;
    if (min_count == 0) min_count = 1;
    rc = t->extract_offsets(t->d_keys.p, min_count, &in_table);
    if (rc) return rc;
    const uint64_t ones = w[kStOnes] >= min_count ? w[kStOnes] : 0, need = in_table + (ones ? 1 : 0);
    *n = need;
    if (need > cap) return NTK_ERR_CAPACITY;
    if (need == 0) return NTK_OK;
    if (!d_keys || !d_counts) return NTK_ERR_BAD_ARG;
    if (in_table) {
        rc = t->scatter_sort<uint64_t>(
            in_table,
            [&](uint64_t *tk, uint64_t *tc) {
                hipLaunchKernelGGL(kt_extract_scatter_kernel, dim3((unsigned)t->extract_blocks()), dim3(kThreads), 0, t->stream, t->d_keys.p,
                                   t->d_counts.p, t->slots, min_count, t->d_offsets.p, tk, tc);
            },
            // the keys are < 4^k: a radix sort on the low 2k bits orders them
            [&](void *tmp, size_t &tmp_bytes, uint64_t *tk, uint64_t *tc) {
                return rocprim::radix_sort_pairs(tmp, tmp_bytes, tk, d_keys, tc, d_counts, in_table, 0u, 2 * t->k, t->stream);
            });
        if (rc) return rc;
    }
    if (ones) {   // the all-ones key sorts last
        t->h_stage.p[0] = kEmpty; t->h_stage.p[1] = ones;
        CT_HIPCHK(hipMemcpyAsync(d_keys + in_table, t->h_stage.p, sizeof(uint64_t), hipMemcpyHostToDevice, t->stream));
        return t->h_stage.write(t->stream, d_counts + in_table, 1, 1);
    }
    return NTK_OK;
}

int ntk_kmer_table_spectrum(ntk_kmer_table *t, uint64_t *hist, uint32_t n_bins)
{
    if (!t || !hist || n_bins < 2 || n_bins > kMaxBins) return NTK_ERR_BAD_ARG;
    uint64_t w[kStWords];
    int rc = t->read_complete(w, kStWords);
    if (!rc) rc = t->spectrum(t->d_keys.p, hist, n_bins);
    if (rc) return rc;
    if (w[kStOnes]) hist[w[kStOnes] < n_bins - 1 ? w[kStOnes] : n_bins - 1]++;
    return NTK_OK;
}

int ntk_kmer_table_lookup_device(ntk_kmer_table *t, const uint64_t *d_queries, uint64_t n, uint64_t *d_counts)
{
    if (!t || ((!d_queries || !d_counts) && n)) return NTK_ERR_BAD_ARG;
    uint64_t w[kStWords];
    int rc = t->read_complete(w, kStWords);
    if (rc) return rc;
    if (n == 0) return NTK_OK;
    hipLaunchKernelGGL(kt_lookup_kernel, dim3(grid_for(n, kThreads, (unsigned)t->n_cu * 8)), dim3(kThreads), 0, t->stream, t->d_keys.p,
                       t->d_counts.p, t->slots - 1, t->probe_max, w[kStOnes], d_queries, n, d_counts);
    CT_HIPCHK(hipGetLastError());
    CT_HIPCHK(hipStreamSynchronize(t->stream));
    return NTK_OK;
}

}  // extern "C"
