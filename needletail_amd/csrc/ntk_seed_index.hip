// Seeding reads against references (include_staged/needletail_amd/seed_index.h): a minimizer index of a reference batch held on the
// device, and the minimizer lists of a read batch matched against it into a per-read CSR of anchors.  A consumer of the core's public ABI
// on the shared scaffold (ntk_consumer.hpp); it reads minimizer-list CSRs alone, never a base, and links nothing but the core.
//
// Build: verify the list, search every entry's record (si_owner_kernel), sort (value -> entry index) with rocPRIM's stable radix sort,
// mark and number the first occurrence of each value, and pack keys, ranges, ref and rpos.  Match: verify the list, look every seed up
// (si_lookup_kernel), scan the anchor counts, sum the rows per read with a wave (si_rows_kernel), read the total back - the capacity rule
// and the growth of the anchor arrays happen there - expand one anchor per thread (si_fill_kernel), and sort every read's anchors: in
// LDS up to SI_SORT_TILE of them (si_sort_kernel), through two stable segmented radix sorts beyond, on a compact copy of those reads'
// anchors.  rocPRIM's temporary storage is held inside a call only.  The rule is ntk_si_rule.hpp's.
// DESIGN.md section 23.
#include "../../include_staged/needletail_amd/seed_index.h"
#include "ntk_consumer.hpp"
#include "ntk_si_rule.hpp"

#include <rocprim/device/device_radix_sort.hpp>
#include <rocprim/device/device_scan.hpp>
#include <rocprim/device/device_segmented_radix_sort.hpp>

#include <new>

namespace {

// the counter words: what the verification raised, the list's first and last entry, the largest occ / the anchors of the long route
constexpr int kCtrFlags = 0, kCtrLo = 1, kCtrHi = 2, kCtrMax = 3, kCtrWords = 4;
constexpr int kCtrLong = kCtrMax;   // the anchors of the reads of the long route
constexpr uint32_t kAbsent = 0xFFFFFFFFu;   // a seed's key index where its value is no key (a key index is below 2^32 - 1)

static_assert(SI_THREADS == kThreads, "block_sum_u32 sums a block of kThreads");

__device__ inline void or_agent(uint64_t *p, uint64_t v) { (void)__hip_atomic_fetch_or(p, v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT); }
__device__ inline void max_agent(uint64_t *p, uint64_t v) { (void)__hip_atomic_fetch_max(p, v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT); }

__device__ inline uint64_t first_item() { return (uint64_t)blockIdx.x * SI_THREADS + threadIdx.x; }
__device__ inline uint64_t item_step() { return (uint64_t)gridDim.x * SI_THREADS; }

// The list as the rule reads it: offsets non-decreasing and offsets[n_records] <= n, and no pos of an entry of a record at or above
// 2^32.  offsets[0] and offsets[n_records] are read before they are known to be good: they only select the entries whose pos is looked
// at, every one of them below n.  ctr is zeroed before.
__global__ __launch_bounds__(SI_THREADS) void si_verify_kernel(const uint64_t *offsets, uint64_t n_records, const uint64_t *pos, uint64_t n,
                                                               uint64_t *ctr)
{
    const uint64_t lo = offsets[0], hi = offsets[n_records], items = n_records + 1 > n ? n_records + 1 : n;
    uint32_t bad = 0;
    for (uint64_t i = first_item(); i < items; i += item_step()) {
        if (i < n_records && offsets[i] > offsets[i + 1]) bad |= SI_BAD_OFFSETS;
        if (i == n_records && offsets[i] > n) bad |= SI_BAD_OFFSETS;
        if (i < n && i >= lo && i < hi && (pos[i] >> 32)) bad |= SI_BAD_POS;
    }
    if (bad) or_agent(ctr + kCtrFlags, bad);
    if (first_item() == 0) { ctr[kCtrLo] = lo; ctr[kCtrHi] = hi; }
}

// entry lo + i of the list: its record, and its own index for the sort to carry
__global__ __launch_bounds__(SI_THREADS) void si_owner_kernel(const uint64_t *offsets, uint64_t n_records, uint64_t lo, uint64_t m,
                                                              uint32_t *owner, uint32_t *idx)
{
    for (uint64_t i = first_item(); i < m; i += item_step()) {
        owner[i] = (uint32_t)(si_at_or_before(offsets, n_records + 1, lo + i) - 1);
        idx[i] = (uint32_t)i;
    }
}

// head[j] = the sorted value j is the first of its kind
__global__ __launch_bounds__(SI_THREADS) void si_heads_kernel(const uint64_t *sorted, uint64_t m, uint32_t *head)
{
    for (uint64_t j = first_item(); j < m; j += item_step()) head[j] = j == 0 || sorted[j] != sorted[j - 1];
}

struct PackArgs {
    const uint64_t *sorted, *pos;        // the sorted values; the list's pos
    const uint32_t *perm, *owner, *head, *rank, *info;
    uint64_t lo, m, n_keys;
    uint64_t *keys;
    uint32_t *start, *ref, *rpos;
};

// occurrence j of the index: the entry the sort put there; the first of a value also writes its key and where its range starts
__global__ __launch_bounds__(SI_THREADS) void si_pack_kernel(PackArgs a)
{
    for (uint64_t j = first_item(); j < a.m; j += item_step()) {
        const uint32_t e = a.perm[j];
        a.ref[j] = si_ref(a.owner[e], a.info[a.lo + e]);
        a.rpos[j] = (uint32_t)a.pos[a.lo + e];
        if (a.head[j]) {
            const uint32_t key = a.rank[j] - 1;
            a.keys[key] = a.sorted[j];
            a.start[key] = (uint32_t)j;
        }
        if (j + 1 == a.m) a.start[a.n_keys] = (uint32_t)a.m;
    }
}

// The occ of every key: its bin (n_bins != 0; the bins below SI_SPECTRUM_LDS are summed in LDS first) and the largest of all.
__global__ __launch_bounds__(SI_THREADS) void si_spectrum_kernel(const uint32_t *start, uint64_t n_keys, uint64_t *hist, uint32_t n_bins,
                                                                 uint64_t *largest)
{
    __shared__ uint32_t s_bin[SI_SPECTRUM_LDS];
    for (uint32_t c = threadIdx.x; c < SI_SPECTRUM_LDS; c += SI_THREADS) s_bin[c] = 0;
    __syncthreads();
    uint64_t most = 0;
    for (uint64_t key = first_item(); key < n_keys; key += item_step()) {
        const uint32_t occ = start[key + 1] - start[key];
        most = occ > most ? occ : most;
        if (n_bins) {
            const uint32_t c = occ < n_bins - 1 ? occ : n_bins - 1;
            if (c < SI_SPECTRUM_LDS) atomicAdd(&s_bin[c], 1u); else add_agent(hist + c, 1);
        }
    }
    __syncthreads();
    for (uint32_t c = threadIdx.x; c < SI_SPECTRUM_LDS && c < n_bins; c += SI_THREADS)
        if (s_bin[c]) add_agent(hist + c, s_bin[c]);
    if (most) max_agent(largest, most);
}

struct MatchArgs {
    const uint64_t *offsets, *pos, *values;   // the read list
    const uint32_t *info;
    uint64_t n_reads, lo, n_seeds;            // its seeds are the entries [lo, lo + n_seeds)
    const uint64_t *keys;                     // the index
    const uint32_t *start, *ref, *rpos;
    uint64_t n_keys;
    uint32_t max_occ;
    uint32_t *hit, *count;                    // per seed: its key index (kAbsent: none) and its anchors
    const uint64_t *base;                     // the exclusive scan of count, n_seeds + 1 long
    uint64_t *a_offsets, *seg_begin, *seg_end;
    uint32_t *rows;
    uint64_t *ctr;
    uint64_t n_anchors;
    uint32_t *a_ref_rev, *a_rpos, *a_qpos;
};

// one seed per thread: searched, classified, counted.  count[n_seeds] = 0 closes the scan.
__global__ __launch_bounds__(SI_THREADS) void si_lookup_kernel(MatchArgs a)
{
    for (uint64_t s = first_item(); s <= a.n_seeds; s += item_step()) {
        if (s == a.n_seeds) { a.count[s] = 0; break; }
        const uint64_t v = a.values[a.lo + s], at = si_find(a.keys, a.n_keys, v);
        const bool present = at < a.n_keys && a.keys[at] == v;
        const uint32_t occ = present ? a.start[at + 1] - a.start[at] : 0;
        a.hit[s] = present ? (uint32_t)at : kAbsent;
        a.count[s] = si_classify(present, occ, a.max_occ) == SI_HIT ? occ : 0;
    }
}

// One wave per read: its row, where its anchors start, and its segment of the compact arrays the segmented sort works on: a read of the
// long route takes as many places as it has anchors from the counter (in whatever order the waves come: the places only have to be
// disjoint), every other read has the empty segment.  Wave n_reads closes a_offsets.
__global__ __launch_bounds__(SI_THREADS) void si_rows_kernel(MatchArgs a)
{
    const uint32_t lane = threadIdx.x & 63;
    const uint64_t waves = (uint64_t)gridDim.x * (SI_THREADS / 64);
    for (uint64_t q = (uint64_t)blockIdx.x * (SI_THREADS / 64) + (threadIdx.x >> 6); q <= a.n_reads; q += waves) {
        if (q == a.n_reads) {
            if (lane == 0) a.a_offsets[q] = a.base[a.n_seeds];
            break;
        }
        const uint64_t b = a.offsets[q] - a.lo, e = a.offsets[q + 1] - a.lo;
        uint64_t n_hit = 0, n_rep = 0, n_absent = 0;
        for (uint64_t s = b + lane; s < e; s += 64) {
            const bool absent = a.hit[s] == kAbsent, hit = a.count[s] != 0;
            n_absent += absent; n_hit += hit; n_rep += !absent && !hit;
        }
        n_hit = wave_sum(n_hit); n_rep = wave_sum(n_rep); n_absent = wave_sum(n_absent);
        if (lane == 0) {
            a.rows[4 * q] = (uint32_t)(e - b); a.rows[4 * q + 1] = (uint32_t)n_hit;
            a.rows[4 * q + 2] = (uint32_t)n_rep; a.rows[4 * q + 3] = (uint32_t)n_absent;
            const uint64_t first = a.base[b], last = a.base[e];
            const uint64_t n = last - first;
            const uint64_t place = n > SI_SORT_TILE ? __hip_atomic_fetch_add(a.ctr + kCtrLong, n, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) : 0;
            a.a_offsets[q] = first;
            a.seg_begin[q] = place;
            a.seg_end[q] = n > SI_SORT_TILE ? place + n : place;
        }
    }
}

// One ANCHOR per thread: its seed is the last one whose base is at or before it (a seed without anchors shares its base with the next),
// its occurrence the one that far into the key's range.  Seeds are visited in list order and a key's occurrences in (ref, rpos) order.
__global__ __launch_bounds__(SI_THREADS) void si_fill_kernel(MatchArgs a)
{
    for (uint64_t i = first_item(); i < a.n_anchors; i += item_step()) {
        const uint64_t s = si_at_or_before(a.base, a.n_seeds + 1, i) - 1;
        const uint64_t o = a.start[a.hit[s]] + (i - a.base[s]), e = a.lo + s;
        a.a_ref_rev[i] = si_ref_rev(a.ref[o], a.info[e]);
        a.a_rpos[i] = a.rpos[o];
        a.a_qpos[i] = (uint32_t)a.pos[e];
    }
}

// One block per read with 2 .. SI_SORT_TILE anchors: a bitonic sort in LDS of (key, qpos), padded to a power of two with the largest
// pair (a real anchor equal to the padding is equal to it in every word, so their order does not show).
__global__ __launch_bounds__(SI_THREADS) void si_sort_kernel(MatchArgs a)
{
    __shared__ uint64_t s_key[SI_SORT_TILE];
    __shared__ uint32_t s_qpos[SI_SORT_TILE];
    for (uint64_t q = blockIdx.x; q < a.n_reads; q += gridDim.x) {
        const uint64_t first = a.a_offsets[q];
        const uint64_t n = a.a_offsets[q + 1] - first;
        if (n < 2 || n > SI_SORT_TILE) continue;   // (the same for the whole block)
        uint32_t padded = 2;
        while (padded < n) padded *= 2;
        for (uint32_t i = threadIdx.x; i < padded; i += SI_THREADS) {
            s_key[i] = i < n ? si_sort_key(a.a_ref_rev[first + i], a.a_rpos[first + i]) : ~(uint64_t)0;
            s_qpos[i] = i < n ? a.a_qpos[first + i] : ~(uint32_t)0;
        }
        __syncthreads();
        for (uint32_t run = 2; run <= padded; run *= 2) {
            for (uint32_t j = run / 2; j > 0; j /= 2) {
                for (uint32_t t = threadIdx.x; t < padded / 2; t += SI_THREADS) {
                    const uint32_t lo = ((t & ~(j - 1)) << 1) | (t & (j - 1)), hi = lo | j;
                    const bool ascending = (lo & run) == 0;
                    const uint64_t k_lo = s_key[lo], k_hi = s_key[hi];
                    const uint32_t q_lo = s_qpos[lo], q_hi = s_qpos[hi];
                    if (si_before(k_hi, q_hi, k_lo, q_lo) == ascending) {
                        s_key[lo] = k_hi; s_key[hi] = k_lo;
                        s_qpos[lo] = q_hi; s_qpos[hi] = q_lo;
                    }
                }
                __syncthreads();
            }
        }
        for (uint32_t i = threadIdx.x; i < n; i += SI_THREADS) {
            a.a_ref_rev[first + i] = (uint32_t)(s_key[i] >> 32);
            a.a_rpos[first + i] = (uint32_t)s_key[i];
            a.a_qpos[first + i] = s_qpos[i];
        }
        __syncthreads();   // the LDS is free again
    }
}

// the anchors of the reads the segmented sort takes, as 64-bit keys and qpos in their compact segments, one block per read ...
__global__ __launch_bounds__(SI_THREADS) void si_widen_kernel(MatchArgs a, uint64_t *key, uint32_t *qpos)
{
    for (uint64_t q = blockIdx.x; q < a.n_reads; q += gridDim.x) {
        const uint64_t first = a.a_offsets[q], place = a.seg_begin[q], n = a.seg_end[q] - place;
        for (uint64_t j = threadIdx.x; j < n; j += SI_THREADS) {
            key[place + j] = si_sort_key(a.a_ref_rev[first + j], a.a_rpos[first + j]);
            qpos[place + j] = a.a_qpos[first + j];
        }
    }
}

// ... and back, sorted
__global__ __launch_bounds__(SI_THREADS) void si_narrow_kernel(MatchArgs a, const uint64_t *key, const uint32_t *qpos)
{
    for (uint64_t q = blockIdx.x; q < a.n_reads; q += gridDim.x) {
        const uint64_t first = a.a_offsets[q], place = a.seg_begin[q], n = a.seg_end[q] - place;
        for (uint64_t j = threadIdx.x; j < n; j += SI_THREADS) {
            a.a_ref_rev[first + j] = (uint32_t)(key[place + j] >> 32);
            a.a_rpos[first + j] = (uint32_t)key[place + j];
            a.a_qpos[first + j] = qpos[place + j];
        }
    }
}

}  // namespace

struct ntk_seed_index : Consumer {
    Pinned<uint64_t> h_stage;                              // kCtrWords words
    DeviceArray<uint64_t> d_keys;                          // the index: the distinct values ...
    DeviceArray<uint32_t> d_start, d_ref, d_rpos;          // ... the n_keys + 1 starts of their ranges, and the occurrences
    DeviceArray<uint32_t> d_a_ref_rev, d_a_rpos, d_a_qpos; // the match result: the anchors ...
    DeviceArray<uint64_t> d_a_offsets;                     // ... their n_reads + 1 ranges ...
    DeviceArray<uint32_t> d_rows;                          // ... and the rows
    DeviceArray<uint64_t> d_sorted;                        // the build's work: the sorted values ...
    DeviceArray<uint32_t> d_idx, d_perm, d_owner, d_head, d_rank;   // ... entry indices before and behind the sort, owners, heads, their scan
    DeviceArray<uint32_t> d_hit, d_count;                  // the match's work: per seed its key index and its anchors ...
    DeviceArray<uint64_t> d_base, d_seg_begin, d_seg_end;  // ... their scan; per read its segment of the long route's arrays
    DeviceArray<uint64_t> d_key_a, d_key_b;                // the long reads' keys, twice ...
    DeviceArray<uint32_t> d_qpos_a, d_qpos_b;              // ... and their qpos, twice
    DeviceArray<uint64_t> d_hist, d_ctr;                   // the spectrum's bins; kCtrWords words
    DeviceArray<char> d_tmp;                               // rocPRIM's temporary storage: held inside a build or a match only
    bool built = false, matched = false;                   // an index is held; a match result is held (n_reads may be 0)
    uint64_t n_refs = 0, n_occ = 0, n_keys = 0, max_occ = 0;          // of the index
    uint64_t n_reads = 0, n_seeds = 0, n_anchors = 0, n_held = 0;     // of the match: anchors it makes, anchors held
    int failed = 0;                                        // the status of a build or match that failed halfway

    uint64_t device_bytes() const
    {
        return d_keys.bytes() + d_start.bytes() + d_ref.bytes() + d_rpos.bytes() + d_a_ref_rev.bytes() + d_a_rpos.bytes() + d_a_qpos.bytes() +
               d_a_offsets.bytes() + d_rows.bytes() + d_sorted.bytes() + d_idx.bytes() + d_perm.bytes() + d_owner.bytes() + d_head.bytes() +
               d_rank.bytes() + d_hit.bytes() + d_count.bytes() + d_base.bytes() + d_seg_begin.bytes() + d_seg_end.bytes() + d_key_a.bytes() +
               d_key_b.bytes() + d_qpos_a.bytes() + d_qpos_b.bytes() + d_hist.bytes() + d_ctr.bytes() + d_tmp.bytes();
    }

    // the match result and every work array: the index stays
    void release_work()
    {
        d_a_ref_rev.release(); d_a_rpos.release(); d_a_qpos.release(); d_a_offsets.release(); d_rows.release();
        d_sorted.release(); d_idx.release(); d_perm.release(); d_owner.release(); d_head.release(); d_rank.release();
        d_hit.release(); d_count.release(); d_base.release(); d_seg_begin.release(); d_seg_end.release();
        d_key_a.release(); d_key_b.release(); d_qpos_a.release(); d_qpos_b.release();
        d_hist.release(); d_ctr.release(); d_tmp.release();
    }

    void release_index() { d_keys.release(); d_start.release(); d_ref.release(); d_rpos.release(); }
};

namespace {

using Handle = ntk_seed_index;

// what a call that takes a list refuses before any device call
int check_list(const Handle *m, const uint64_t *d_offsets, const uint64_t *d_pos, const uint64_t *d_values, const uint32_t *d_info,
               uint64_t n_records, uint64_t n)
{
    if (!m) return NTK_ERR_BAD_ARG;
    if ((n >> 32) || (n_records >> 31)) return NTK_ERR_BAD_ARG;
    if (!d_offsets || ((uintptr_t)d_offsets & 7)) return NTK_ERR_BAD_ARG;
    if (n && (!d_pos || !d_values || !d_info || ((uintptr_t)d_pos & 7) || ((uintptr_t)d_values & 7) || ((uintptr_t)d_info & 3))) return NTK_ERR_BAD_ARG;
    return NTK_OK;
}

// The verification on the device: NTK_OK with the list's entries [lo, hi) in the stage, or the refusal.  Nothing held is touched.
int verify(Handle *m, const uint64_t *d_offsets, const uint64_t *d_pos, uint64_t n_records, uint64_t n, uint64_t &lo, uint64_t &hi)
{
    int rc;
    hipStream_t st = m->stream;
    CT_HIPCHK(hipSetDevice(m->device));
    if ((rc = m->d_ctr.ensure(st, kCtrWords, grow_exact))) return rc;
    CT_HIPCHK(hipMemsetAsync(m->d_ctr.p, 0, kCtrWords * sizeof(uint64_t), st));
    const uint64_t items = n_records + 1 > n ? n_records + 1 : n;
    hipLaunchKernelGGL(si_verify_kernel, dim3(grid_for(items, SI_THREADS, (unsigned)m->n_cu * SI_BLOCKS_PER_CU)), dim3(SI_THREADS), 0, st,
                       d_offsets, n_records, d_pos, n, m->d_ctr.p);
    CT_HIPCHK(hipGetLastError());
    if ((rc = m->h_stage.read(st, m->d_ctr.p, kCtrWords))) return rc;
    if (m->h_stage.p[kCtrFlags] & SI_BAD_OFFSETS) return NTK_ERR_BAD_ARG;
    if (m->h_stage.p[kCtrFlags] & SI_BAD_POS) return NTK_ERR_UNSUPPORTED;
    lo = m->h_stage.p[kCtrLo]; hi = m->h_stage.p[kCtrHi];
    return NTK_OK;
}

inline unsigned grid_of(const Handle *m, uint64_t items, unsigned per_block = SI_THREADS)
{
    return grid_for(items, per_block, (unsigned)m->n_cu * SI_BLOCKS_PER_CU);
}

// the largest occ of the index, and with n_bins != 0 its spectrum in d_hist
int occ_pass(Handle *m, uint32_t n_bins)
{
    hipStream_t st = m->stream;
    CT_HIPCHK(hipMemsetAsync(m->d_ctr.p + kCtrMax, 0, sizeof(uint64_t), st));
    if (n_bins) CT_HIPCHK(hipMemsetAsync(m->d_hist.p, 0, n_bins * sizeof(uint64_t), st));
    hipLaunchKernelGGL(si_spectrum_kernel, dim3(grid_of(m, m->n_keys)), dim3(SI_THREADS), 0, st, m->d_start.p, m->n_keys, m->d_hist.p, n_bins,
                       m->d_ctr.p + kCtrMax);
    CT_HIPCHK(hipGetLastError());
    return m->h_stage.read(st, m->d_ctr.p + kCtrMax, 1, kCtrMax);
}

// rocPRIM's temporary storage is held inside a call only, so that what the handle holds between calls has no term of a size that
// only rocPRIM knows: freed when the call's work is done
void drop_tmp(Handle *m)
{
    if (!m->d_tmp.p) return;
    (void)hipStreamSynchronize(m->stream);
    m->d_tmp.release();
    (void)hipGetLastError();
}

// the whole build behind the verification; a failure in here marks the handle
int build(Handle *m, const uint64_t *d_offsets, const uint64_t *d_pos, const uint64_t *d_values, const uint32_t *d_info, uint64_t n_refs,
          uint64_t lo, uint64_t n)
{
    int rc;
    hipStream_t st = m->stream;
    if ((rc = m->d_sorted.ensure(st, n, grow_exact)) || (rc = m->d_idx.ensure(st, n, grow_exact)) || (rc = m->d_perm.ensure(st, n, grow_exact)) ||
        (rc = m->d_owner.ensure(st, n, grow_exact)) || (rc = m->d_head.ensure(st, n, grow_exact)) || (rc = m->d_rank.ensure(st, n, grow_exact)))
        return rc;
    uint64_t n_keys = 0;
    if (n) {
        hipLaunchKernelGGL(si_owner_kernel, dim3(grid_of(m, n)), dim3(SI_THREADS), 0, st, d_offsets, n_refs, lo, n, m->d_owner.p, m->d_idx.p);
        CT_HIPCHK(hipGetLastError());
        rc = with_tmp(m->d_tmp, st, grow_exact, [&](void *tmp, size_t &bytes) {
            return rocprim::radix_sort_pairs(tmp, bytes, d_values + lo, m->d_sorted.p, m->d_idx.p, m->d_perm.p, (size_t)n, 0u, 64u, st);
        });
        if (rc) return rc;
        hipLaunchKernelGGL(si_heads_kernel, dim3(grid_of(m, n)), dim3(SI_THREADS), 0, st, m->d_sorted.p, n, m->d_head.p);
        CT_HIPCHK(hipGetLastError());
        rc = with_tmp(m->d_tmp, st, grow_exact, [&](void *tmp, size_t &bytes) {
            return rocprim::inclusive_scan(tmp, bytes, m->d_head.p, m->d_rank.p, (size_t)n, rocprim::plus<uint32_t>(), st);
        });
        if (rc) return rc;
        CT_HIPCHK(hipMemcpyAsync(m->h_stage.p, m->d_rank.p + (n - 1), sizeof(uint32_t), hipMemcpyDeviceToHost, st));
        CT_HIPCHK(hipStreamSynchronize(st));
        n_keys = *(const uint32_t *)m->h_stage.p;
    }
    if ((rc = m->d_keys.ensure(st, n_keys, grow_exact)) || (rc = m->d_start.ensure(st, n_keys + 1, grow_exact)) ||
        (rc = m->d_ref.ensure(st, n, grow_exact)) || (rc = m->d_rpos.ensure(st, n, grow_exact)))
        return rc;
    m->n_keys = n_keys;   // (occ_pass reads it; the counts are the handle's once the build has succeeded)
    if (!n) {
        CT_HIPCHK(hipMemsetAsync(m->d_start.p, 0, sizeof(uint32_t), st));
        CT_HIPCHK(hipStreamSynchronize(st));
        return NTK_OK;
    }
    PackArgs a;
    a.sorted = m->d_sorted.p; a.pos = d_pos; a.perm = m->d_perm.p; a.owner = m->d_owner.p; a.head = m->d_head.p; a.rank = m->d_rank.p;
    a.info = d_info; a.lo = lo; a.m = n; a.n_keys = n_keys;
    a.keys = m->d_keys.p; a.start = m->d_start.p; a.ref = m->d_ref.p; a.rpos = m->d_rpos.p;
    hipLaunchKernelGGL(si_pack_kernel, dim3(grid_of(m, n)), dim3(SI_THREADS), 0, st, a);
    CT_HIPCHK(hipGetLastError());
    if ((rc = occ_pass(m, 0))) return rc;
    m->max_occ = m->h_stage.p[kCtrMax];
    return NTK_OK;
}

// Both segmented sorts of the reads with more than SI_SORT_TILE anchors, n anchors in all, on a compact copy of them: by qpos, then -
// stable - by the 64-bit key.
int sort_long_reads(Handle *m, const MatchArgs &a, uint64_t n)
{
    int rc;
    hipStream_t st = m->stream;
    if ((rc = m->d_key_a.ensure(st, n, grow_exact)) || (rc = m->d_key_b.ensure(st, n, grow_exact)) || (rc = m->d_qpos_a.ensure(st, n, grow_exact)) ||
        (rc = m->d_qpos_b.ensure(st, n, grow_exact)))
        return rc;
    const unsigned blocks = grid_of(m, a.n_reads, 1);
    hipLaunchKernelGGL(si_widen_kernel, dim3(blocks), dim3(SI_THREADS), 0, st, a, m->d_key_a.p, m->d_qpos_a.p);
    CT_HIPCHK(hipGetLastError());
    rc = with_tmp(m->d_tmp, st, grow_exact, [&](void *tmp, size_t &bytes) {
        return rocprim::segmented_radix_sort_pairs(tmp, bytes, m->d_qpos_a.p, m->d_qpos_b.p, m->d_key_a.p, m->d_key_b.p, (unsigned)n,
                                                   (unsigned)a.n_reads, a.seg_begin, a.seg_end, 0u, 32u, st);
    });
    if (rc) return rc;
    rc = with_tmp(m->d_tmp, st, grow_exact, [&](void *tmp, size_t &bytes) {
        return rocprim::segmented_radix_sort_pairs(tmp, bytes, m->d_key_b.p, m->d_key_a.p, m->d_qpos_b.p, m->d_qpos_a.p, (unsigned)n,
                                                   (unsigned)a.n_reads, a.seg_begin, a.seg_end, 0u, 64u, st);
    });
    if (rc) return rc;
    hipLaunchKernelGGL(si_narrow_kernel, dim3(blocks), dim3(SI_THREADS), 0, st, a, m->d_key_a.p, m->d_qpos_a.p);
    CT_HIPCHK(hipGetLastError());
    return NTK_OK;
}

// the whole match behind the verification; a failure in here marks the handle
int match(Handle *m, const uint64_t *d_offsets, const uint64_t *d_pos, const uint64_t *d_values, const uint32_t *d_info, uint64_t n_reads,
          uint64_t lo, uint64_t n_seeds, uint32_t max_occ, uint64_t max_anchors)
{
    int rc;
    hipStream_t st = m->stream;
    if ((rc = m->d_hit.ensure(st, n_seeds, grow_exact)) || (rc = m->d_count.ensure(st, n_seeds + 1, grow_exact)) ||
        (rc = m->d_base.ensure(st, n_seeds + 1, grow_exact)) || (rc = m->d_seg_begin.ensure(st, n_reads, grow_exact)) ||
        (rc = m->d_seg_end.ensure(st, n_reads, grow_exact)) ||
        (rc = m->d_a_offsets.ensure(st, n_reads + 1, grow_exact)) || (rc = m->d_rows.ensure(st, 4 * n_reads, grow_exact)))
        return rc;
    MatchArgs a;
    a.offsets = d_offsets; a.pos = d_pos; a.values = d_values; a.info = d_info;
    a.n_reads = n_reads; a.lo = lo; a.n_seeds = n_seeds;
    a.keys = m->d_keys.p; a.start = m->d_start.p; a.ref = m->d_ref.p; a.rpos = m->d_rpos.p; a.n_keys = m->n_keys;
    a.max_occ = max_occ;
    a.hit = m->d_hit.p; a.count = m->d_count.p; a.base = m->d_base.p;
    a.a_offsets = m->d_a_offsets.p; a.seg_begin = m->d_seg_begin.p; a.seg_end = m->d_seg_end.p; a.rows = m->d_rows.p; a.ctr = m->d_ctr.p;
    a.n_anchors = 0; a.a_ref_rev = a.a_rpos = a.a_qpos = nullptr;
    CT_HIPCHK(hipMemsetAsync(m->d_ctr.p + kCtrLong, 0, sizeof(uint64_t), st));
    hipLaunchKernelGGL(si_lookup_kernel, dim3(grid_of(m, n_seeds + 1)), dim3(SI_THREADS), 0, st, a);
    CT_HIPCHK(hipGetLastError());
    rc = with_tmp(m->d_tmp, st, grow_exact, [&](void *tmp, size_t &bytes) {
        return rocprim::exclusive_scan(tmp, bytes, m->d_count.p, m->d_base.p, (uint64_t)0, (size_t)(n_seeds + 1), rocprim::plus<uint64_t>(), st);
    });
    if (rc) return rc;
    hipLaunchKernelGGL(si_rows_kernel, dim3(grid_of(m, n_reads + 1, SI_THREADS / 64)), dim3(SI_THREADS), 0, st, a);
    CT_HIPCHK(hipGetLastError());
    CT_HIPCHK(hipMemcpyAsync(m->h_stage.p, m->d_base.p + n_seeds, sizeof(uint64_t), hipMemcpyDeviceToHost, st));
    if ((rc = m->h_stage.read(st, m->d_ctr.p + kCtrLong, 1, kCtrLong))) return rc;
    const uint64_t total = m->h_stage.p[0], n_long = m->h_stage.p[kCtrLong];
    m->n_anchors = total;
    if ((max_anchors && total > max_anchors) || (total >> 32)) {
        // the rows stay; the ranges are emptied, since no anchor is held
        CT_HIPCHK(hipMemsetAsync(m->d_a_offsets.p, 0, (n_reads + 1) * sizeof(uint64_t), st));
        CT_HIPCHK(hipStreamSynchronize(st));
        return NTK_ERR_CAPACITY;
    }
    if ((rc = m->d_a_ref_rev.ensure(st, total, grow_half_again)) || (rc = m->d_a_rpos.ensure(st, total, grow_half_again)) ||
        (rc = m->d_a_qpos.ensure(st, total, grow_half_again)))
        return rc;
    m->n_held = total;
    if (total) {
        a.n_anchors = total; a.a_ref_rev = m->d_a_ref_rev.p; a.a_rpos = m->d_a_rpos.p; a.a_qpos = m->d_a_qpos.p;
        hipLaunchKernelGGL(si_fill_kernel, dim3(grid_of(m, total)), dim3(SI_THREADS), 0, st, a);
        CT_HIPCHK(hipGetLastError());
        hipLaunchKernelGGL(si_sort_kernel, dim3(grid_of(m, n_reads, 1)), dim3(SI_THREADS), 0, st, a);
        CT_HIPCHK(hipGetLastError());
        if (n_long && (rc = sort_long_reads(m, a, n_long))) return rc;
    }
    CT_HIPCHK(hipStreamSynchronize(st));
    return NTK_OK;
}

}  // namespace

extern "C" {

int ntk_seed_index_create(ntk_ctx *ctx, ntk_seed_index **out)
{
    if (!ctx || !out) return NTK_ERR_BAD_ARG;
    *out = nullptr;
    ntk_seed_index *m = new (std::nothrow) ntk_seed_index();
    if (!m) return NTK_ERR_NOMEM;
    int rc = m->bind(ctx, 0, 0);
    if (rc) { delete m; return rc; }
    if ((rc = m->h_stage.alloc(kCtrWords))) { delete m; return rc; }
    *out = m;
    return NTK_OK;
}

int ntk_seed_index_trim(ntk_seed_index *m)
{
    if (!m) return NTK_ERR_BAD_ARG;
    CT_HIPCHK(hipSetDevice(m->device));
    CT_HIPCHK(hipStreamSynchronize(m->stream));
    m->release_work();
    (void)hipGetLastError();
    m->matched = false;
    m->n_reads = m->n_seeds = m->n_anchors = m->n_held = 0;
    m->failed = 0;
    return NTK_OK;
}

void ntk_seed_index_destroy(ntk_seed_index *m)
{
    if (!m) return;
    (void)ntk_seed_index_trim(m);
    m->release_index();
    m->h_stage.release();
    (void)hipGetLastError();
    delete m;
}

int ntk_seed_index_build_device(ntk_seed_index *m, const uint64_t *d_offsets, const uint64_t *d_pos, const uint64_t *d_values,
                                const uint32_t *d_info, uint64_t n_refs, uint64_t n_entries)
{
    int rc = check_list(m, d_offsets, d_pos, d_values, d_info, n_refs, n_entries);
    if (rc) return rc;
    uint64_t lo = 0, hi = 0;
    if ((rc = verify(m, d_offsets, d_pos, n_refs, n_entries, lo, hi))) return rc;
    // the build starts over: neither the index held so far nor a match against it is part of the new state
    m->built = m->matched = false; m->failed = 0;
    m->n_refs = m->n_occ = m->n_keys = m->max_occ = 0;
    m->n_reads = m->n_seeds = m->n_anchors = m->n_held = 0;
    m->release_index();   // (the verification left the stream idle) the index arrays are those of the index held, never larger
    rc = build(m, d_offsets, d_pos, d_values, d_info, n_refs, lo, hi - lo);
    drop_tmp(m);
    if (rc) {
        m->failed = rc;
        m->n_keys = m->max_occ = 0;
    } else {
        m->built = true;
        m->n_refs = n_refs; m->n_occ = hi - lo;
    }
    return rc;
}

int ntk_seed_index_spectrum(ntk_seed_index *m, uint64_t *hist, uint32_t n_bins)
{
    if (!m || !hist || n_bins < 2 || !m->built) return NTK_ERR_BAD_ARG;
    int rc;
    CT_HIPCHK(hipSetDevice(m->device));
    if ((rc = m->d_hist.ensure(m->stream, n_bins, grow_exact)) || (rc = m->d_ctr.ensure(m->stream, kCtrWords, grow_exact)) || (rc = occ_pass(m, n_bins)))
        return rc;
    CT_HIPCHK(hipMemcpyAsync(hist, m->d_hist.p, n_bins * sizeof(uint64_t), hipMemcpyDeviceToHost, m->stream));
    CT_HIPCHK(hipStreamSynchronize(m->stream));
    return NTK_OK;
}

int ntk_seed_index_match_device(ntk_seed_index *m, const uint64_t *d_offsets, const uint64_t *d_pos, const uint64_t *d_values,
                                const uint32_t *d_info, uint64_t n_reads, uint64_t n_entries, uint32_t max_occ, uint64_t max_anchors)
{
    int rc = check_list(m, d_offsets, d_pos, d_values, d_info, n_reads, n_entries);
    if (rc) return rc;
    if (!m->built) return NTK_ERR_BAD_ARG;
    uint64_t lo = 0, hi = 0;
    if ((rc = verify(m, d_offsets, d_pos, n_reads, n_entries, lo, hi))) return rc;
    // the match starts over: nothing of the result held so far is part of the new one
    m->matched = true; m->failed = 0;
    m->n_reads = n_reads; m->n_seeds = hi - lo;
    m->n_anchors = m->n_held = 0;
    rc = match(m, d_offsets, d_pos, d_values, d_info, n_reads, lo, hi - lo, max_occ, max_anchors);
    drop_tmp(m);
    if (rc && rc != NTK_ERR_CAPACITY) m->failed = rc;
    return rc;
}

int ntk_seed_index_read(ntk_seed_index *m, uint64_t *a_offsets, uint32_t *ref_rev, uint32_t *rpos, uint32_t *qpos, uint32_t *rows, uint64_t cap,
                        uint64_t *n)
{
    if (!m || !n || (cap && (!ref_rev || !rpos || !qpos))) return NTK_ERR_BAD_ARG;
    if (m->failed) return m->failed;
    *n = m->matched ? m->n_held : 0;
    if (!m->matched) return NTK_OK;
    if (m->n_held > cap) return NTK_ERR_CAPACITY;
    if (!a_offsets) return NTK_OK;   // the size alone
    CT_HIPCHK(hipSetDevice(m->device));
    CT_HIPCHK(hipMemcpyAsync(a_offsets, m->d_a_offsets.p, (m->n_reads + 1) * sizeof(uint64_t), hipMemcpyDeviceToHost, m->stream));
    if (rows && m->n_reads) CT_HIPCHK(hipMemcpyAsync(rows, m->d_rows.p, 4 * m->n_reads * sizeof(uint32_t), hipMemcpyDeviceToHost, m->stream));
    if (m->n_held) {
        CT_HIPCHK(hipMemcpyAsync(ref_rev, m->d_a_ref_rev.p, m->n_held * sizeof(uint32_t), hipMemcpyDeviceToHost, m->stream));
        CT_HIPCHK(hipMemcpyAsync(rpos, m->d_a_rpos.p, m->n_held * sizeof(uint32_t), hipMemcpyDeviceToHost, m->stream));
        CT_HIPCHK(hipMemcpyAsync(qpos, m->d_a_qpos.p, m->n_held * sizeof(uint32_t), hipMemcpyDeviceToHost, m->stream));
    }
    CT_HIPCHK(hipStreamSynchronize(m->stream));
    return NTK_OK;
}

int ntk_seed_index_result_device(ntk_seed_index *m, const uint64_t **d_a_offsets, const uint32_t **d_ref_rev, const uint32_t **d_rpos,
                                 const uint32_t **d_qpos, const uint32_t **d_rows, uint64_t *n)
{
    if (!m || !d_a_offsets || !d_ref_rev || !d_rpos || !d_qpos || !d_rows || !n) return NTK_ERR_BAD_ARG;
    if (m->failed) return m->failed;
    const bool any = m->matched && m->n_held;
    *d_a_offsets = m->matched ? m->d_a_offsets.p : nullptr;
    *d_rows = m->matched && m->n_reads ? m->d_rows.p : nullptr;
    *d_ref_rev = any ? m->d_a_ref_rev.p : nullptr;
    *d_rpos = any ? m->d_a_rpos.p : nullptr;
    *d_qpos = any ? m->d_a_qpos.p : nullptr;
    *n = m->matched ? m->n_held : 0;
    return NTK_OK;
}

int ntk_seed_index_stats(ntk_seed_index *m, struct ntk_seed_index_stats *out)
{
    if (!m || !out) return NTK_ERR_BAD_ARG;
    if (m->failed) return m->failed;
    CT_HIPCHK(hipSetDevice(m->device));
    CT_HIPCHK(hipStreamSynchronize(m->stream));
    out->n_refs = m->n_refs; out->n_entries = m->n_occ; out->n_keys = m->n_keys; out->max_occ = m->max_occ;
    out->n_reads = m->n_reads; out->n_seeds = m->n_seeds; out->n_anchors = m->n_anchors;
    out->device_bytes = m->device_bytes();
    return NTK_OK;
}

}  // extern "C"
