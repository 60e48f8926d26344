// Primary and secondary chains and their mapping quality (include_pending/needletail_amd/mapping.h): minimap2's mm_set_parent with a
// hard mask level, mm_select_sub and its chain-only mapping quality, over the per-read CSR of chains the chain library leaves on the
// device.  A consumer of the core's public ABI on the shared scaffold (ntk_consumer.hpp); it reads chain and anchor arrays alone, never
// a base, and links nothing but the core.
//
// run_device: verify the arrays (mp_verify_kernel; mp_span_kernel without writing where a blen could not be bounded), compute the
// per-chain fields with one wave per chain (mp_span_kernel), rank every read's chains by (score descending, index ascending) with one
// segmented radix sort of 64-bit keys (mp_keys_kernel, rocPRIM), find links, parents, secondaries and mapping qualities with one wave per
// read (mp_parent_kernel), scan the reported counts (rocPRIM), read the total back - out grows there - and write out (mp_emit_kernel).
// rocPRIM's temporary storage is held inside a call only.  The rule is ntk_map_rule.hpp's.  DESIGN.md section 25.
#include "../../include_pending/needletail_amd/mapping.h"
#include "ntk_consumer.hpp"
#include "ntk_map_rule.hpp"

#include <rocprim/device/device_scan.hpp>
#include <rocprim/device/device_segmented_radix_sort.hpp>

#include <new>

namespace {

// the counter words: what the verification raised, the first and last chain of a read, and what the parent kernel counted
constexpr int kCtrFlags = 0, kCtrLo = 1, kCtrHi = 2, kCtrPrimary = 3, kCtrSecondary = 4, kCtrMost = 5, kCtrWords = 6;
constexpr uint32_t kWaves = MP_THREADS / 64;

static_assert(MP_THREADS == kThreads, "the blocks of the scaffold");
static_assert(sizeof(struct ntk_mapping_params) == 32 && sizeof(struct ntk_mapping_stats) == 64, "the header's struct sizes");

__device__ inline void or_agent(uint64_t *p, uint64_t v) { (void)__hip_atomic_fetch_or(p, v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT); }
__device__ inline void max_agent(uint64_t *p, uint64_t v) { (void)__hip_atomic_fetch_max(p, v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT); }
__device__ inline void add_word(uint32_t *p, uint32_t v) { (void)__hip_atomic_fetch_add(p, v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT); }
__device__ inline void max_word(uint32_t *p, uint32_t v) { (void)__hip_atomic_fetch_max(p, v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT); }
__device__ inline uint32_t load_word(const uint32_t *p) { return __hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT); }

// What one lane of a wave stored, or added to a row, is seen by the loads of the other lanes behind this.  A fence of workgroup scope is
// enough for lanes of one wave and compiles to no instruction on gfx950, where the memory operations of one compute unit stay in order;
// one of agent scope (__threadfence) is buffer_wbl2 sc1, s_waitcnt vmcnt(0), buffer_inv sc1 - an L2 write-back and an L1 invalidation,
// 20 ms of a 22 ms run on 1 M reads when every read paid one (profiles/mapping/README.md)
__device__ inline void wave_fence()
{
    __builtin_amdgcn_fence(__ATOMIC_SEQ_CST, "workgroup");
    __builtin_amdgcn_wave_barrier();
}

__device__ inline uint64_t first_item() { return (uint64_t)blockIdx.x * MP_THREADS + threadIdx.x; }
__device__ inline uint64_t item_step() { return (uint64_t)gridDim.x * MP_THREADS; }

struct MapArgs {
    const uint64_t *c_offsets;                // the chains: n_reads + 1 offsets ...
    const uint32_t *chain_rows;               // ... n_chains rows of eight words ...
    const uint64_t *m_offsets;                // ... their n_chains + 1 member ranges ...
    const uint32_t *members;                  // ... and n_members members,
    const uint32_t *rpos, *qpos;              // indices into the n_anchors anchors
    uint64_t n_reads, n_chains, n_members, n_anchors, lo, hi;   // the chains of the reads are [lo, hi)
    mp_rule_params r;
    uint32_t *rows, *order;                   // the result per chain
    uint64_t *keys, *sorted;                  // the rank keys before and behind the sort; `keys` then holds qe << 32 | qs in rank order
    uint32_t *par, *slot;                     // per chain: the rank of its parent (under its rank), its place among its read's reported
    uint32_t *n_out;                          // per read: its reported chains
    uint64_t *out_offsets;                    // their scan
    uint32_t *out, *read_rows;
    uint64_t *ctr;
};

// The arrays as the rule reads them, one offset, one chain and one member per thread; ctr is zeroed before.  c_offsets[0] and
// c_offsets[n_reads] are read before they are known to be good: they only select the chains that are looked at, every one of them below
// n_chains.  A chain's members are read only where its range lies inside the members, a member's anchor only where it is below
// n_anchors, and the search of a member's chain stays inside m_offsets whatever they hold.
__global__ __launch_bounds__(MP_THREADS) void mp_verify_kernel(MapArgs a)
{
    const uint64_t lo = a.c_offsets[0], end = a.c_offsets[a.n_reads], hi = end < a.n_chains ? end : a.n_chains;
    uint64_t items = a.n_reads > a.n_chains ? a.n_reads : a.n_chains;
    items = (items + 1 > a.n_members) ? items + 1 : a.n_members;
    uint32_t bad = 0;
    for (uint64_t i = first_item(); i < items; i += item_step()) {
        if (i < a.n_reads) {
            const uint64_t b = a.c_offsets[i], e = a.c_offsets[i + 1];
            if (b > e) bad |= MP_BAD_OFFSETS;
            else if (e - b >= MP_READ_CHAINS) bad |= MP_MANY_CHAINS;
        }
        if (i == a.n_reads && a.c_offsets[i] > a.n_chains) bad |= MP_BAD_OFFSETS;
        if (i < a.n_chains && a.m_offsets[i] > a.m_offsets[i + 1]) bad |= MP_BAD_OFFSETS;
        if (i == a.n_chains && a.m_offsets[i] > a.n_members) bad |= MP_BAD_OFFSETS;
        if (i < a.n_chains && i >= lo && i < hi) {   // a chain of a read
            const uint64_t b = a.m_offsets[i], e = a.m_offsets[i + 1];
            const uint32_t score = a.chain_rows[8 * i];
            if (score < 1 || score > MP_SCORE_MAX) bad |= MP_BAD_SCORE;
            if (b >= e) bad |= MP_NO_MEMBER;
            else if (e <= a.n_members) {
                const uint32_t first = a.members[b], last = a.members[e - 1];
                if (first < a.n_anchors && last < a.n_anchors) {
                    const uint64_t r0 = a.rpos[first], r1 = a.rpos[last], q0 = a.qpos[first], q1 = a.qpos[last];
                    const uint64_t q_hi = q0 > q1 ? q0 : q1, q_lo = q0 > q1 ? q1 : q0;
                    if (r1 + a.r.k > 0xFFFFFFFFull || q_hi + a.r.k > 0xFFFFFFFFull) bad |= MP_LONG_END;
                    // blen = k + the sum of max(dr, dq) is at most k + the sum of dr + the sum of dq
                    else if (r1 >= r0 && a.r.k + (r1 - r0) + (q_hi - q_lo) > 0xFFFFFFFFull) bad |= MP_MAYBE_BLEN;
                }
            }
        }
        if (i < a.n_members) {
            const uint64_t at = mp_at_or_before(a.m_offsets, a.n_chains + 1, i);   // the member's chain is at - 1
            if (at >= 1 && at <= a.n_chains && at - 1 >= lo && at - 1 < hi) {
                const uint64_t c = at - 1;
                const uint32_t m = a.members[i];
                if (m >= a.n_anchors) bad |= MP_BAD_MEMBER;
                else if (i > a.m_offsets[c]) {   // (not the chain's first: member i - 1 is the chain's too)
                    const uint32_t prev = a.members[i - 1];
                    if (prev < a.n_anchors) {
                        int64_t dr, dq;
                        mp_step(a.chain_rows[8 * c + 2] & 1, a.rpos[prev], a.qpos[prev], a.rpos[m], a.qpos[m], dr, dq);
                        if (dr < 1 || dq < 1) bad |= MP_BAD_ORDER;
                    }
                }
            }
        }
    }
    if (bad) or_agent(a.ctr + kCtrFlags, bad);
    if (first_item() == 0) { a.ctr[kCtrLo] = lo; a.ctr[kCtrHi] = hi; }
}

// The per-chain fields, one wave per chain of verified arrays: lanes stride over the chain's consecutive member pairs and a wave sum
// gives mlen and blen.  write == 0: nothing is written and a blen that does not fit a u32 raises MP_LONG_BLEN.  write != 0: lane 0
// writes the chain's row, its parent, subsc, n_sub, mapq, flags and rank as zeros; a chain of no read gets a row of zeros.
__global__ __launch_bounds__(MP_THREADS) void mp_span_kernel(MapArgs a, uint32_t write)
{
    const uint32_t wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
    const uint64_t waves = (uint64_t)gridDim.x * kWaves;
    for (uint64_t c = (uint64_t)blockIdx.x * kWaves + wave; c < a.n_chains; c += waves) {
        uint32_t *row = a.rows + MP_ROW_WORDS * c;
        if (c < a.lo || c >= a.hi) {
            if (write && lane < MP_ROW_WORDS) row[lane] = 0;
            continue;
        }
        const uint64_t b = a.m_offsets[c], e = a.m_offsets[c + 1];
        const uint32_t ref_rev = a.chain_rows[8 * c + 2];
        uint64_t mlen = 0, blen = 0;
        for (uint64_t t = b + 1 + lane; t < e; t += 64) {
            const uint32_t j = a.members[t - 1], i = a.members[t];
            int64_t dr, dq;
            mp_step(ref_rev & 1, a.rpos[j], a.qpos[j], a.rpos[i], a.qpos[i], dr, dq);
            mlen += mp_step_mlen(dr, dq, a.r.k);
            blen += mp_step_blen(dr, dq);
        }
        mlen = wave_sum(mlen) + a.r.k;
        blen = wave_sum(blen) + a.r.k;
        if (lane != 0) continue;
        if (!write) {
            if (blen > 0xFFFFFFFFull) or_agent(a.ctr + kCtrFlags, MP_LONG_BLEN);
            continue;
        }
        const uint32_t first = a.members[b], last = a.members[e - 1];
        const uint32_t q0 = a.qpos[first], q1 = a.qpos[last];
        row[MP_QS] = q0 < q1 ? q0 : q1; row[MP_QE] = (q0 < q1 ? q1 : q0) + a.r.k;
        row[MP_RS] = a.rpos[first]; row[MP_RE] = a.rpos[last] + a.r.k;
        row[MP_REF_REV] = ref_rev; row[MP_SCORE] = a.chain_rows[8 * c]; row[MP_CNT] = (uint32_t)(e - b);
        row[MP_MLEN] = (uint32_t)mlen; row[MP_BLEN] = (uint32_t)blen;
        for (uint32_t w = MP_PARENT; w < MP_ROW_WORDS; w++) row[w] = 0;
    }
}

// the rank key of every chain; order is zeroed for the chains of no read
__global__ __launch_bounds__(MP_THREADS) void mp_keys_kernel(MapArgs a)
{
    for (uint64_t c = first_item(); c < a.n_chains; c += item_step()) {
        a.keys[c] = mp_rank_key(a.chain_rows[8 * c], (uint32_t)c);
        a.order[c] = 0;
    }
}

// Links, parents, secondaries and mapping qualities, one wave per read.  The read's n < 2^16 intervals are staged in rank order, in the
// wave's LDS where n <= MP_LDS_CHAINS and in the work arrays otherwise (a.keys, free since the sort, and a.par): the same loop through
// generic pointers, with a fence (wave_fence) where another lane's global store is read.  Then
//   for every rank i in order: lane l tests rank 64 s + l of every strip s below i; the first set bit of the first ballot that is not
//     empty is link, and par[i] = link is none ? i : par[link], known since link < i;
//   for the ranks 64 at a time: the eligible chains in front of each by a ballot, parent, flags, rank and the place among the reported
//     written, every child added to its primary's n_sub and subsc (atomics on the rows: the children of a primary lie in any lane);
//   for every primary: its mapq from the finished n_sub and subsc.
// Lane 0 writes the read's row and its reported count; the thread of item n_reads closes the counts for their scan.
__global__ __launch_bounds__(MP_THREADS) void mp_parent_kernel(MapArgs a)
{
    __shared__ uint64_t s_iv[kWaves][MP_LDS_CHAINS];
    __shared__ uint32_t s_par[kWaves][MP_LDS_CHAINS];
    const uint32_t wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
    const uint64_t waves = (uint64_t)gridDim.x * kWaves, below = ((uint64_t)1 << lane) - 1;
    uint64_t n_primary = 0, n_secondary = 0;
    uint32_t most = 0;
    if (first_item() == 0) a.n_out[a.n_reads] = 0;
    for (uint64_t q = (uint64_t)blockIdx.x * kWaves + wave; q < a.n_reads; q += waves) {
        const uint64_t b = a.c_offsets[q];
        const uint32_t n = (uint32_t)(a.c_offsets[q + 1] - b);
        const bool in_lds = n <= MP_LDS_CHAINS;
        volatile uint64_t *iv = in_lds ? s_iv[wave] : a.keys + b;
        volatile uint32_t *par = in_lds ? s_par[wave] : a.par + b;
        most = n > most ? n : most;
        for (uint32_t r = lane; r < n; r += 64) {
            const uint32_t c = (uint32_t)a.sorted[b + r];
            a.order[b + r] = c;
            iv[r] = (uint64_t)a.rows[MP_ROW_WORDS * (uint64_t)c + MP_QE] << 32 | a.rows[MP_ROW_WORDS * (uint64_t)c + MP_QS];
        }
        if (in_lds) __builtin_amdgcn_wave_barrier(); else wave_fence();
        for (uint32_t i = 0; i < n; i++) {
            const uint64_t me = iv[i];
            uint32_t link = MP_NONE;
            for (uint32_t s = 0; s < i; s += 64) {
                const uint32_t j = s + lane;
                bool hit = false;
                if (j < i) {
                    const uint64_t it = iv[j];
                    hit = mp_overlap((uint32_t)me, (uint32_t)(me >> 32), (uint32_t)it, (uint32_t)(it >> 32), a.r.mask_level_pm);
                }
                const uint64_t hits = __ballot(hit);
                if (hits) { link = s + (uint32_t)__ffsll((unsigned long long)hits) - 1; break; }
            }
            const uint32_t p = link == MP_NONE ? i : par[link];
            if (lane == 0) par[i] = p;
            if (in_lds) __builtin_amdgcn_wave_barrier(); else wave_fence();
        }
        uint32_t eligible_before = 0, out_before = 0, primaries = 0;
        for (uint32_t s = 0; s < n; s += 64) {
            const uint32_t r = s + lane;
            bool primary = false, eligible = false;
            uint32_t c = 0, pc = 0, score = 0;
            if (r < n) {
                const uint32_t pr = par[r];
                c = (uint32_t)a.sorted[b + r]; pc = (uint32_t)a.sorted[b + pr];
                score = a.rows[MP_ROW_WORDS * (uint64_t)c + MP_SCORE];
                primary = pr == r;
                eligible = !primary && mp_eligible(score, a.rows[MP_ROW_WORDS * (uint64_t)pc + MP_SCORE], a.r.pri_ratio_pm);
            }
            const uint64_t el = __ballot(eligible);
            const bool kept = eligible && eligible_before + (uint32_t)__popcll(el & below) < a.r.best_n;
            const uint64_t rep = __ballot(primary || kept);
            if (r < n) {
                uint32_t *row = a.rows + MP_ROW_WORDS * (uint64_t)c, *prow = a.rows + MP_ROW_WORDS * (uint64_t)pc;
                row[MP_PARENT] = pc; row[MP_FLAGS] = primary ? MP_PRIMARY : kept ? MP_SECONDARY : 0; row[MP_RANK] = r;
                a.slot[c] = primary || kept ? out_before + (uint32_t)__popcll(rep & below) : MP_NONE;
                if (!primary) { add_word(prow + MP_N_SUB, 1); max_word(prow + MP_SUBSC, score); }
            }
            eligible_before += (uint32_t)__popcll(el); out_before += (uint32_t)__popcll(rep);
            primaries += (uint32_t)__popcll(__ballot(primary));
        }
        wave_fence();
        uint32_t top = 0;
        for (uint32_t r = lane; r < n; r += 64) {
            if (par[r] != r) continue;
            uint32_t *row = a.rows + MP_ROW_WORDS * (uint64_t)(uint32_t)a.sorted[b + r];
            const uint32_t mapq = mp_mapq(row[MP_SCORE], row[MP_CNT], load_word(row + MP_SUBSC), load_word(row + MP_N_SUB), a.r.min_chain_score);
            row[MP_MAPQ] = mapq;
            if (r == 0) top = mapq;
        }
        __builtin_amdgcn_wave_barrier();   // the next read's staging follows this read's last look at par
        if (lane == 0) {
            a.read_rows[4 * q] = n; a.read_rows[4 * q + 1] = primaries; a.read_rows[4 * q + 2] = out_before - primaries; a.read_rows[4 * q + 3] = top;
            a.n_out[q] = out_before;
        }
        n_primary += primaries; n_secondary += out_before - primaries;
    }
    if (lane == 0) {
        if (n_primary) add_agent(a.ctr + kCtrPrimary, n_primary);
        if (n_secondary) add_agent(a.ctr + kCtrSecondary, n_secondary);
        if (most) max_agent(a.ctr + kCtrMost, most);
    }
}

// out: a reported chain goes to its place behind its read's offset; its read by a binary search of c_offsets
__global__ __launch_bounds__(MP_THREADS) void mp_emit_kernel(MapArgs a)
{
    for (uint64_t c = a.lo + first_item(); c < a.hi; c += item_step()) {
        const uint32_t place = a.slot[c];
        if (place == MP_NONE) continue;
        const uint64_t q = mp_at_or_before(a.c_offsets, a.n_reads + 1, c) - 1;
        a.out[a.out_offsets[q] + place] = (uint32_t)c;
    }
}

}  // namespace

struct ntk_mapping : Consumer {
    Pinned<uint64_t> h_stage;                              // kCtrWords words
    DeviceArray<uint32_t> d_rows, d_order;                 // the result: per chain its row and, under c_offsets, the chains by rank
    DeviceArray<uint64_t> d_out_offsets;                   // the n_reads + 1 ranges of the reads' reported chains ...
    DeviceArray<uint32_t> d_out, d_read_rows;              // ... those chains, and the read rows
    DeviceArray<uint64_t> d_keys, d_sorted;                // the work: the rank keys before and behind the sort
    DeviceArray<uint32_t> d_par, d_slot;                   // per chain its parent's rank and its place among the reported
    DeviceArray<uint32_t> d_n_out;                         // per read its reported chains
    DeviceArray<uint64_t> d_ctr;                           // kCtrWords words
    DeviceArray<char> d_tmp;                               // rocPRIM's temporary storage: held inside a run only
    bool held = false;                                     // a result is held (n_reads may be 0)
    uint64_t n_reads = 0, n_chains = 0, n_primary = 0, n_secondary = 0, n_reported = 0, most_chains = 0;
    int failed = 0;                                        // the status of a run that failed halfway

    uint64_t device_bytes() const
    {
        return d_rows.bytes() + d_order.bytes() + d_out_offsets.bytes() + d_out.bytes() + d_read_rows.bytes() + d_keys.bytes() + d_sorted.bytes() +
               d_par.bytes() + d_slot.bytes() + d_n_out.bytes() + d_ctr.bytes() + d_tmp.bytes();
    }

    // the result and every work array
    void release_all()
    {
        d_rows.release(); d_order.release(); d_out_offsets.release(); d_out.release(); d_read_rows.release(); d_keys.release(); d_sorted.release();
        d_par.release(); d_slot.release(); d_n_out.release(); d_ctr.release(); d_tmp.release();
    }
};

namespace {

using Handle = ntk_mapping;

// what run_device refuses before any device call: the parameters ...
int check_params(const ntk_mapping_params *p)
{
    if (!p) return NTK_ERR_BAD_ARG;
    if (p->k < 1 || p->k > MP_K_MAX || p->mask_level_pm > MP_PM_MAX || p->pri_ratio_pm > MP_PM_MAX || p->best_n > MP_BEST_N_MAX) return NTK_ERR_BAD_ARG;
    if (p->min_chain_score < 1 || p->reserved[0] || p->reserved[1] || p->reserved[2]) return NTK_ERR_BAD_ARG;
    return NTK_OK;
}

// ... and the arrays
int check_arrays(const Handle *m, const uint64_t *d_c_offsets, const uint32_t *d_chain_rows, const uint64_t *d_m_offsets, const uint32_t *d_members,
                 const uint32_t *d_rpos, const uint32_t *d_qpos, uint64_t n_reads, uint64_t n_chains, uint64_t n_members, uint64_t n_anchors)
{
    if (!m) return NTK_ERR_BAD_ARG;
    if ((n_chains >> 32) || (n_reads >> 32)) return NTK_ERR_BAD_ARG;
    if (!d_c_offsets || ((uintptr_t)d_c_offsets & 7) || !d_m_offsets || ((uintptr_t)d_m_offsets & 7)) return NTK_ERR_BAD_ARG;
    if (n_chains && (!d_chain_rows || ((uintptr_t)d_chain_rows & 3))) return NTK_ERR_BAD_ARG;
    if (n_members && (!d_members || ((uintptr_t)d_members & 3))) return NTK_ERR_BAD_ARG;
    if (n_anchors && (!d_rpos || !d_qpos || ((uintptr_t)d_rpos & 3) || ((uintptr_t)d_qpos & 3))) return NTK_ERR_BAD_ARG;
    return NTK_OK;
}

inline unsigned grid_of(const Handle *m, uint64_t items, unsigned per_block = MP_THREADS)
{
    return grid_for(items, per_block, (unsigned)m->n_cu * MP_BLOCKS_PER_CU);
}

// The verification on the device: NTK_OK with the chains of the reads [a.lo, a.hi), or the refusal.  Nothing held is touched: the span
// kernel runs without writing.
int verify(Handle *m, MapArgs &a)
{
    int rc;
    hipStream_t st = m->stream;
    CT_HIPCHK(hipSetDevice(m->device));
    if ((rc = m->d_ctr.ensure(st, kCtrWords, grow_exact))) return rc;
    a.ctr = m->d_ctr.p;
    CT_HIPCHK(hipMemsetAsync(m->d_ctr.p, 0, kCtrWords * sizeof(uint64_t), st));
    uint64_t items = a.n_reads > a.n_chains ? a.n_reads : a.n_chains;
    items = items + 1 > a.n_members ? items + 1 : a.n_members;
    hipLaunchKernelGGL(mp_verify_kernel, dim3(grid_of(m, items)), dim3(MP_THREADS), 0, st, a);
    CT_HIPCHK(hipGetLastError());
    if ((rc = m->h_stage.read(st, m->d_ctr.p, kCtrWords))) return rc;
    if (m->h_stage.p[kCtrFlags] & MP_BAD_ARG_FLAGS) return NTK_ERR_BAD_ARG;
    if (m->h_stage.p[kCtrFlags] & MP_UNSUPPORTED_FLAGS) return NTK_ERR_UNSUPPORTED;
    a.lo = m->h_stage.p[kCtrLo]; a.hi = m->h_stage.p[kCtrHi];
    if (m->h_stage.p[kCtrFlags] & MP_MAYBE_BLEN) {   // the bound of some chain's blen does not fit: the exact sums
        hipLaunchKernelGGL(mp_span_kernel, dim3(grid_of(m, a.n_chains, kWaves)), dim3(MP_THREADS), 0, st, a, 0u);
        CT_HIPCHK(hipGetLastError());
        if ((rc = m->h_stage.read(st, m->d_ctr.p, 1))) return rc;
        if (m->h_stage.p[kCtrFlags] & MP_LONG_BLEN) return NTK_ERR_UNSUPPORTED;
    }
    return NTK_OK;
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

// the whole run behind the verification; a failure in here marks the handle
int map(Handle *m, MapArgs &a, uint64_t n_reads, uint64_t n_chains)
{
    int rc;
    hipStream_t st = m->stream;
    if ((rc = m->d_rows.ensure(st, 16 * n_chains, grow_exact)) || (rc = m->d_order.ensure(st, n_chains, grow_exact)) ||
        (rc = m->d_keys.ensure(st, n_chains, grow_exact)) || (rc = m->d_sorted.ensure(st, n_chains, grow_exact)) ||
        (rc = m->d_par.ensure(st, n_chains, grow_exact)) || (rc = m->d_slot.ensure(st, n_chains, grow_exact)) ||
        (rc = m->d_out_offsets.ensure(st, n_reads + 1, grow_exact)) || (rc = m->d_read_rows.ensure(st, 4 * n_reads, grow_exact)) ||
        (rc = m->d_n_out.ensure(st, n_reads + 1, grow_exact)))
        return rc;
    a.rows = m->d_rows.p; a.order = m->d_order.p; a.keys = m->d_keys.p; a.sorted = m->d_sorted.p; a.par = m->d_par.p; a.slot = m->d_slot.p;
    a.out_offsets = m->d_out_offsets.p; a.read_rows = m->d_read_rows.p; a.n_out = m->d_n_out.p;
    if (n_chains) {
        hipLaunchKernelGGL(mp_span_kernel, dim3(grid_of(m, n_chains, kWaves)), dim3(MP_THREADS), 0, st, a, 1u);
        CT_HIPCHK(hipGetLastError());
        hipLaunchKernelGGL(mp_keys_kernel, dim3(grid_of(m, n_chains)), dim3(MP_THREADS), 0, st, a);
        CT_HIPCHK(hipGetLastError());
        if (n_reads) {
            rc = with_tmp(m->d_tmp, st, grow_exact, [&](void *tmp, size_t &bytes) {
                return rocprim::segmented_radix_sort_keys(tmp, bytes, m->d_keys.p, m->d_sorted.p, (unsigned)n_chains, (unsigned)n_reads, a.c_offsets,
                                                          a.c_offsets + 1, 0u, 64u, st);
            });
            if (rc) return rc;
        }
    }
    hipLaunchKernelGGL(mp_parent_kernel, dim3(grid_of(m, n_reads, kWaves)), dim3(MP_THREADS), 0, st, a);
    CT_HIPCHK(hipGetLastError());
    rc = with_tmp(m->d_tmp, st, grow_exact, [&](void *tmp, size_t &bytes) {
        return rocprim::exclusive_scan(tmp, bytes, m->d_n_out.p, m->d_out_offsets.p, (uint64_t)0, (size_t)(n_reads + 1), rocprim::plus<uint64_t>(), st);
    });
    if (rc) return rc;
    CT_HIPCHK(hipMemcpyAsync(m->h_stage.p, m->d_out_offsets.p + n_reads, sizeof(uint64_t), hipMemcpyDeviceToHost, st));
    if ((rc = m->h_stage.read(st, m->d_ctr.p + kCtrPrimary, 3, kCtrPrimary))) return rc;
    const uint64_t n_reported = m->h_stage.p[0];
    if ((rc = m->d_out.ensure(st, n_reported, grow_exact))) return rc;
    a.out = m->d_out.p;
    if (a.hi > a.lo) {
        hipLaunchKernelGGL(mp_emit_kernel, dim3(grid_of(m, a.hi - a.lo)), dim3(MP_THREADS), 0, st, a);
        CT_HIPCHK(hipGetLastError());
    }
    CT_HIPCHK(hipStreamSynchronize(st));
    m->n_primary = m->h_stage.p[kCtrPrimary]; m->n_secondary = m->h_stage.p[kCtrSecondary]; m->most_chains = m->h_stage.p[kCtrMost];
    m->n_reported = n_reported;
    return NTK_OK;
}

}  // namespace

extern "C" {

int ntk_mapping_create(ntk_ctx *ctx, ntk_mapping **out)
{
    if (!ctx || !out) return NTK_ERR_BAD_ARG;
    *out = nullptr;
    ntk_mapping *m = new (std::nothrow) ntk_mapping();
    if (!m) return NTK_ERR_NOMEM;
    int rc = m->bind(ctx, 0, 0);
    if (rc) { delete m; return rc; }
    if ((rc = m->h_stage.alloc(kCtrWords))) { delete m; return rc; }
    *out = m;
    return NTK_OK;
}

int ntk_mapping_trim(ntk_mapping *m)
{
    if (!m) return NTK_ERR_BAD_ARG;
    CT_HIPCHK(hipSetDevice(m->device));
    CT_HIPCHK(hipStreamSynchronize(m->stream));
    m->release_all();
    (void)hipGetLastError();
    m->held = false;
    m->n_reads = m->n_chains = m->n_primary = m->n_secondary = m->n_reported = m->most_chains = 0;
    m->failed = 0;
    return NTK_OK;
}

void ntk_mapping_destroy(ntk_mapping *m)
{
    if (!m) return;
    (void)ntk_mapping_trim(m);
    m->h_stage.release();
    (void)hipGetLastError();
    delete m;
}

int ntk_mapping_run_device(ntk_mapping *m, const uint64_t *d_c_offsets, const uint32_t *d_chain_rows, const uint64_t *d_m_offsets,
                           const uint32_t *d_members, const uint32_t *d_rpos, const uint32_t *d_qpos, uint64_t n_reads, uint64_t n_chains,
                           uint64_t n_members, uint64_t n_anchors, const struct ntk_mapping_params *params)
{
    int rc = check_arrays(m, d_c_offsets, d_chain_rows, d_m_offsets, d_members, d_rpos, d_qpos, n_reads, n_chains, n_members, n_anchors);
    if (rc || (rc = check_params(params))) return rc;
    MapArgs a = {};
    a.c_offsets = d_c_offsets; a.chain_rows = d_chain_rows; a.m_offsets = d_m_offsets; a.members = d_members; a.rpos = d_rpos; a.qpos = d_qpos;
    a.n_reads = n_reads; a.n_chains = n_chains; a.n_members = n_members; a.n_anchors = n_anchors;
    a.r.k = params->k; a.r.mask_level_pm = params->mask_level_pm; a.r.pri_ratio_pm = params->pri_ratio_pm; a.r.best_n = params->best_n;
    a.r.min_chain_score = params->min_chain_score;
    if ((rc = verify(m, a))) return rc;
    // the run starts over: nothing of the result held so far is part of the new one
    m->held = true; m->failed = 0;
    m->n_reads = n_reads; m->n_chains = n_chains;
    m->n_primary = m->n_secondary = m->n_reported = m->most_chains = 0;
    rc = map(m, a, n_reads, n_chains);
    drop_tmp(m);
    if (rc) m->failed = rc;
    return rc;
}

int ntk_mapping_read(ntk_mapping *m, uint32_t *rows, uint32_t *order, uint64_t *out_offsets, uint32_t *out, uint32_t *read_rows,
                     uint64_t cap_chains, uint64_t cap_out, uint64_t *n_chains, uint64_t *n_out)
{
    if (!m || !n_chains || !n_out || (cap_chains && (!rows || !order)) || (cap_out && !out)) return NTK_ERR_BAD_ARG;
    if (m->failed) return m->failed;
    *n_chains = m->held ? m->n_chains : 0;
    *n_out = m->held ? m->n_reported : 0;
    if (!m->held) return NTK_OK;
    if (m->n_chains > cap_chains || m->n_reported > cap_out) return NTK_ERR_CAPACITY;
    if (!out_offsets) return NTK_OK;   // the sizes alone
    hipStream_t st = m->stream;
    CT_HIPCHK(hipSetDevice(m->device));
    CT_HIPCHK(hipMemcpyAsync(out_offsets, m->d_out_offsets.p, (m->n_reads + 1) * sizeof(uint64_t), hipMemcpyDeviceToHost, st));
    if (read_rows && m->n_reads) CT_HIPCHK(hipMemcpyAsync(read_rows, m->d_read_rows.p, 4 * m->n_reads * sizeof(uint32_t), hipMemcpyDeviceToHost, st));
    if (m->n_chains) {
        CT_HIPCHK(hipMemcpyAsync(rows, m->d_rows.p, 16 * m->n_chains * sizeof(uint32_t), hipMemcpyDeviceToHost, st));
        CT_HIPCHK(hipMemcpyAsync(order, m->d_order.p, m->n_chains * sizeof(uint32_t), hipMemcpyDeviceToHost, st));
    }
    if (m->n_reported) CT_HIPCHK(hipMemcpyAsync(out, m->d_out.p, m->n_reported * sizeof(uint32_t), hipMemcpyDeviceToHost, st));
    CT_HIPCHK(hipStreamSynchronize(st));
    return NTK_OK;
}

int ntk_mapping_result_device(ntk_mapping *m, const uint32_t **d_rows, const uint32_t **d_order, const uint64_t **d_out_offsets,
                              const uint32_t **d_out, const uint32_t **d_read_rows, uint64_t *n_chains, uint64_t *n_out)
{
    if (!m || !d_rows || !d_order || !d_out_offsets || !d_out || !d_read_rows || !n_chains || !n_out) return NTK_ERR_BAD_ARG;
    if (m->failed) return m->failed;
    const bool held = m->held;
    *d_rows = held && m->n_chains ? m->d_rows.p : nullptr;
    *d_order = held && m->n_chains ? m->d_order.p : nullptr;
    *d_out_offsets = held ? m->d_out_offsets.p : nullptr;
    *d_out = held && m->n_reported ? m->d_out.p : nullptr;
    *d_read_rows = held && m->n_reads ? m->d_read_rows.p : nullptr;
    *n_chains = held ? m->n_chains : 0;
    *n_out = held ? m->n_reported : 0;
    return NTK_OK;
}

int ntk_mapping_stats(ntk_mapping *m, struct ntk_mapping_stats *out)
{
    if (!m || !out) return NTK_ERR_BAD_ARG;
    if (m->failed) return m->failed;
    CT_HIPCHK(hipSetDevice(m->device));
    CT_HIPCHK(hipStreamSynchronize(m->stream));
    out->n_reads = m->n_reads; out->n_chains = m->n_chains; out->n_primary = m->n_primary; out->n_secondary = m->n_secondary;
    out->n_reported = m->n_reported; out->most_chains = m->most_chains; out->reserved = 0;
    out->device_bytes = m->device_bytes();
    return NTK_OK;
}

}  // extern "C"
