// Chaining seed anchors (include_pending/needletail_amd/chain.h): minimap2's chaining recurrence over a fixed predecessor window and its
// backtrack, over a per-read CSR of anchors, into a per-read CSR of chains with their members.  A consumer of the core's public ABI on
// the shared scaffold (ntk_consumer.hpp); it reads anchor arrays alone, never a base, and links nothing but the core.
//
// run_device: verify the arrays (ch_verify_kernel), mark and number the runs (ch_heads_kernel, a rocPRIM scan, ch_runs_kernel), run the
// recurrence with one wave per run (ch_dp_kernel), order every read's anchors by (f descending, index ascending) with one segmented
// radix sort of 64-bit keys (ch_keys_kernel, rocPRIM), and backtrack with one thread per read (ch_walk_kernel): a first pass counts
// chains and members, two scans give the bases, the totals are read back - the result arrays grow there - and a second pass writes
// rows and members.  rocPRIM's temporary storage is held inside a call only.  The rule is ntk_chain_rule.hpp's.
// DESIGN.md section 24.
#include "../../include_pending/needletail_amd/chain.h"
#include "ntk_consumer.hpp"
#include "ntk_chain_rule.hpp"

#include <rocprim/device/device_scan.hpp>
#include <rocprim/device/device_segmented_radix_sort.hpp>

#include <new>

namespace {

// the counter words: what the verification raised, the first and last anchor of a read, the longest run
constexpr int kCtrFlags = 0, kCtrLo = 1, kCtrHi = 2, kCtrLongest = 3, kCtrWords = 4;
constexpr uint32_t kWaves = CH_THREADS / 64;

static_assert(CH_THREADS == kThreads, "the blocks of the scaffold");
static_assert(sizeof(struct ntk_chain_params) == 32 && sizeof(struct ntk_chain_stats) == 64, "the header's struct sizes");

__device__ inline void or_agent(uint64_t *p, uint64_t v) { (void)__hip_atomic_fetch_or(p, v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT); }
__device__ inline void max_agent(uint64_t *p, uint64_t v) { (void)__hip_atomic_fetch_max(p, v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT); }

__device__ inline uint64_t first_item() { return (uint64_t)blockIdx.x * CH_THREADS + threadIdx.x; }
__device__ inline uint64_t item_step() { return (uint64_t)gridDim.x * CH_THREADS; }

__device__ inline uint64_t wave_max(uint64_t v)
{
    for (int off = 32; off > 0; off >>= 1) {
        const uint64_t o = __shfl_xor(v, off, 64);
        v = o > v ? o : v;
    }
    return v;
}

// The arrays as the rule reads them: offsets non-decreasing and offsets[n_reads] <= n, no read of CH_READ_ANCHORS anchors or more, and
// within a read every triple strictly behind the one in front of it.  offsets[0] and offsets[n_reads] are read before they are known to
// be good: they only select the anchors that are looked at, every one of them below n, and the search of an anchor's read stays inside
// the offsets whatever they hold.  ctr is zeroed before.
__global__ __launch_bounds__(CH_THREADS) void ch_verify_kernel(const uint64_t *offsets, uint64_t n_reads, const uint32_t *ref_rev, const uint32_t *rpos,
                                                               const uint32_t *qpos, uint64_t n, uint64_t *ctr)
{
    const uint64_t lo = offsets[0], end = offsets[n_reads], hi = end < n ? end : n, items = n_reads + 1 > n ? n_reads + 1 : n;
    uint32_t bad = 0;
    for (uint64_t i = first_item(); i < items; i += item_step()) {
        if (i < n_reads) {
            const uint64_t b = offsets[i], e = offsets[i + 1];
            if (b > e) bad |= CH_BAD_OFFSETS;
            else if (e - b >= CH_READ_ANCHORS) bad |= CH_LONG_READ;
        }
        if (i == n_reads && offsets[i] > n) bad |= CH_BAD_OFFSETS;
        if (i < n && i > lo && i < hi) {   // (anchor lo is the first of its read)
            const uint64_t c = ch_at_or_before(offsets, n_reads + 1, i);
            if (c && offsets[c - 1] != i && !ch_before(ref_rev[i - 1], rpos[i - 1], qpos[i - 1], ref_rev[i], rpos[i], qpos[i])) bad |= CH_BAD_ORDER;
        }
    }
    if (bad) or_agent(ctr + kCtrFlags, bad);
    if (first_item() == 0) { ctr[kCtrLo] = lo; ctr[kCtrHi] = hi; }
}

struct ChainArgs {
    const uint64_t *offsets;                  // the anchors: n_reads + 1 offsets ...
    const uint32_t *ref_rev, *rpos, *qpos;    // ... and n triples
    uint64_t n_reads, n, lo, hi;              // the anchors of the reads are [lo, hi)
    ch_rule_params r;
    uint32_t min_score, min_cnt;
    uint32_t *head, *rank, *run_start;        // per anchor: it starts a run, and the scan of that; where each of the n_runs + 1 runs starts
    uint64_t n_runs;
    int32_t *f;
    uint32_t *p;
    uint64_t *keys, *order;                   // the visit keys before and behind the sort
    uint8_t *used;
    uint32_t *n_c, *n_m;                      // per read: its chains and their members
    uint64_t *c_offsets, *m_base;             // their scans
    uint32_t *chain_rows, *members, *read_rows;
    uint64_t *m_offsets;
    uint64_t *ctr;
};

// head[i] = anchor i starts a run; an anchor of no read starts none and gets its f and p here
__global__ __launch_bounds__(CH_THREADS) void ch_heads_kernel(ChainArgs a)
{
    for (uint64_t i = first_item(); i < a.n; i += item_step()) {
        if (i < a.lo || i >= a.hi) {
            a.head[i] = 0; a.f[i] = 0; a.p[i] = CH_NONE;
            continue;
        }
        const bool first = a.offsets[ch_at_or_before(a.offsets, a.n_reads + 1, i) - 1] == i;
        a.head[i] = ch_run_head(first, first ? 0 : a.ref_rev[i - 1], first ? 0 : a.rpos[i - 1], a.ref_rev[i], a.rpos[i], a.r.max_dist);
    }
}

// where run number rank - 1 starts; the runs lie back to back in [lo, hi), so the entry behind the last one is hi
__global__ __launch_bounds__(CH_THREADS) void ch_runs_kernel(ChainArgs a)
{
    for (uint64_t i = first_item(); i < a.n; i += item_step()) {
        if (a.head[i]) a.run_start[a.rank[i] - 1] = (uint32_t)i;
        if (i + 1 == a.n) a.run_start[a.n_runs] = (uint32_t)a.hi;
    }
}

// The recurrence, one wave per run.  The wave takes the run's anchors 64 at a time into registers, one per lane, and walks them in order:
// anchor i's coordinates come from their lane, lane l scores predecessor i - 1 - l of every strip of 64 up to h from the wave's ring
// (slot = index mod CH_RING: the at most h <= CH_RING anchors in front of i were written by this wave for this run), and the largest
// candidate word of the wave is the rule's choice.  Lane 0 writes f and p and the anchor's slot of the ring.
__global__ __launch_bounds__(CH_THREADS) void ch_dp_kernel(ChainArgs a)
{
    __shared__ uint32_t s_rpos[kWaves][CH_RING], s_qpos[kWaves][CH_RING];
    __shared__ int32_t s_f[kWaves][CH_RING];
    const uint32_t wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
    volatile uint32_t *ring_r = s_rpos[wave], *ring_q = s_qpos[wave];
    volatile int32_t *ring_f = s_f[wave];
    const uint64_t waves = (uint64_t)gridDim.x * kWaves;
    uint32_t longest = 0;
    for (uint64_t run = (uint64_t)blockIdx.x * kWaves + wave; run < a.n_runs; run += waves) {
        const uint32_t b = a.run_start[run], e = a.run_start[run + 1];
        const uint32_t rev = a.ref_rev[b] & 1;
        longest = e - b > longest ? e - b : longest;
        for (uint32_t c = b; c < e; c += 64) {
            const uint32_t count = e - c < 64 ? e - c : 64;
            uint32_t my_r = 0, my_q = 0;
            if (lane < count) { my_r = a.rpos[c + lane]; my_q = a.qpos[c + lane]; }
            for (uint32_t t = 0; t < count; t++) {
                const uint32_t i = c + t, ri = __shfl(my_r, t, 64), qi = __shfl(my_q, t, 64);
                const uint32_t n_pred = i - b < a.r.h ? i - b : a.r.h;
                uint64_t best = 0;
                for (uint32_t s = 0; s < n_pred; s += 64) {
                    const uint32_t back = s + lane;
                    uint32_t out_of_reach = 0;
                    if (back < n_pred) {
                        const uint32_t j = i - 1 - back, slot = j & (CH_RING - 1);
                        const uint32_t rj = ring_r[slot], qj = ring_q[slot];
                        const uint64_t cand = ch_candidate(rev, rj, qj, ring_f[slot], j, ri, qi, a.r);
                        best = cand > best ? cand : best;
                        out_of_reach = ri - rj > a.r.max_dist;
                    }
                    // the order is by rpos: where the nearest anchor of a strip is out of reach, so is every anchor in front of it
                    if (__builtin_amdgcn_readfirstlane(out_of_reach)) break;
                }
                best = wave_max(best);
                if (lane == 0) {
                    const int32_t fi = ch_f_of(best, a.r.k);
                    const uint32_t slot = i & (CH_RING - 1);
                    a.f[i] = fi; a.p[i] = ch_p_of(best);
                    ring_r[slot] = ri; ring_q[slot] = qi; ring_f[slot] = fi;
                }
                __builtin_amdgcn_wave_barrier();
            }
        }
    }
    if (lane == 0 && longest) max_agent(a.ctr + kCtrLongest, longest);
}

__global__ __launch_bounds__(CH_THREADS) void ch_keys_kernel(ChainArgs a)
{
    for (uint64_t i = first_item(); i < a.n; i += item_step()) a.keys[i] = ch_visit_key(a.f[i], (uint32_t)i);
}

// The backtrack, one thread per read, over the read's anchors in visit order; `used` is zeroed before.  write == 0: the read's chains
// and their members are counted (item n_reads closes the counts for their scans).  write != 0: the same walk writes the chain rows, each
// chain's members back to front - the walk meets them in descending order - and the read's row (item n_reads closes m_offsets).
__global__ __launch_bounds__(CH_THREADS) void ch_walk_kernel(ChainArgs a, uint32_t write)
{
    for (uint64_t q = first_item(); q <= a.n_reads; q += item_step()) {
        if (q == a.n_reads) {
            if (write) a.m_offsets[a.c_offsets[q]] = a.m_base[q]; else a.n_c[q] = a.n_m[q] = 0;
            break;
        }
        const uint64_t b = a.offsets[q], e = a.offsets[q + 1];
        uint64_t c_at = write ? a.c_offsets[q] : 0, m_at = write ? a.m_base[q] : 0;
        uint32_t chains = 0, kept = 0, best = 0;
        for (uint64_t v = b; v < e; v++) {
            const uint32_t i = (uint32_t)a.order[v];
            const int32_t fi = a.f[i];
            if ((uint32_t)fi < a.min_score) break;   // the order is by f: no anchor behind this one starts a chain either
            if (a.used[i]) continue;
            uint32_t cnt = 0, t = i, first = i;
            while (t != CH_NONE && !a.used[t]) {
                a.used[t] = 1; cnt++; first = t;
                t = a.p[t];
            }
            const int64_t score = (int64_t)fi - (t != CH_NONE ? a.f[t] : 0);
            if (score < (int64_t)a.min_score || cnt < a.min_cnt) continue;   // dropped: its anchors stay used
            if (write) {
                uint32_t *row = a.chain_rows + 8 * c_at;
                row[0] = (uint32_t)score; row[1] = cnt; row[2] = a.ref_rev[i];
                row[3] = a.rpos[first]; row[4] = a.qpos[first]; row[5] = a.rpos[i]; row[6] = a.qpos[i]; row[7] = 0;
                a.m_offsets[c_at] = m_at;
                t = i;
                for (uint32_t s = cnt; s-- > 0;) { a.members[m_at + s] = t; t = a.p[t]; }
            }
            c_at++; m_at += cnt; chains++; kept += cnt;
            best = (uint32_t)score > best ? (uint32_t)score : best;
        }
        if (write) {
            a.read_rows[4 * q] = (uint32_t)(e - b); a.read_rows[4 * q + 1] = chains; a.read_rows[4 * q + 2] = kept; a.read_rows[4 * q + 3] = best;
        } else {
            a.n_c[q] = chains; a.n_m[q] = kept;
        }
    }
}

}  // namespace

struct ntk_chain : Consumer {
    Pinned<uint64_t> h_stage;                              // kCtrWords words
    DeviceArray<int32_t> d_f;                              // the result: per anchor f ...
    DeviceArray<uint32_t> d_p;                             // ... and p
    DeviceArray<uint64_t> d_c_offsets;                     // the n_reads + 1 ranges of the reads' chains ...
    DeviceArray<uint32_t> d_read_rows, d_chain_rows;       // ... the read rows and the chain rows
    DeviceArray<uint64_t> d_m_offsets;                     // the n_chains + 1 ranges of the chains' members ...
    DeviceArray<uint32_t> d_members;                       // ... and the members
    DeviceArray<uint32_t> d_head, d_rank, d_run_start;     // the work: run heads, their scan, where each run starts
    DeviceArray<uint64_t> d_keys, d_order;                 // the visit keys before and behind the sort
    DeviceArray<uint8_t> d_used;                           // the marks of the backtrack
    DeviceArray<uint32_t> d_n_c, d_n_m;                    // per read its chains and their members ...
    DeviceArray<uint64_t> d_m_base;                        // ... and the scan of the members
    DeviceArray<uint64_t> d_ctr;                           // kCtrWords words
    DeviceArray<char> d_tmp;                               // rocPRIM's temporary storage: held inside a run only
    bool held = false;                                     // a result is held (n_reads may be 0)
    uint64_t n_reads = 0, n_anchors = 0, n_runs = 0, longest_run = 0, n_chains = 0, n_members = 0;
    int failed = 0;                                        // the status of a run that failed halfway

    uint64_t device_bytes() const
    {
        return d_f.bytes() + d_p.bytes() + d_c_offsets.bytes() + d_read_rows.bytes() + d_chain_rows.bytes() + d_m_offsets.bytes() +
               d_members.bytes() + d_head.bytes() + d_rank.bytes() + d_run_start.bytes() + d_keys.bytes() + d_order.bytes() + d_used.bytes() +
               d_n_c.bytes() + d_n_m.bytes() + d_m_base.bytes() + d_ctr.bytes() + d_tmp.bytes();
    }

    // the result and every work array
    void release_all()
    {
        d_f.release(); d_p.release(); d_c_offsets.release(); d_read_rows.release(); d_chain_rows.release(); d_m_offsets.release();
        d_members.release(); d_head.release(); d_rank.release(); d_run_start.release(); d_keys.release(); d_order.release(); d_used.release();
        d_n_c.release(); d_n_m.release(); d_m_base.release(); d_ctr.release(); d_tmp.release();
    }
};

namespace {

using Handle = ntk_chain;

// what run_device refuses before any device call: the parameters ...
int check_params(const ntk_chain_params *p)
{
    if (!p) return NTK_ERR_BAD_ARG;
    if (p->k < 1 || p->k > CH_K_MAX || p->max_dist < 1 || p->max_dist > CH_MAX_DIST_MAX || p->bw > p->max_dist) return NTK_ERR_BAD_ARG;
    if (p->h < 1 || p->h > CH_H_MAX || p->min_score < 1 || p->min_cnt < 1 || p->reserved[0] || p->reserved[1]) return NTK_ERR_BAD_ARG;
    return NTK_OK;
}

// ... and the arrays
int check_arrays(const Handle *m, const uint64_t *d_a_offsets, const uint32_t *d_ref_rev, const uint32_t *d_rpos, const uint32_t *d_qpos,
                 uint64_t n_reads, uint64_t n)
{
    if (!m) return NTK_ERR_BAD_ARG;
    if ((n >> 32) || (n_reads >> 31)) return NTK_ERR_BAD_ARG;
    if (!d_a_offsets || ((uintptr_t)d_a_offsets & 7)) return NTK_ERR_BAD_ARG;
    if (n && (!d_ref_rev || !d_rpos || !d_qpos || ((uintptr_t)d_ref_rev & 3) || ((uintptr_t)d_rpos & 3) || ((uintptr_t)d_qpos & 3))) return NTK_ERR_BAD_ARG;
    return NTK_OK;
}

inline unsigned grid_of(const Handle *m, uint64_t items, unsigned per_block = CH_THREADS)
{
    return grid_for(items, per_block, (unsigned)m->n_cu * CH_BLOCKS_PER_CU);
}

// The verification on the device: NTK_OK with the anchors of the reads [lo, hi) in the stage, or the refusal.  Nothing held is touched.
int verify(Handle *m, const uint64_t *d_a_offsets, const uint32_t *d_ref_rev, const uint32_t *d_rpos, const uint32_t *d_qpos, uint64_t n_reads,
           uint64_t n, uint64_t &lo, uint64_t &hi)
{
    int rc;
    hipStream_t st = m->stream;
    CT_HIPCHK(hipSetDevice(m->device));
    if ((rc = m->d_ctr.ensure(st, kCtrWords, grow_exact))) return rc;
    CT_HIPCHK(hipMemsetAsync(m->d_ctr.p, 0, kCtrWords * sizeof(uint64_t), st));
    const uint64_t items = n_reads + 1 > n ? n_reads + 1 : n;
    hipLaunchKernelGGL(ch_verify_kernel, dim3(grid_of(m, items)), dim3(CH_THREADS), 0, st, d_a_offsets, n_reads, d_ref_rev, d_rpos, d_qpos, n,
                       m->d_ctr.p);
    CT_HIPCHK(hipGetLastError());
    if ((rc = m->h_stage.read(st, m->d_ctr.p, kCtrWords))) return rc;
    if (m->h_stage.p[kCtrFlags] & (CH_BAD_OFFSETS | CH_BAD_ORDER)) return NTK_ERR_BAD_ARG;
    if (m->h_stage.p[kCtrFlags] & CH_LONG_READ) return NTK_ERR_UNSUPPORTED;
    lo = m->h_stage.p[kCtrLo]; hi = m->h_stage.p[kCtrHi];
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
int chain(Handle *m, ChainArgs &a, uint64_t n_reads, uint64_t n)
{
    int rc;
    hipStream_t st = m->stream;
    if ((rc = m->d_f.ensure(st, n, grow_exact)) || (rc = m->d_p.ensure(st, n, grow_exact)) || (rc = m->d_head.ensure(st, n, grow_exact)) ||
        (rc = m->d_rank.ensure(st, n, grow_exact)) || (rc = m->d_keys.ensure(st, n, grow_exact)) || (rc = m->d_order.ensure(st, n, grow_exact)) ||
        (rc = m->d_used.ensure(st, n, grow_exact)) || (rc = m->d_c_offsets.ensure(st, n_reads + 1, grow_exact)) ||
        (rc = m->d_read_rows.ensure(st, 4 * n_reads, grow_exact)) || (rc = m->d_n_c.ensure(st, n_reads + 1, grow_exact)) ||
        (rc = m->d_n_m.ensure(st, n_reads + 1, grow_exact)) || (rc = m->d_m_base.ensure(st, n_reads + 1, grow_exact)))
        return rc;
    a.head = m->d_head.p; a.rank = m->d_rank.p; a.f = m->d_f.p; a.p = m->d_p.p; a.keys = m->d_keys.p; a.order = m->d_order.p;
    a.used = m->d_used.p; a.n_c = m->d_n_c.p; a.n_m = m->d_n_m.p; a.c_offsets = m->d_c_offsets.p; a.m_base = m->d_m_base.p;
    a.read_rows = m->d_read_rows.p; a.ctr = m->d_ctr.p;
    uint64_t n_runs = 0;
    if (n) {
        hipLaunchKernelGGL(ch_heads_kernel, dim3(grid_of(m, n)), dim3(CH_THREADS), 0, st, a);
        CT_HIPCHK(hipGetLastError());
        rc = with_tmp(m->d_tmp, st, grow_exact, [&](void *tmp, size_t &bytes) {
            return rocprim::inclusive_scan(tmp, bytes, m->d_head.p, m->d_rank.p, (size_t)n, rocprim::plus<uint32_t>(), st);
        });
        if (rc) return rc;
        CT_HIPCHK(hipMemcpyAsync(m->h_stage.p, m->d_rank.p + (n - 1), sizeof(uint32_t), hipMemcpyDeviceToHost, st));
        CT_HIPCHK(hipStreamSynchronize(st));
        n_runs = *(const uint32_t *)m->h_stage.p;
    }
    if ((rc = m->d_run_start.ensure(st, n_runs + 1, grow_exact))) return rc;
    a.run_start = m->d_run_start.p; a.n_runs = n_runs;
    m->n_runs = n_runs;
    if (n) {
        hipLaunchKernelGGL(ch_runs_kernel, dim3(grid_of(m, n)), dim3(CH_THREADS), 0, st, a);
        CT_HIPCHK(hipGetLastError());
        if (n_runs) {
            hipLaunchKernelGGL(ch_dp_kernel, dim3(grid_of(m, n_runs, kWaves)), dim3(CH_THREADS), 0, st, a);
            CT_HIPCHK(hipGetLastError());
        }
        hipLaunchKernelGGL(ch_keys_kernel, dim3(grid_of(m, n)), dim3(CH_THREADS), 0, st, a);
        CT_HIPCHK(hipGetLastError());
        if (n_reads) {
            rc = with_tmp(m->d_tmp, st, grow_exact, [&](void *tmp, size_t &bytes) {
                return rocprim::segmented_radix_sort_keys(tmp, bytes, m->d_keys.p, m->d_order.p, (unsigned)n, (unsigned)n_reads, a.offsets,
                                                          a.offsets + 1, 0u, 64u, st);
            });
            if (rc) return rc;
        }
        CT_HIPCHK(hipMemsetAsync(m->d_used.p, 0, n, st));
    }
    hipLaunchKernelGGL(ch_walk_kernel, dim3(grid_of(m, n_reads + 1)), dim3(CH_THREADS), 0, st, a, 0u);
    CT_HIPCHK(hipGetLastError());
    rc = with_tmp(m->d_tmp, st, grow_exact, [&](void *tmp, size_t &bytes) {
        return rocprim::exclusive_scan(tmp, bytes, m->d_n_c.p, m->d_c_offsets.p, (uint64_t)0, (size_t)(n_reads + 1), rocprim::plus<uint64_t>(), st);
    });
    if (rc) return rc;
    rc = with_tmp(m->d_tmp, st, grow_exact, [&](void *tmp, size_t &bytes) {
        return rocprim::exclusive_scan(tmp, bytes, m->d_n_m.p, m->d_m_base.p, (uint64_t)0, (size_t)(n_reads + 1), rocprim::plus<uint64_t>(), st);
    });
    if (rc) return rc;
    CT_HIPCHK(hipMemcpyAsync(m->h_stage.p, m->d_c_offsets.p + n_reads, sizeof(uint64_t), hipMemcpyDeviceToHost, st));
    CT_HIPCHK(hipMemcpyAsync(m->h_stage.p + 1, m->d_m_base.p + n_reads, sizeof(uint64_t), hipMemcpyDeviceToHost, st));
    if ((rc = m->h_stage.read(st, m->d_ctr.p + kCtrLongest, 1, kCtrLongest))) return rc;
    const uint64_t n_chains = m->h_stage.p[0], n_members = m->h_stage.p[1];
    m->longest_run = m->h_stage.p[kCtrLongest];
    if ((rc = m->d_chain_rows.ensure(st, 8 * n_chains, grow_exact)) || (rc = m->d_m_offsets.ensure(st, n_chains + 1, grow_exact)) ||
        (rc = m->d_members.ensure(st, n_members, grow_exact)))
        return rc;
    a.chain_rows = m->d_chain_rows.p; a.m_offsets = m->d_m_offsets.p; a.members = m->d_members.p;
    if (n) CT_HIPCHK(hipMemsetAsync(m->d_used.p, 0, n, st));
    hipLaunchKernelGGL(ch_walk_kernel, dim3(grid_of(m, n_reads + 1)), dim3(CH_THREADS), 0, st, a, 1u);
    CT_HIPCHK(hipGetLastError());
    CT_HIPCHK(hipStreamSynchronize(st));
    m->n_chains = n_chains; m->n_members = n_members;
    return NTK_OK;
}

}  // namespace

extern "C" {

int ntk_chain_create(ntk_ctx *ctx, ntk_chain **out)
{
    if (!ctx || !out) return NTK_ERR_BAD_ARG;
    *out = nullptr;
    ntk_chain *m = new (std::nothrow) ntk_chain();
    if (!m) return NTK_ERR_NOMEM;
    int rc = m->bind(ctx, 0, 0);
    if (rc) { delete m; return rc; }
    if ((rc = m->h_stage.alloc(kCtrWords))) { delete m; return rc; }
    *out = m;
    return NTK_OK;
}

int ntk_chain_trim(ntk_chain *m)
{
    if (!m) return NTK_ERR_BAD_ARG;
    CT_HIPCHK(hipSetDevice(m->device));
    CT_HIPCHK(hipStreamSynchronize(m->stream));
    m->release_all();
    (void)hipGetLastError();
    m->held = false;
    m->n_reads = m->n_anchors = m->n_runs = m->longest_run = m->n_chains = m->n_members = 0;
    m->failed = 0;
    return NTK_OK;
}

void ntk_chain_destroy(ntk_chain *m)
{
    if (!m) return;
    (void)ntk_chain_trim(m);
    m->h_stage.release();
    (void)hipGetLastError();
    delete m;
}

int ntk_chain_run_device(ntk_chain *m, const uint64_t *d_a_offsets, const uint32_t *d_ref_rev, const uint32_t *d_rpos, const uint32_t *d_qpos,
                         uint64_t n_reads, uint64_t n_anchors, const struct ntk_chain_params *params)
{
    int rc = check_arrays(m, d_a_offsets, d_ref_rev, d_rpos, d_qpos, n_reads, n_anchors);
    if (rc || (rc = check_params(params))) return rc;
    uint64_t lo = 0, hi = 0;
    if ((rc = verify(m, d_a_offsets, d_ref_rev, d_rpos, d_qpos, n_reads, n_anchors, lo, hi))) return rc;
    // the run starts over: nothing of the result held so far is part of the new one
    m->held = true; m->failed = 0;
    m->n_reads = n_reads; m->n_anchors = n_anchors;
    m->n_runs = m->longest_run = m->n_chains = m->n_members = 0;
    ChainArgs a = {};
    a.offsets = d_a_offsets; a.ref_rev = d_ref_rev; a.rpos = d_rpos; a.qpos = d_qpos;
    a.n_reads = n_reads; a.n = n_anchors; a.lo = lo; a.hi = hi;
    a.r.k = params->k; a.r.max_dist = params->max_dist; a.r.bw = params->bw; a.r.h = params->h;
    a.min_score = params->min_score; a.min_cnt = params->min_cnt;
    rc = chain(m, a, n_reads, n_anchors);
    drop_tmp(m);
    if (rc) m->failed = rc;
    return rc;
}

int ntk_chain_read(ntk_chain *m, uint64_t *c_offsets, uint32_t *chain_rows, uint64_t *m_offsets, uint32_t *members, int32_t *f, uint32_t *p,
                   uint32_t *read_rows, uint64_t cap_chains, uint64_t cap_members, uint64_t *n_chains, uint64_t *n_members)
{
    if (!m || !n_chains || !n_members || (cap_chains && (!chain_rows || !m_offsets)) || (cap_members && !members)) return NTK_ERR_BAD_ARG;
    if (m->failed) return m->failed;
    *n_chains = m->held ? m->n_chains : 0;
    *n_members = m->held ? m->n_members : 0;
    if (!m->held) return NTK_OK;
    if (m->n_chains > cap_chains || m->n_members > cap_members) return NTK_ERR_CAPACITY;
    if (!c_offsets) return NTK_OK;   // the sizes alone
    hipStream_t st = m->stream;
    CT_HIPCHK(hipSetDevice(m->device));
    CT_HIPCHK(hipMemcpyAsync(c_offsets, m->d_c_offsets.p, (m->n_reads + 1) * sizeof(uint64_t), hipMemcpyDeviceToHost, st));
    if (read_rows && m->n_reads) CT_HIPCHK(hipMemcpyAsync(read_rows, m->d_read_rows.p, 4 * m->n_reads * sizeof(uint32_t), hipMemcpyDeviceToHost, st));
    if (m_offsets) CT_HIPCHK(hipMemcpyAsync(m_offsets, m->d_m_offsets.p, (m->n_chains + 1) * sizeof(uint64_t), hipMemcpyDeviceToHost, st));
    if (m->n_chains) CT_HIPCHK(hipMemcpyAsync(chain_rows, m->d_chain_rows.p, 8 * m->n_chains * sizeof(uint32_t), hipMemcpyDeviceToHost, st));
    if (m->n_members) CT_HIPCHK(hipMemcpyAsync(members, m->d_members.p, m->n_members * sizeof(uint32_t), hipMemcpyDeviceToHost, st));
    if (f && m->n_anchors) CT_HIPCHK(hipMemcpyAsync(f, m->d_f.p, m->n_anchors * sizeof(int32_t), hipMemcpyDeviceToHost, st));
    if (p && m->n_anchors) CT_HIPCHK(hipMemcpyAsync(p, m->d_p.p, m->n_anchors * sizeof(uint32_t), hipMemcpyDeviceToHost, st));
    CT_HIPCHK(hipStreamSynchronize(st));
    return NTK_OK;
}

int ntk_chain_result_device(ntk_chain *m, const uint64_t **d_c_offsets, const uint32_t **d_chain_rows, const uint64_t **d_m_offsets,
                            const uint32_t **d_members, const int32_t **d_f, const uint32_t **d_p, const uint32_t **d_read_rows,
                            uint64_t *n_chains, uint64_t *n_members)
{
    if (!m || !d_c_offsets || !d_chain_rows || !d_m_offsets || !d_members || !d_f || !d_p || !d_read_rows || !n_chains || !n_members)
        return NTK_ERR_BAD_ARG;
    if (m->failed) return m->failed;
    const bool held = m->held;
    *d_c_offsets = held ? m->d_c_offsets.p : nullptr;
    *d_m_offsets = held ? m->d_m_offsets.p : nullptr;
    *d_chain_rows = held && m->n_chains ? m->d_chain_rows.p : nullptr;
    *d_members = held && m->n_members ? m->d_members.p : nullptr;
    *d_f = held && m->n_anchors ? m->d_f.p : nullptr;
    *d_p = held && m->n_anchors ? m->d_p.p : nullptr;
    *d_read_rows = held && m->n_reads ? m->d_read_rows.p : nullptr;
    *n_chains = held ? m->n_chains : 0;
    *n_members = held ? m->n_members : 0;
    return NTK_OK;
}

int ntk_chain_stats(ntk_chain *m, struct ntk_chain_stats *out)
{
    if (!m || !out) return NTK_ERR_BAD_ARG;
    if (m->failed) return m->failed;
    CT_HIPCHK(hipSetDevice(m->device));
    CT_HIPCHK(hipStreamSynchronize(m->stream));
    out->n_reads = m->n_reads; out->n_anchors = m->n_anchors; out->n_runs = m->n_runs; out->longest_run = m->longest_run;
    out->n_chains = m->n_chains; out->n_members = m->n_members; out->reserved = 0;
    out->device_bytes = m->device_bytes();
    return NTK_OK;
}

}  // extern "C"
