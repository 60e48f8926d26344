// MinHash sketches of device batches (include/needletail_amd_minhash.h): bottom-s and scaled, with abundance.  A consumer of the
// core's public ABI like the cardinality sketch (ntk_sketch.hip), with its two routes: k <= 32 reads the values
// ntk_materialize_device_quality emits, k = 33..63 walks the batch bytes (ntk_wide_walk.hpp).
//
// THE ONE PLACE that fixes the hash is minhash_hash below (fmix64 is ntk_consumer.hpp's, the tables' hash): the sketch library's
// hash, restated; the header states it and tests/_minhash_model.py takes it from tests/_sketch_model.py.
//
// State: S, the kept (hash, count) pairs, sorted and unique; the threshold tau, the largest hash that can still enter (it only falls);
// a candidate buffer of `cap` hashes with a reservation counter on the device.  The filter kernels append every hash <= tau; a merge
// sorts the buffer, run-length encodes it, merges it with S adding the counts of equal hashes, cuts the result by the handle's rule and
// lowers tau.  A launch is only ever taken whole (run_range below): the counter keeps counting past the capacity, the host reads it
// after every launch, and a launch that did not fit is discarded and redone in sub-ranges that cannot overflow.  Hence every hash
// <= the final tau has every one of its occurrences in S or the buffer.  Adds on the one counter serialise (about 12 ns each), so an
// optimistic launch reserves per wave and kSlab slots at a time and pads what a wave leaves unused.  DESIGN.md section 15.
#include "../../include/needletail_amd_minhash.h"
#include "ntk_consumer.hpp"
#include "ntk_wide_walk.hpp"

#include <rocprim/device/device_merge.hpp>
#include <rocprim/device/device_radix_sort.hpp>
#include <rocprim/device/device_reduce_by_key.hpp>
#include <rocprim/device/device_run_length_encode.hpp>

#include <new>
#include <vector>

namespace {

constexpr uint64_t kXor = 0x9E3779B97F4A7C15ull;         // C: key 0 (AAA...A) must not hash to 0
constexpr int kFilterThreads = 256;                      // 64 B of LDS, few registers: eight blocks per CU keep 8 waves per SIMD
constexpr unsigned kBlocksPerCu = 8;
constexpr uint32_t kPerLane = 4;                         // window ends per lane and round of mh_filter_kernel (loads in flight)
constexpr uint64_t kAll = ~(uint64_t)0;
constexpr uint64_t kFirstEnds = 4096;                    // bottom-s: window ends of the first launch (or 16 s, if that is more)
constexpr uint64_t kLadder = 8;                          // bottom-s: a launch is at most this many times the window ends seen before
constexpr uint64_t kLadderFloor = (uint64_t)1 << 16;     // bottom-s: ... or this many window ends
constexpr uint64_t kEagerFill = 4096;                    // bottom-s: the buffer is merged once it holds this many hashes (or 4 s)
constexpr int kCtrFill = 0, kCtrWindows = 1, kCtrHoles = 2; // the device counters: slots reserved in the buffer, windows seen, padding
constexpr uint32_t kSlab = 16;                           // slots a wave reserves at a time in an optimistic launch

static_assert(kXor == NTK_MINHASH_XOR, "the header states the hash constant");
static_assert(NTK_MINHASH_BUFFER_MIN >= kLaneRun, "a redo sub-range of the wide kernel is at least one lane run");

__host__ __device__ inline uint64_t minhash_hash(uint64_t key) { return fmix64(key ^ kXor); }
__host__ __device__ inline uint64_t minhash_hash(uint64_t hi, uint64_t lo) { return fmix64(lo ^ fmix64(hi) ^ kXor); }

struct Candidates {
    uint64_t *buf;      // the candidate buffer
    uint64_t cap;       // its size in hashes
    uint64_t *ctr;      // ctr[kCtrFill]: slots reserved so far (counts on past cap), ctr[kCtrWindows]: windows seen, ctr[kCtrHoles]:
                        // reserved slots that were padded
    uint64_t tau;       // hashes <= tau are appended
    uint32_t slabs;     // 0: every reservation is exactly the passing lanes (a launch of n window ends takes at most n slots);
                        // 1: a wave reserves kSlab slots at a time and pads what it leaves unused (far fewer adds on the one counter)
};

// a wave's slab: the next free slot and the slab's end, in LDS so that lanes that append from divergent code agree on it
struct Slab {
    uint64_t next, end;
};

// The lanes of the wave that call this together (all of them pass) reserve their slots with one agent-scope add, by the first of them,
// and store their hashes at base + rank: a coalesced store, and only below the capacity.
__device__ __forceinline__ void append_exact(const Candidates &c, uint64_t h)
{
    const uint64_t mask = __ballot(1);
    const uint32_t lane = threadIdx.x & 63;
    const uint32_t rank = (uint32_t)__popcll(mask & (((uint64_t)1 << lane) - 1));
    const int leader = __ffsll((unsigned long long)mask) - 1;
    uint64_t base = 0;
    if ((int)lane == leader)
        base = __hip_atomic_fetch_add(c.ctr + kCtrFill, (uint64_t)__popcll(mask), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    base = __shfl(base, leader, 64);
    const uint64_t at = base + rank;
    if (at < c.cap) c.buf[at] = h;
}

// The same through the wave's slab: the add happens only when the slab cannot take the passing lanes; what is left of the old slab
// is padded with ~0 and counted in `holes` (the leader's), so that the host can drop exactly that many entries from the end of the
// sorted buffer.  Every store is below the capacity.
__device__ __forceinline__ void append_slab(const Candidates &c, volatile Slab *slab, uint64_t h, uint64_t &holes)
{
    const uint64_t mask = __ballot(1);
    const uint32_t lane = threadIdx.x & 63, n = (uint32_t)__popcll(mask);
    const uint32_t rank = (uint32_t)__popcll(mask & (((uint64_t)1 << lane) - 1));
    const int leader = __ffsll((unsigned long long)mask) - 1;
    uint64_t next = slab->next, end = slab->end;   // the same for every lane of the wave
    if (next + n > end) {
        for (uint64_t at = next + rank; at < end; at += n)
            if (at < c.cap) c.buf[at] = kAll;
        const uint64_t want = n > kSlab ? n : kSlab;
        uint64_t base = 0;
        if ((int)lane == leader) {
            holes += end - next;
            base = __hip_atomic_fetch_add(c.ctr + kCtrFill, want, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        }
        next = __shfl(base, leader, 64);
        end = next + want;
    }
    if (next + rank < c.cap) c.buf[next + rank] = h;
    if ((int)lane == leader) { slab->next = next + n; slab->end = end; }
    __builtin_amdgcn_wave_barrier();
}

__device__ __forceinline__ void append_passing(const Candidates &c, volatile Slab *slab, uint64_t h, uint64_t &holes)
{
    if (c.slabs) append_slab(c, slab, h, holes);
    else append_exact(c, h);
}

// the block's slabs start empty
__device__ inline volatile Slab *open_slab(Slab *slabs)
{
    if ((threadIdx.x & 63) == 0) slabs[threadIdx.x >> 6] = Slab{0, 0};
    __builtin_amdgcn_wave_barrier();
    return slabs + (threadIdx.x >> 6);
}

// the rest of the wave's last slab is padding; the wave's padding count: one add per wave
__device__ inline void close_slab(const Candidates &c, volatile Slab *slab, uint64_t holes)
{
    const uint64_t next = slab->next, end = slab->end;
    for (uint64_t at = next + (threadIdx.x & 63); at < end; at += 64)
        if (at < c.cap) c.buf[at] = kAll;
    if ((threadIdx.x & 63) == 0) holes += end - next;
    holes = wave_sum(holes);
    if ((threadIdx.x & 63) == 0 && holes) add_agent(c.ctr + kCtrHoles, holes);
}

// the wave's windows: one add per wave
__device__ inline void add_windows(const Candidates &c, uint64_t windows)
{
    windows = wave_sum(windows);
    if ((threadIdx.x & 63) == 0 && windows) add_agent(c.ctr + kCtrWindows, windows);
}

struct FilterArgs {
    const uint64_t *values;    // materialised values, indexed by window end
    const uint16_t *valid16;   // bit (15 - e % 16) of word e / 16: window e is emitted
    uint64_t first, n;         // windows ending in [first, n) are taken
    Candidates c;
};

// k <= 32.  sk_update_kernel's shape: grid-stride over window ends, kPerLane ends per lane and round (each a coalesced 8-byte load
// across the wave, issued before any is used) with the valid plane's bit.  Every lane runs the same number of rounds.  In steady state
// almost no window passes, and the kernel is the stream of the values, a hash and a compare.
__global__ __launch_bounds__(kFilterThreads) void mh_filter_kernel(FilterArgs a)
{
    __shared__ Slab slabs[kFilterThreads / 64];
    volatile Slab *slab = open_slab(slabs);
    uint64_t windows = 0, holes = 0;
    const uint64_t step = (uint64_t)gridDim.x * kFilterThreads, span = a.n - a.first;
    const uint64_t rounds = (span + step * kPerLane - 1) / (step * kPerLane);
    uint64_t i = (uint64_t)blockIdx.x * kFilterThreads + threadIdx.x;
    for (uint64_t r = 0; r < rounds; r++, i += step * kPerLane) {
        uint64_t key[kPerLane];
        bool take[kPerLane];
#pragma unroll
        for (uint32_t u = 0; u < kPerLane; u++) {
            const uint64_t at = i + u * step, e = a.first + at;
            take[u] = at < span;
            key[u] = take[u] ? a.values[e] : 0;
            take[u] = take[u] && ((a.valid16[e >> 4] >> (15 - (e & 15))) & 1u);
        }
#pragma unroll
        for (uint32_t u = 0; u < kPerLane; u++) {
            const uint64_t h = minhash_hash(key[u]);
            windows += take[u] ? 1 : 0;
            if (take[u] && h <= a.c.tau) append_passing(a.c, slab, h, holes);   // inclusive: a repeat of the s-th hash still counts
        }
    }
    close_slab(a.c, slab, holes);
    add_windows(a.c, windows);
}

struct WideFilterArgs {
    const uint8_t *seq, *qual;   // qual: nullptr = no mask
    uint64_t n_bytes;            // no byte at or past it is a base
    uint64_t run_lo, run_hi;     // the lane runs [run_lo, run_hi) are taken: window ends [run_lo * kLaneRun, run_hi * kLaneRun)
    uint32_t k, cutoff;
    Candidates c;
};

// k = 33..63.  Lane r (grid-stride) owns the window ends [r * kLaneRun, (r + 1) * kLaneRun) and walks them as wt_count_kernel does
// (walk_lane_run); 64-bit offsets, no chunking, no scratch.  The lanes of a wave walk in step, so those that pass at the same byte
// share one reservation.
__global__ __launch_bounds__(kFilterThreads) void mh_wide_filter_kernel(WideFilterArgs a)
{
    __shared__ Slab slabs[kFilterThreads / 64];
    volatile Slab *slab = open_slab(slabs);
    uint64_t windows = 0, holes = 0;
    const uint64_t stride = (uint64_t)gridDim.x * kFilterThreads;
    for (uint64_t r = a.run_lo + (uint64_t)blockIdx.x * kFilterThreads + threadIdx.x; r < a.run_hi; r += stride)
        walk_lane_run<kLaneRun, kPrime>(a.seq, a.qual, a.n_bytes, a.k, a.cutoff, r * kLaneRun, [&](uint64_t hi, uint64_t lo) __attribute__((always_inline)) {
            const uint64_t h = minhash_hash(hi, lo);
            windows++;
            if (h <= a.c.tau) append_passing(a.c, slab, h, holes);
        });
    close_slab(a.c, slab, holes);
    add_windows(a.c, windows);
}

// hashes and counts on the device, grown on demand (contents are not kept)
struct HashCounts {
    DeviceArray<uint64_t> k, c;

    void release() { k.release(); c.release(); }

    int ensure(hipStream_t stream, uint64_t n)
    {
        const int rc = k.ensure(stream, n, grow_half_again);
        return rc ? rc : c.ensure(stream, n, grow_half_again);
    }
};

}  // namespace

struct ntk_minhash : Consumer {
    uint64_t num = 0, scaled = 0, max_hash = kAll;
    uint64_t cap = 0;                 // buffer_entries
    DeviceArray<uint64_t> d_buf;      // the candidate buffer
    DeviceArray<uint64_t> d_sorted;   // its sorted copy
    DeviceArray<uint64_t> d_ctr;      // the three counters, then one word for the lengths rocPRIM reports
    Pinned<uint64_t> h_stage;         // 4 words: the counters' three, then the word of a length or a threshold
    DeviceArray<char> d_tmp;          // rocPRIM's temporary storage
    HashCounts kept, runs, merged, next;   // S; the buffer's runs (or a foreign sketch); S and the runs merged; the next S
    uint64_t n_kept = 0, tau = kAll;
    uint64_t fill = 0;                // buffer slots in use (the device counter's value between launches)
    uint64_t holes = 0;               // of which padding (likewise)
    uint64_t windows = 0;             // windows of the launches taken (the device counter's value between launches) and of the merges
    uint64_t ends_seen = 0;           // window ends launched since reset (the ladder of run_range)
    uint64_t n_merges = 0, n_redone = 0;
    int failed = 0;                   // the status of a call that failed halfway; every call but reset and destroy answers it again
    MaterialiseScratch scratch;       // k <= 32 only
};

namespace {

// the device counters on the host (synchronises)
struct Counters {
    uint64_t fill, windows, holes;
};

int read_counters(ntk_minhash *m, Counters *c)
{
    const int rc = m->h_stage.read(m->stream, m->d_ctr.p, 3);
    if (rc) return rc;
    c->fill = m->h_stage.p[kCtrFill]; c->windows = m->h_stage.p[kCtrWindows]; c->holes = m->h_stage.p[kCtrHoles];
    return NTK_OK;
}

// a launch that fitted is taken: the host's view follows the device's
void take_counters(ntk_minhash *m, const Counters &c)
{
    m->fill = c.fill; m->windows = c.windows; m->holes = c.holes;
}

// the device counters := the host's view of them (synchronises: the stage is free again).
// THE INVARIANT every caller keeps: between launches the device's three counters equal m->fill, m->windows and m->holes.  A launch that
// fitted is followed by take_counters; a launch that did not leaves the device's reserved count above `cap` and its windows and padding
// counted in, and only this write-back (flush ends in it) undoes that - so nothing may be launched, and nothing answered, between a
// failed launch and the flush that follows it in run_range.  A call that fails in between leaves the two views apart: the handle is
// marked (ntk_minhash::failed) and refuses everything but reset, which zeroes both.
int write_counters(ntk_minhash *m)
{
    m->h_stage.p[kCtrFill] = m->fill; m->h_stage.p[kCtrWindows] = m->windows; m->h_stage.p[kCtrHoles] = m->holes;
    return m->h_stage.write(m->stream, m->d_ctr.p, 3);
}

// S := S combined with the n sorted unique pairs of m->runs (counts of equal hashes add), cut by the handle's rule; tau follows
int combine(ntk_minhash *m, uint64_t n)
{
    if (n == 0) return NTK_OK;
    uint64_t *d_len = m->d_ctr.p + 3;
    HashCounts *result = &m->runs;
    uint64_t n_result = n;
    if (m->n_kept) {
        const uint64_t total = m->n_kept + n;
        int rc = m->merged.ensure(m->stream, total);
        if (!rc) rc = m->next.ensure(m->stream, total);
        if (rc) return rc;
        rc = with_tmp(m->d_tmp, m->stream, grow_exact, [&](void *tmp, size_t &bytes) {
            return rocprim::merge(tmp, bytes, m->kept.k.p, m->runs.k.p, m->merged.k.p, m->kept.c.p, m->runs.c.p, m->merged.c.p,
                                  (size_t)m->n_kept, (size_t)n, rocprim::less<uint64_t>(), m->stream);
        });
        if (rc) return rc;
        rc = with_tmp(m->d_tmp, m->stream, grow_exact, [&](void *tmp, size_t &bytes) {
            return rocprim::reduce_by_key(tmp, bytes, m->merged.k.p, m->merged.c.p, (size_t)total, m->next.k.p, m->next.c.p, d_len,
                                          rocprim::plus<uint64_t>(), rocprim::equal_to<uint64_t>(), m->stream);
        });
        if (rc) return rc;
        if ((rc = m->h_stage.read(m->stream, d_len, 1, 3))) return rc;
        n_result = m->h_stage.p[3];
        result = &m->next;
    }
    // the cut: the num smallest; with `scaled` nothing above max_hash ever got here
    if (m->num && n_result > m->num) n_result = m->num;
    const HashCounts old = m->kept;
    m->kept = *result;
    *result = old;
    m->n_kept = n_result;
    if (m->num && n_result == m->num) {
        const int rc = m->h_stage.read(m->stream, m->kept.k.p + (n_result - 1), 1, 3);
        if (rc) return rc;
        m->tau = m->h_stage.p[3];   // only ever falls: the num-th smallest of a growing multiset
    }
    m->n_merges++;
    return NTK_OK;
}

// the buffer into S; the device counters are the host's again (fill 0) afterwards.  Whatever a discarded launch wrote at or past
// m->fill is not looked at.  The padding of the slabs is ~0, so after the sort it is the last m->holes entries (a real hash ~0 sorts
// among them and is as good as any of them).
int flush(ntk_minhash *m)
{
    CT_HIPCHK(hipSetDevice(m->device));
    if (m->fill > m->holes) {
        const uint64_t n = m->fill - m->holes;
        int rc = with_tmp(m->d_tmp, m->stream, grow_exact, [&](void *tmp, size_t &bytes) {
            return rocprim::radix_sort_keys(tmp, bytes, m->d_buf.p, m->d_sorted.p, (size_t)m->fill, 0u, 64u, m->stream);
        });
        if (rc) return rc;
        if ((rc = m->runs.ensure(m->stream, n))) return rc;
        uint64_t *d_len = m->d_ctr.p + 3;
        rc = with_tmp(m->d_tmp, m->stream, grow_exact, [&](void *tmp, size_t &bytes) {
            return rocprim::run_length_encode(tmp, bytes, m->d_sorted.p, (unsigned int)n, m->runs.k.p, m->runs.c.p, d_len, m->stream);
        });
        if (rc) return rc;
        if ((rc = m->h_stage.read(m->stream, d_len, 1, 3))) return rc;
        if ((rc = combine(m, m->h_stage.p[3]))) return rc;
    }
    m->fill = m->holes = 0;
    return write_counters(m);
}

// The redo rule.  `launch(lo, hi)` queues the filter kernel over the units [lo, hi) of `ends` window ends each (1: k <= 32; kLaneRun:
// the wide kernel's lane runs).  Every launch is followed by a read of the counters and is taken whole or not at all.
//
// A bottom-s sketch's threshold is what a sample of the input says, and every passing window costs an add on one counter, so it climbs
// a ladder: while fewer than s hashes are held everything passes, and the launches start small (kFirstEnds) and grow by kLadder, each
// one fitting the room left and merged at once; afterwards a launch is at most kLadder times the window ends seen since reset
// (or kLadderFloor, below which a launch costs less than a merge whatever passes), and the buffer is merged as soon as it holds
// kEagerFill hashes, which lowers the threshold for the next launch.  A scaled sketch's threshold is fixed: one launch.
template <class Launch>
int run_range(ntk_minhash *m, uint64_t lo, uint64_t hi, uint64_t ends, Launch launch)
{
    int rc;
    Counters c;
    // a launch of at most the room left cannot overflow: exact reservations, no slabs
    auto fitting = [&](uint64_t take) -> int {
        launch(lo, lo + take, 0u);
        CT_HIPCHK(hipGetLastError());
        if ((rc = read_counters(m, &c))) return rc;
        if (c.fill > m->cap) return NTK_ERR_HIP;   // cannot happen
        take_counters(m, c);
        m->ends_seen += take * ends;
        lo += take;
        return NTK_OK;
    };
    const uint64_t eager = 4 * m->num > kEagerFill ? 4 * m->num : kEagerFill;
    // bottom-s with fewer than s hashes held: everything passes
    for (uint64_t step = (16 * m->num > kFirstEnds ? 16 * m->num : kFirstEnds) / ends; lo < hi && m->num && m->tau == kAll; step *= kLadder) {
        if (m->cap - m->fill < ends && (rc = flush(m))) return rc;
        uint64_t take = (m->cap - m->fill) / ends;
        if (step && step < take) take = step;
        if (hi - lo < take) take = hi - lo;
        if ((rc = fitting(take)) || (rc = flush(m))) return rc;
    }
    while (lo < hi) {
        // the optimistic launch: over all that is left, or the ladder's next step
        uint64_t take = hi - lo;
        if (m->num) {
            const uint64_t seen = kLadder * m->ends_seen > kLadderFloor ? kLadder * m->ends_seen : kLadderFloor;
            if (seen / ends < take) take = seen / ends;
        }
        // a launch that does not fit costs a pass over its range: start it with at least half the buffer free
        if (m->fill > m->cap / 2 && (rc = flush(m))) return rc;
        launch(lo, lo + take, 1u);
        CT_HIPCHK(hipGetLastError());
        if ((rc = read_counters(m, &c))) return rc;
        if (c.fill <= m->cap) {
            take_counters(m, c);
            m->ends_seen += take * ends;
            lo += take;
            if (m->num && m->fill >= eager && (rc = flush(m))) return rc;
            continue;
        }
        // it did not fit: its appends are dropped (m->fill and m->windows still say what was there before), the buffer is merged - tau
        // may fall - and the range is redone in sub-ranges of at most cap window ends, which fit an empty buffer
        m->n_redone++;
        if ((rc = flush(m))) return rc;
        const uint64_t sub = m->cap / ends, end = lo + take;
        while (lo < end) {
            const uint64_t part = end - lo < sub ? end - lo : sub;
            if (m->cap - m->fill < part * ends && (rc = flush(m))) return rc;
            if ((rc = fitting(part))) return rc;
        }
    }
    return NTK_OK;
}

// the status of work on the handle's state: a failure marks the handle
int settled(ntk_minhash *m, int rc)
{
    if (rc) m->failed = rc;
    return rc;
}

Candidates candidates(const ntk_minhash *m, uint32_t slabs)
{
    Candidates c;
    c.buf = m->d_buf.p; c.cap = m->cap; c.ctr = m->d_ctr.p; c.tau = m->tau; c.slabs = slabs;
    return c;
}

}  // namespace

extern "C" {

int ntk_minhash_create(ntk_ctx *ctx, uint32_t k, uint32_t path, uint64_t num, uint64_t scaled, uint64_t buffer_entries, ntk_minhash **out)
{
    if (!ctx || !out) return NTK_ERR_BAD_ARG;
    *out = nullptr;
    if (k < 1 || k > kKMax) return NTK_ERR_BAD_K;
    if (path > NTK_PATH_BITS_CANONICAL) return NTK_ERR_BAD_ARG;
    if (k > 32 && path != NTK_PATH_BYTES_CANONICAL) return NTK_ERR_BAD_K;   // the 2-bit iterator stops at k = 32
    if ((num == 0) == (scaled == 0) || num > NTK_MINHASH_MAX_NUM) return NTK_ERR_BAD_ARG;
    if (buffer_entries == 0) buffer_entries = NTK_MINHASH_BUFFER_DEFAULT;
    if (buffer_entries < NTK_MINHASH_BUFFER_MIN || buffer_entries > NTK_MINHASH_BUFFER_MAX) return NTK_ERR_BAD_ARG;
    ntk_minhash *m = new (std::nothrow) ntk_minhash();
    if (!m) return NTK_ERR_NOMEM;
    int rc = m->bind(ctx, k, path);
    if (rc) { delete m; return rc; }
    m->num = num; m->scaled = scaled; m->max_hash = scaled ? kAll / scaled : kAll;
    m->cap = buffer_entries;
    if ((rc = m->d_buf.ensure(m->stream, m->cap, grow_exact)) || (rc = m->d_sorted.ensure(m->stream, m->cap, grow_exact)) ||
        (rc = m->d_ctr.ensure(m->stream, 4, grow_exact)) || (rc = m->h_stage.alloc(4)) || (rc = ntk_minhash_reset(m))) {
        ntk_minhash_destroy(m);
        return rc;
    }
    *out = m;
    return NTK_OK;
}

void ntk_minhash_destroy(ntk_minhash *m)
{
    if (!m) return;
    (void)hipSetDevice(m->device);
    (void)hipStreamSynchronize(m->stream);
    m->scratch.release();
    for (HashCounts *p : {&m->kept, &m->runs, &m->merged, &m->next}) p->release();
    m->d_buf.release(); m->d_sorted.release(); m->d_ctr.release(); m->d_tmp.release();
    m->h_stage.release();
    (void)hipGetLastError();
    delete m;
}

int ntk_minhash_reset(ntk_minhash *m)
{
    if (!m) return NTK_ERR_BAD_ARG;
    CT_HIPCHK(hipSetDevice(m->device));
    CT_HIPCHK(hipMemsetAsync(m->d_ctr.p, 0, 4 * sizeof(uint64_t), m->stream));
    m->n_kept = 0; m->fill = 0; m->holes = 0; m->windows = 0; m->ends_seen = 0; m->n_merges = 0; m->n_redone = 0;
    m->tau = m->max_hash;   // ~0 with `num`
    m->failed = 0;
    return NTK_OK;
}

int ntk_minhash_add_device(ntk_minhash *m, const uint8_t *d_seq, const uint8_t *d_qual, uint64_t n_bytes, const ntk_params *p)
{
    int rc = check_batch_params(m, p);
    if (rc || n_bytes == 0) return rc;
    if ((rc = check_batch_pointers(d_seq, d_qual))) return rc;
    if (m->failed) return m->failed;
    return settled(m, [&]() -> int {
    CT_HIPCHK(hipSetDevice(m->device));
    const unsigned resident = (unsigned)m->n_cu * kBlocksPerCu;
    if (m->k > 32) {
        WideFilterArgs a;
        a.seq = d_seq; a.n_bytes = n_bytes; a.k = m->k;
        set_quality(a, p, d_qual);
        const uint64_t runs = (n_bytes + kLaneRun - 1) / kLaneRun;
        return run_range(m, 0, runs, kLaneRun, [&](uint64_t lo, uint64_t hi, uint32_t slabs) {
            a.run_lo = lo; a.run_hi = hi; a.c = candidates(m, slabs);
            hipLaunchKernelGGL(mh_wide_filter_kernel, dim3(grid_for(hi - lo, kFilterThreads, resident)), dim3(kFilterThreads), 0, m->stream, a);
        });
    }
    // of every chunk only the windows ending at or after its start are taken
    return for_each_chunk(*m, m->scratch, d_seq, d_qual, n_bytes, p, [&](const Chunk &c) -> int {
        FilterArgs a;
        a.values = m->scratch.d_values.p; a.valid16 = m->scratch.d_valid16.p;
        return run_range(m, c.skip(), c.len(), 1, [&](uint64_t lo, uint64_t hi, uint32_t slabs) {
            a.first = lo; a.n = hi; a.c = candidates(m, slabs);
            const uint64_t rounds = (hi - lo + kPerLane - 1) / kPerLane;
            hipLaunchKernelGGL(mh_filter_kernel, dim3(grid_for(rounds, kFilterThreads, resident)), dim3(kFilterThreads), 0, m->stream, a);
        });
    });
    }());
}

int ntk_minhash_stats(ntk_minhash *m, struct ntk_minhash_stats *out)
{
    if (!m || !out) return NTK_ERR_BAD_ARG;
    if (m->failed) return m->failed;
    const int rc = settled(m, flush(m));
    if (rc) return rc;
    out->n_windows = m->windows;
    out->n_kept = m->n_kept;
    out->threshold = m->tau;
    out->num = m->num; out->scaled = m->scaled;
    out->buffer_entries = m->cap;
    out->n_merges = m->n_merges; out->n_redone = m->n_redone;
    out->k = m->k; out->path = m->path;
    return NTK_OK;
}

int ntk_minhash_read(ntk_minhash *m, uint64_t *hashes, uint64_t *counts, uint64_t cap, uint64_t *n)
{
    if (!m || !n || (cap && (!hashes || !counts))) return NTK_ERR_BAD_ARG;
    if (m->failed) return m->failed;
    const int rc = settled(m, flush(m));
    if (rc) return rc;
    *n = m->n_kept;
    if (m->n_kept > cap) return NTK_ERR_CAPACITY;
    if (m->n_kept == 0) return NTK_OK;
    CT_HIPCHK(hipMemcpyAsync(hashes, m->kept.k.p, m->n_kept * sizeof(uint64_t), hipMemcpyDeviceToHost, m->stream));
    CT_HIPCHK(hipMemcpyAsync(counts, m->kept.c.p, m->n_kept * sizeof(uint64_t), hipMemcpyDeviceToHost, m->stream));
    CT_HIPCHK(hipStreamSynchronize(m->stream));
    return NTK_OK;
}

int ntk_minhash_merge(ntk_minhash *m, const uint64_t *hashes, const uint64_t *counts, uint64_t n, uint64_t n_windows)
{
    if (!m || (n && !hashes)) return NTK_ERR_BAD_ARG;
    for (uint64_t i = 1; i < n; i++)
        if (hashes[i] <= hashes[i - 1]) return NTK_ERR_BAD_ARG;
    if (m->failed) return m->failed;
    return settled(m, [&]() -> int {
    int rc = flush(m);
    if (rc) return rc;
    // what can enter: nothing above tau (it only falls), and with `num` no more than the num smallest
    uint64_t take = 0;
    while (take < n && hashes[take] <= m->tau && (!m->num || take < m->num)) take++;
    if (take) {
        if ((rc = m->runs.ensure(m->stream, take))) return rc;
        CT_HIPCHK(hipMemcpyAsync(m->runs.k.p, hashes, take * sizeof(uint64_t), hipMemcpyHostToDevice, m->stream));
        std::vector<uint64_t> ones;
        if (!counts) {
            ones.assign(take, 1);
            counts = ones.data();
        }
        CT_HIPCHK(hipMemcpyAsync(m->runs.c.p, counts, take * sizeof(uint64_t), hipMemcpyHostToDevice, m->stream));
        CT_HIPCHK(hipStreamSynchronize(m->stream));   // the caller's arrays are free again
        if ((rc = combine(m, take))) return rc;
    }
    m->windows += n_windows;
    return write_counters(m);
    }());
}

int ntk_minhash_compare(const uint64_t *a, const uint64_t *ca, uint64_t na, const uint64_t *b, const uint64_t *cb, uint64_t nb, uint64_t num,
                        uint64_t max_hash, struct ntk_minhash_comparison *out)
{
    if (!out || (na && !a) || (nb && !b)) return NTK_ERR_BAD_ARG;
    for (uint64_t i = 1; i < na; i++)
        if (a[i] <= a[i - 1]) return NTK_ERR_BAD_ARG;
    for (uint64_t i = 1; i < nb; i++)
        if (b[i] <= b[i - 1]) return NTK_ERR_BAD_ARG;
    while (na && a[na - 1] > max_hash) na--;
    while (nb && b[nb - 1] > max_hash) nb--;
    uint64_t i = 0, j = 0, n_union = 0, n_shared = 0;
    double dot = 0.0, norm2_a = 0.0, norm2_b = 0.0;
    // the union in ascending order, up to num members
    while ((i < na || j < nb) && (num == 0 || n_union < num)) {
        const bool in_a = i < na && (j >= nb || a[i] <= b[j]), in_b = j < nb && (i >= na || b[j] <= a[i]);
        const double x = in_a ? (ca ? (double)ca[i] : 1.0) : 0.0, y = in_b ? (cb ? (double)cb[j] : 1.0) : 0.0;
        n_union++;
        if (in_a && in_b) { n_shared++; dot += x * y; }
        if (in_a) { norm2_a += x * x; i++; }
        if (in_b) { norm2_b += y * y; j++; }
    }
    out->n_a = na; out->n_b = nb;
    out->n_shared = n_shared; out->n_union = n_union;
    out->dot = dot; out->norm2_a = norm2_a; out->norm2_b = norm2_b;
    return NTK_OK;
}

}  // extern "C"
