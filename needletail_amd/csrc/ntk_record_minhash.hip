// One MinHash sketch per record of a device batch, all in one call (include/needletail_amd_record_minhash.h): the sketches of
// ntk_minhash.hip (bottom-s and scaled, with abundance; the same hash), but with a threshold PER RECORD and the record's index carried
// along with every candidate.  A consumer of the core's public ABI alone, on the shared scaffold (ntk_consumer.hpp): k <= 32, the values
// ntk_materialize_device_quality emits, chunk by chunk.
//
// State of a run: per record r the interval [lo[r], tau[r]] of hashes the filter appends, the window count, and start[r], the CSR of
// the kept list K = (record, hash, count) triples sorted by (record, hash), unique; a candidate buffer of `cap` (record, hash) pairs with
// a reservation counter on the device.  rmh_filter_kernel streams a range of window ends, finds each window's record from the offsets
// (one search per wave, then it advances) and appends what passes; a wave stages its appends in LDS and reserves room with one add per
// flush, exactly as many slots as it writes - nothing pads the buffer, so the hash ~0 needs no care.  A launch is only ever taken whole:
// the counter keeps counting past the capacity, the host reads it after every launch, and a launch that did not fit is discarded and
// redone in pieces of at most `cap` window ends.  A fold sorts the buffer with the kept entries of the records it can touch by
// (record, hash), adds the counts of equal pairs and keeps the first `num` of every record.  Bottom-s thresholds are guessed, verified
// and raised (ntk_rmh_rule.hpp): rmh_retry_kernel scans only the records that were not accepted, and only for the hashes above their old
// threshold.  DESIGN.md section 18.
#include "../../include/needletail_amd_record_minhash.h"
#include "ntk_consumer.hpp"
#include "ntk_rmh_rule.hpp"

#include <rocprim/device/device_radix_sort.hpp>
#include <rocprim/device/device_scan.hpp>

#include <new>
#include <vector>

namespace {

constexpr uint64_t kXor = 0x9E3779B97F4A7C15ull;         // the MinHash library's C
constexpr int kFilterThreads = 256;
constexpr unsigned kBlocksPerCu = 8;                     // 6 KB of LDS per block
constexpr uint32_t kPerLane = 4;                         // window ends per lane and tile (loads in flight)
constexpr uint64_t kTile = 64 * kPerLane;                // window ends a wave takes at a time: lane l has t0 + l, + 64, + 128, + 192
constexpr uint32_t kStage = 128;                         // pairs a wave stages in LDS before it reserves room for them
constexpr uint64_t kSegment = 4 * kTile * 4;             // retry: window ends of a record a block takes at a time (4 tiles per wave)
constexpr uint64_t kAll = ~(uint64_t)0;
constexpr int kCtrFill = 0, kCtrList = 1, kCtrMinRec = 2, kCtrWords = 4;

static_assert(kXor == NTK_RECORD_MINHASH_XOR, "the header states the hash constant");
static_assert(kRmhAllPass == NTK_RECORD_MINHASH_ALLPASS, "the header states the all-pass length");
static_assert(NTK_RECORD_MINHASH_BUFFER_MIN >= kTile, "a redo piece is at least one tile");
static_assert(kStage >= 2 * 64, "a wave's appends of one step fit an empty stage");

__device__ inline uint64_t record_minhash_hash(uint64_t key) { return fmix64(key ^ kXor); }

struct Buffer {
    uint64_t *hash;     // the candidates' hashes ...
    uint32_t *rec;      // ... and records
    uint64_t cap;       // pairs it holds
    uint64_t *fill;     // slots reserved so far (counts on past cap)
};

// a wave's staged appends, in LDS
struct Stage {
    uint64_t hash[kStage];
    uint32_t rec[kStage];
};

// the wave's n staged pairs (n > 0, the same in every lane) into the buffer: one agent-scope add, coalesced stores, only below the capacity
__device__ inline void stage_flush(const Buffer &b, volatile Stage *st, uint32_t n)
{
    const uint32_t lane = threadIdx.x & 63;
    uint64_t base = 0;
    if (lane == 0) base = __hip_atomic_fetch_add(b.fill, (uint64_t)n, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    base = uniform(__shfl(base, 0, 64));
    for (uint32_t i = lane; i < n; i += 64) {
        const uint64_t at = base + i;
        if (at < b.cap) { b.hash[at] = st->hash[i]; b.rec[at] = st->rec[i]; }
    }
    __builtin_amdgcn_wave_barrier();
}

// every lane of the wave calls this together; those with `pass` stage (r, h).  n: the wave's staged pairs, the same in every lane.
__device__ __forceinline__ void stage_push(const Buffer &b, volatile Stage *st, uint32_t &n, bool pass, uint64_t h, uint32_t r)
{
    const uint64_t mask = __ballot(pass);
    if (!mask) return;
    const uint32_t add = (uint32_t)__popcll(mask);
    if (n + add > kStage) { stage_flush(b, st, n); n = 0; }
    if (pass) {
        const uint32_t at = n + (uint32_t)__popcll(mask & (((uint64_t)1 << (threadIdx.x & 63)) - 1));
        st->hash[at] = h; st->rec[at] = r;
    }
    n += add;
    __builtin_amdgcn_wave_barrier();
}

struct Scan {
    const uint64_t *values;    // materialised values of the chunk, indexed by window end - base
    const uint16_t *valid16;   // bit (15 - x % 16) of word x / 16: the window ending at base + x is emitted
    uint64_t base;             // the chunk was materialised from this byte of the batch (a multiple of 16)
    const uint64_t *offsets;   // n_records + 1 record starts
    uint64_t n_records, n_bytes;
    uint32_t k;
    const uint64_t *lo, *tau;  // per record: hashes in [lo, tau] are appended
    Buffer b;
};

__device__ inline bool plane_bit(uint16_t word, uint64_t x) { return (word >> (15 - (x & 15))) & 1u; }

// record start j (j <= n_records) as the rule reads it: beyond the batch is its end
__device__ inline uint64_t start_of(const Scan &s, uint64_t j)
{
    const uint64_t o = s.offsets[j];
    return o > s.n_bytes ? s.n_bytes : o;
}

// The window ends [t0, t1) (at most kTile) of which those in [first, last) are record r's, all of them: kPerLane coalesced 8-byte loads
// in flight with the valid plane's bit, then hash, compare with the record's interval and stage.  Everything but the lane is uniform.
__device__ __forceinline__ void scan_tile(const Scan &s, uint64_t t0, uint64_t t1, uint64_t first, uint64_t last, uint64_t hlo, uint64_t hhi,
                                          uint32_t r, volatile Stage *st, uint32_t &n)
{
    const uint32_t lane = threadIdx.x & 63;
    uint64_t key[kPerLane];
    bool ok[kPerLane];
#pragma unroll
    for (uint32_t u = 0; u < kPerLane; u++) {
        const uint64_t e = t0 + u * 64 + lane, x = e - s.base;
        ok[u] = e < t1 && e >= first && e < last;
        key[u] = ok[u] ? s.values[x] : 0;
        ok[u] = ok[u] && plane_bit(s.valid16[x >> 4], x);
    }
#pragma unroll
    for (uint32_t u = 0; u < kPerLane; u++) {
        const uint64_t h = record_minhash_hash(key[u]);
        stage_push(s.b, st, n, ok[u] && h >= hlo && h <= hhi, h, r);
    }
}

struct StreamArgs {
    Scan s;
    uint64_t lo, hi;   // the window ends [lo, hi) of the batch are taken (inside the chunk)
};

// Round 0, every record.  The tiles of [lo, hi) are dealt to the waves in contiguous runs, so a wave searches the offsets once, for the
// first window end of its run, and advances from there: i is the number of record starts at or before the tile's first end, so the end
// belongs to record i - 1 (nobody's where i is 0 or n_records + 1).  A tile inside one record - every tile but two of a long record -
// takes the uniform path; a tile that holds a record start lets every lane advance on its own from i.
__global__ __launch_bounds__(kFilterThreads) void rmh_filter_kernel(StreamArgs a)
{
    __shared__ Stage stages[kFilterThreads / 64];
    const Scan &s = a.s;
    const uint32_t lane = threadIdx.x & 63, wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    volatile Stage *st = stages + wave;
    const uint64_t waves = (uint64_t)gridDim.x * (kFilterThreads / 64), w = (uint64_t)blockIdx.x * (kFilterThreads / 64) + wave;
    const uint64_t tiles = (a.hi - a.lo + kTile - 1) / kTile, per = (tiles + waves - 1) / waves;
    const uint64_t t_begin = w * per, t_end = t_begin + per < tiles ? t_begin + per : tiles;
    if (t_begin >= t_end) return;
    // i = |{j <= n_records : start_of(j) <= first end}|
    const uint64_t e0 = a.lo + t_begin * kTile;
    uint64_t i = 0, top = s.n_records + 1;
    while (i < top) {
        const uint64_t mid = uniform(i + (top - i) / 2);
        if (start_of(s, mid) <= e0) i = mid + 1; else top = mid;
    }
    uint32_t n = 0;
    uint64_t cur = kAll, first = 0, last = 0, hlo = 1, hhi = 0;   // the record whose span and interval are loaded (i - 1), if any
    for (uint64_t t = t_begin; t < t_end; t++) {
        const uint64_t t0 = a.lo + t * kTile, t1 = t0 + kTile < a.hi ? t0 + kTile : a.hi;
        while (i <= s.n_records && uniform(start_of(s, i)) <= t0) i++;
        const uint64_t next = i <= s.n_records ? uniform(start_of(s, i)) : kAll;   // the first end that is not record i - 1's
        if (next >= t1) {
            if (i == 0 || i > s.n_records) continue;
            if (cur != i - 1) {
                cur = i - 1;
                const uint64_t b = uniform(start_of(s, cur));
                first = b + s.k - 1; last = next - 1;   // next >= t1 >= 1
                hlo = uniform(s.lo[cur]); hhi = uniform(s.tau[cur]);
            }
            scan_tile(s, t0, t1, first, last, hlo, hhi, (uint32_t)cur, st, n);
            continue;
        }
#pragma unroll 1
        for (uint32_t u = 0; u < kPerLane; u++) {
            const uint64_t e = t0 + u * 64 + lane, x = e - s.base;
            bool ok = e < t1;
            uint64_t j = i;
            if (ok)
                while (j <= s.n_records && start_of(s, j) <= e) j++;
            ok = ok && j >= 1 && j <= s.n_records;
            const uint64_t r = ok ? j - 1 : 0;
            if (ok) ok = e >= start_of(s, r) + s.k - 1 && e + 1 < start_of(s, j);
            const uint64_t key = ok ? s.values[x] : 0;
            ok = ok && plane_bit(s.valid16[x >> 4], x);
            const uint64_t rlo = ok ? s.lo[r] : 1, rhi = ok ? s.tau[r] : 0;
            const uint64_t h = record_minhash_hash(key);
            stage_push(s.b, st, n, ok && h >= rlo && h <= rhi, h, (uint32_t)r);
        }
    }
    if (n) stage_flush(s.b, st, n);
}

struct RetryArgs {
    Scan s;
    uint64_t lo, hi;          // only window ends in [lo, hi) are taken (inside the chunk)
    const uint32_t *list;     // the records of this round
    uint64_t n_list;
};

// A later round: only the listed records, each one's span cut into segments that the blocks share (every block walks the list; block
// b takes the segments (b - i) mod gridDim, + gridDim, ... of entry i).  No search: the record is known.
__global__ __launch_bounds__(kFilterThreads) void rmh_retry_kernel(RetryArgs a)
{
    __shared__ Stage stages[kFilterThreads / 64];
    const Scan &s = a.s;
    const uint32_t wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    volatile Stage *st = stages + wave;
    uint32_t n = 0;
    for (uint64_t i = 0; i < a.n_list; i++) {
        const uint64_t r = a.list[i];
        uint64_t first, last;
        record_span(s.offsets, s.n_bytes, s.k, r, first, last);
        const uint64_t lo = first > a.lo ? first : a.lo, hi = last < a.hi ? last : a.hi;
        if (lo >= hi) continue;
        const uint64_t segments = (hi - lo + kSegment - 1) / kSegment;
        const uint64_t hlo = uniform(s.lo[r]), hhi = uniform(s.tau[r]);
        for (uint64_t seg = (blockIdx.x + gridDim.x - i % gridDim.x) % gridDim.x; seg < segments; seg += gridDim.x) {
            const uint64_t s0 = lo + seg * kSegment, s1 = s0 + kSegment < hi ? s0 + kSegment : hi;
            for (uint64_t t0 = s0 + wave * kTile; t0 < s1; t0 += (kFilterThreads / 64) * kTile)
                scan_tile(s, t0, t0 + kTile < s1 ? t0 + kTile : s1, lo, hi, hlo, hhi, (uint32_t)r, st, n);
        }
    }
    if (n) stage_flush(s.b, st, n);
}

struct WindowsArgs {
    const uint16_t *valid16;
    uint64_t base, lo, hi;     // the chunk's plane, from `base`; its own window ends are [lo, hi)
    const uint64_t *offsets;
    uint64_t n_bytes, r0, r1;  // the records [r0, r1) can have windows here
    uint32_t k;
    uint64_t *windows;         // per record, added to
};

// n_windows: a block per record (grid-stride) counts the plane's bits over the record's span inside the chunk.  Launches of one run
// follow each other on the stream, and a record has one block per launch: a plain add.
__global__ __launch_bounds__(kThreads) void rmh_windows_kernel(WindowsArgs a)
{
    __shared__ uint32_t lds[kThreads / 64];
    for (uint64_t r = a.r0 + blockIdx.x; r < a.r1; r += gridDim.x) {
        uint64_t lo, hi;
        record_span(a.offsets, a.n_bytes, a.k, r, lo, hi);
        if (lo < a.lo) lo = a.lo;
        if (hi > a.hi) hi = a.hi;
        if (lo >= hi) continue;   // (the same for the whole block)
        const uint64_t x0 = lo - a.base, x1 = hi - a.base;
        uint32_t count = 0;
        for (uint64_t w = (x0 >> 4) + threadIdx.x; w < (x1 + 15) >> 4; w += kThreads) {
            uint32_t bits = a.valid16[w];
            if (w * 16 < x0) bits &= 0xFFFFu >> (x0 - w * 16);
            if (w * 16 + 16 > x1) bits &= (0xFFFFu << (w * 16 + 16 - x1)) & 0xFFFFu;
            count += __popc(bits);
        }
        count = block_sum_u32(count, lds);
        if (threadIdx.x == 0) a.windows[r] += count;
        __syncthreads();   // the words are free again
    }
}

// ---- the fold's own kernels: one thread per entry ----------------------------------------------------------------------------------

__global__ void rmh_iota_kernel(uint32_t *idx, uint64_t n)
{
    const uint64_t i = (uint64_t)blockIdx.x * kThreads + threadIdx.x;
    if (i < n) idx[i] = (uint32_t)i;
}

__global__ void rmh_gather_rec_kernel(const uint32_t *rec, const uint32_t *idx, uint32_t *out, uint64_t n)
{
    const uint64_t i = (uint64_t)blockIdx.x * kThreads + threadIdx.x;
    if (i < n) out[i] = rec[idx[i]];
}

struct HeadsArgs {
    const uint32_t *idx;       // the order by (record, hash) of the fold's entries
    const uint32_t *rec;       // records in that order
    const uint64_t *hash;      // hashes by entry
    const uint64_t *kept_cnt;  // counts of the first n_kept entries (the others count 1)
    uint64_t n_kept, n;
    uint64_t *out_hash, *out_cnt;   // in order
    uint32_t *head;                 // 1 where a new (record, hash) begins
};

__global__ void rmh_heads_kernel(HeadsArgs a)
{
    const uint64_t i = (uint64_t)blockIdx.x * kThreads + threadIdx.x;
    if (i >= a.n) return;
    const uint32_t j = a.idx[i];
    const uint64_t h = a.hash[j];
    a.out_hash[i] = h;
    a.out_cnt[i] = j < a.n_kept ? a.kept_cnt[j] : 1;
    a.head[i] = i == 0 || a.rec[i - 1] != a.rec[i] || a.hash[a.idx[i - 1]] != h;
}

struct GroupsArgs {
    const uint32_t *rec, *head, *group;   // in order; group: the inclusive scan of head
    const uint64_t *hash, *cnt, *sum;     // in order; sum: the inclusive scan of cnt
    uint64_t n;
    uint32_t *g_rec;                      // per group ...
    uint64_t *g_hash, *g_begin, *g_end;   // ... its count is g_end - g_begin
};

__global__ void rmh_groups_kernel(GroupsArgs a)
{
    const uint64_t i = (uint64_t)blockIdx.x * kThreads + threadIdx.x;
    if (i >= a.n) return;
    const uint32_t g = a.group[i] - 1;
    if (a.head[i]) { a.g_rec[g] = a.rec[i]; a.g_hash[g] = a.hash[i]; a.g_begin[g] = a.sum[i] - a.cnt[i]; }
    if (i + 1 == a.n || a.head[i + 1]) a.g_end[g] = a.sum[i];
}

__device__ inline uint64_t lower_bound_u32(const uint32_t *a, uint64_t n, uint64_t v)
{
    uint64_t lo = 0, hi = n;
    while (lo < hi) {
        const uint64_t mid = lo + (hi - lo) / 2;
        if (a[mid] < v) lo = mid + 1; else hi = mid;
    }
    return lo;
}

// per record r = r0 + t, t < n_seg: where its groups begin and how many it keeps; entry n_seg closes the scan
__global__ void rmh_segments_kernel(const uint32_t *g_rec, uint64_t n_groups, uint64_t r0, uint64_t n_seg, uint64_t limit, uint64_t *seg_start,
                                    uint64_t *len)
{
    const uint64_t t = (uint64_t)blockIdx.x * kThreads + threadIdx.x;
    if (t > n_seg) return;
    if (t == n_seg) { len[t] = 0; return; }
    const uint64_t b = lower_bound_u32(g_rec, n_groups, r0 + t), e = lower_bound_u32(g_rec, n_groups, r0 + t + 1);
    seg_start[t] = b;
    len[t] = e - b < limit ? e - b : limit;
}

struct KeepArgs {
    const uint32_t *g_rec;
    const uint64_t *g_hash, *g_begin, *g_end, *seg_start, *start;   // start: the kept list's CSR, already the new one
    uint64_t n_groups, r0, limit;
    uint32_t *k_rec;
    uint64_t *k_hash, *k_cnt;
};

__global__ void rmh_keep_kernel(KeepArgs a)
{
    const uint64_t g = (uint64_t)blockIdx.x * kThreads + threadIdx.x;
    if (g >= a.n_groups) return;
    const uint64_t r = a.g_rec[g];
    if (r < a.r0) return;   // (only offsets that fall would put a candidate there)
    const uint64_t rank = g - a.seg_start[r - a.r0];
    if (rank >= a.limit) return;
    const uint64_t at = a.start[r] + rank;
    a.k_rec[at] = (uint32_t)r; a.k_hash[at] = a.g_hash[g]; a.k_cnt[at] = a.g_end[g] - a.g_begin[g];
}

struct AcceptArgs {
    const uint32_t *list;     // the round's records; nullptr: all n of them
    uint64_t n, num;
    const uint64_t *start;
    uint64_t *lo, *tau;
    uint32_t *next;           // the next round's records ...
    uint64_t *ctr;            // ... their number (kCtrList) and the smallest of them (kCtrMinRec)
};

// ntk_rmh_rule.hpp on every record of the round
__global__ void rmh_accept_kernel(AcceptArgs a)
{
    const uint64_t i = (uint64_t)blockIdx.x * kThreads + threadIdx.x;
    if (i >= a.n) return;
    const uint64_t r = a.list ? a.list[i] : i, tau = a.tau[r], distinct = a.start[r + 1] - a.start[r];
    if (rmh_accept(tau, distinct, a.num)) return;
    a.lo[r] = tau + 1;
    a.tau[r] = rmh_raise(tau, distinct, a.num);
    const uint64_t at = __hip_atomic_fetch_add(a.ctr + kCtrList, (uint64_t)1, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    a.next[at] = (uint32_t)r;
    (void)__hip_atomic_fetch_min(a.ctr + kCtrMinRec, r, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}

}  // namespace

struct ntk_record_minhash : Consumer {
    uint64_t num = 0, scaled = 0, max_hash = kAll, limit = kAll;
    uint64_t cap = 0;                           // buffer_entries
    Pinned<uint64_t> h_stage;                   // kCtrWords words
    MaterialiseScratch scratch;
    DeviceArray<uint64_t> ctr;                  // kCtrFill: slots reserved; kCtrList, kCtrMinRec: rmh_accept_kernel's
    DeviceArray<uint64_t> b_hash;               // the candidate buffer
    DeviceArray<uint32_t> b_rec;
    DeviceArray<uint64_t> lo, tau, windows, start, seg_start, len;   // per record (start, len: one more)
    DeviceArray<uint32_t> list_a, list_b;       // the round's records and the next round's
    DeviceArray<uint32_t> k_rec;                // K
    DeviceArray<uint64_t> k_hash, k_cnt;
    // a fold's work arrays: its entries (the kept ones first), two index arrays, sorted keys, the order's records, hashes, counts and
    // heads with their scans, and the groups
    DeviceArray<uint64_t> w_hash, s_hash, o_cnt, o_sum, g_hash, g_begin, g_end;
    DeviceArray<uint32_t> w_rec, idx_a, idx_b, r_a, r_b, o_head, o_group, g_rec;
    DeviceArray<char> tmp;                      // rocPRIM's temporary storage
    std::vector<uint64_t> h_offsets;            // the batch's record starts, read back once per run
    uint64_t n_records = 0;                     // of the held result
    bool held = false;                          // a result is held (n_records may be 0)
    bool on_device = false;                     // ... and its arrays are on the device (else every sketch is empty)
    uint64_t n_kept = 0, fill = 0, fold_from = kAll;   // fold_from: no record below it has a candidate in the buffer
    uint64_t n_rounds = 0, n_retried = 0, n_redone = 0, sum_windows = 0;
    int failed = 0;                             // the status of a run that failed halfway

    // f(array) for every device array above (the scratch is apart): what release_all frees is what stats counts
    template <class F>
    void each_array(F f)
    {
        for (DeviceArray<uint64_t> *d : {&ctr, &b_hash, &lo, &tau, &windows, &start, &seg_start, &len, &k_hash, &k_cnt, &w_hash, &s_hash,
                                         &o_cnt, &o_sum, &g_hash, &g_begin, &g_end})
            f(*d);
        for (DeviceArray<uint32_t> *d : {&b_rec, &list_a, &list_b, &k_rec, &w_rec, &idx_a, &idx_b, &r_a, &r_b, &o_head, &o_group, &g_rec})
            f(*d);
        f(tmp);
    }

    void release_all()
    {
        scratch.release();
        each_array([](auto &d) { d.release(); });
    }
};

namespace {

using Handle = ntk_record_minhash;

inline unsigned blocks_for(uint64_t n) { return (unsigned)((n + kThreads - 1) / kThreads); }

// The buffer's m->fill pairs into K, with the kept entries of the records from m->fold_from on (no record below it has a candidate, and
// K is sorted by record, so those are a suffix of K and everything before it stays as it is).  The fold's entries are that suffix, then
// the buffer.  Order: a sort by hash, then a stable sort by record.  Equal (record, hash) pairs are neighbours then: heads, two scans,
// one group per distinct pair with the sum of its counts; per record the first `limit` groups are kept and K's CSR from fold_from on is
// written anew.  Afterwards the buffer is empty and the device counter says so.
int fold(Handle *m, uint64_t n_records)
{
    if (m->fill == 0) return NTK_OK;
    int rc;
    const uint64_t r0 = m->fold_from < n_records ? m->fold_from : 0;
    if ((rc = m->h_stage.read(m->stream, m->start.p + r0, 1))) return rc;
    const uint64_t p = m->h_stage.p[0], n_suffix = m->n_kept - p, n = n_suffix + m->fill, n_seg = n_records - r0;
    if (n >> 32) return NTK_ERR_CAPACITY;
    hipStream_t st = m->stream;
    for (DeviceArray<uint64_t> *d : {&m->w_hash, &m->s_hash, &m->o_cnt, &m->o_sum, &m->g_hash, &m->g_begin, &m->g_end})
        if ((rc = d->ensure(st, n, grow_half_again))) return rc;
    for (DeviceArray<uint32_t> *d : {&m->w_rec, &m->idx_a, &m->idx_b, &m->r_a, &m->r_b, &m->o_head, &m->o_group, &m->g_rec})
        if ((rc = d->ensure(st, n, grow_half_again))) return rc;
    if (n_suffix) {
        CT_HIPCHK(hipMemcpyAsync(m->w_hash.p, m->k_hash.p + p, n_suffix * sizeof(uint64_t), hipMemcpyDeviceToDevice, st));
        CT_HIPCHK(hipMemcpyAsync(m->w_rec.p, m->k_rec.p + p, n_suffix * sizeof(uint32_t), hipMemcpyDeviceToDevice, st));
    }
    CT_HIPCHK(hipMemcpyAsync(m->w_hash.p + n_suffix, m->b_hash.p, m->fill * sizeof(uint64_t), hipMemcpyDeviceToDevice, st));
    CT_HIPCHK(hipMemcpyAsync(m->w_rec.p + n_suffix, m->b_rec.p, m->fill * sizeof(uint32_t), hipMemcpyDeviceToDevice, st));
    const unsigned blocks = blocks_for(n);
    hipLaunchKernelGGL(rmh_iota_kernel, dim3(blocks), dim3(kThreads), 0, st, m->idx_a.p, n);
    CT_HIPCHK(hipGetLastError());
    rc = with_tmp(m->tmp, st, grow_half_again, [&](void *tmp, size_t &bytes) {
        return rocprim::radix_sort_pairs(tmp, bytes, m->w_hash.p, m->s_hash.p, m->idx_a.p, m->idx_b.p, (size_t)n, 0u, 64u, st);
    });
    if (rc) return rc;
    hipLaunchKernelGGL(rmh_gather_rec_kernel, dim3(blocks), dim3(kThreads), 0, st, m->w_rec.p, m->idx_b.p, m->r_a.p, n);
    CT_HIPCHK(hipGetLastError());
    unsigned rec_bits = 1;
    while (rec_bits < 32 && (n_records - 1) >> rec_bits) rec_bits++;
    rc = with_tmp(m->tmp, st, grow_half_again, [&](void *tmp, size_t &bytes) {
        return rocprim::radix_sort_pairs(tmp, bytes, m->r_a.p, m->r_b.p, m->idx_b.p, m->idx_a.p, (size_t)n, 0u, rec_bits, st);
    });
    if (rc) return rc;
    HeadsArgs h;
    h.idx = m->idx_a.p; h.rec = m->r_b.p; h.hash = m->w_hash.p; h.kept_cnt = m->k_cnt.p ? m->k_cnt.p + p : nullptr;
    h.n_kept = n_suffix; h.n = n;
    h.out_hash = m->s_hash.p; h.out_cnt = m->o_cnt.p; h.head = m->o_head.p;   // (the first sort's keys are not needed again)
    hipLaunchKernelGGL(rmh_heads_kernel, dim3(blocks), dim3(kThreads), 0, st, h);
    CT_HIPCHK(hipGetLastError());
    rc = with_tmp(m->tmp, st, grow_half_again, [&](void *tmp, size_t &bytes) {
        return rocprim::inclusive_scan(tmp, bytes, m->o_head.p, m->o_group.p, (size_t)n, rocprim::plus<uint32_t>(), st);
    });
    if (rc) return rc;
    rc = with_tmp(m->tmp, st, grow_half_again, [&](void *tmp, size_t &bytes) {
        return rocprim::inclusive_scan(tmp, bytes, m->o_cnt.p, m->o_sum.p, (size_t)n, rocprim::plus<uint64_t>(), st);
    });
    if (rc) return rc;
    GroupsArgs g;
    g.rec = m->r_b.p; g.head = m->o_head.p; g.group = m->o_group.p; g.hash = m->s_hash.p; g.cnt = m->o_cnt.p; g.sum = m->o_sum.p; g.n = n;
    g.g_rec = m->g_rec.p; g.g_hash = m->g_hash.p; g.g_begin = m->g_begin.p; g.g_end = m->g_end.p;
    hipLaunchKernelGGL(rmh_groups_kernel, dim3(blocks), dim3(kThreads), 0, st, g);
    CT_HIPCHK(hipGetLastError());
    // the number of groups: the last entry's
    CT_HIPCHK(hipMemcpyAsync(m->h_stage.p, m->o_group.p + (n - 1), sizeof(uint32_t), hipMemcpyDeviceToHost, st));
    CT_HIPCHK(hipStreamSynchronize(st));
    const uint64_t n_groups = *(const uint32_t *)m->h_stage.p;
    hipLaunchKernelGGL(rmh_segments_kernel, dim3(blocks_for(n_seg + 1)), dim3(kThreads), 0, st, m->g_rec.p, n_groups, r0, n_seg, m->limit,
                       m->seg_start.p, m->len.p);
    CT_HIPCHK(hipGetLastError());
    rc = with_tmp(m->tmp, st, grow_half_again, [&](void *tmp, size_t &bytes) {
        return rocprim::exclusive_scan(tmp, bytes, m->len.p, m->start.p + r0, p, (size_t)(n_seg + 1), rocprim::plus<uint64_t>(), st);
    });
    if (rc) return rc;
    if ((rc = m->h_stage.read(st, m->start.p + n_records, 1))) return rc;
    const uint64_t n_kept = m->h_stage.p[0];
    if (n_kept >> 32) return NTK_ERR_CAPACITY;
    if ((rc = m->k_rec.ensure(st, n_kept, grow_half_again, p)) || (rc = m->k_hash.ensure(st, n_kept, grow_half_again, p)) ||
        (rc = m->k_cnt.ensure(st, n_kept, grow_half_again, p)))
        return rc;
    KeepArgs k;
    k.g_rec = m->g_rec.p; k.g_hash = m->g_hash.p; k.g_begin = m->g_begin.p; k.g_end = m->g_end.p; k.seg_start = m->seg_start.p;
    k.start = m->start.p; k.n_groups = n_groups; k.r0 = r0; k.limit = m->limit;
    k.k_rec = m->k_rec.p; k.k_hash = m->k_hash.p; k.k_cnt = m->k_cnt.p;
    hipLaunchKernelGGL(rmh_keep_kernel, dim3(blocks_for(n_groups)), dim3(kThreads), 0, st, k);
    CT_HIPCHK(hipGetLastError());
    m->n_kept = n_kept;
    m->fill = 0; m->fold_from = kAll;
    m->h_stage.p[0] = 0;
    return m->h_stage.write(st, m->ctr.p + kCtrFill, 1);
}

// the record that holds window end e, or the one before it (host offsets; never above the true one)
uint64_t record_at(const Handle *m, uint64_t n_records, uint64_t n_bytes, uint64_t e)
{
    uint64_t lo = 0, hi = n_records + 1;
    while (lo < hi) {
        const uint64_t mid = lo + (hi - lo) / 2;
        const uint64_t o = m->h_offsets[mid] > n_bytes ? n_bytes : m->h_offsets[mid];
        if (o <= e) lo = mid + 1; else hi = mid;
    }
    return lo ? lo - 1 : 0;
}

// The redo rule over the window ends [lo, hi) of a chunk.  launch(lo, hi) queues a filter over them; `from` is a record no candidate
// of it lies below.  The launch is followed by a read of the counter and taken whole, or discarded and redone in pieces of at most
// cap window ends, each into an empty buffer.
template <class Launch>
int run_range(Handle *m, uint64_t n_records, uint64_t lo, uint64_t hi, uint64_t from, Launch launch)
{
    int rc;
    if (lo >= hi) return NTK_OK;
    if (m->fill > m->cap / 2 && (rc = fold(m, n_records))) return rc;   // a launch that does not fit costs a pass over its range
    auto take = [&](uint64_t a, uint64_t b) -> int {
        launch(a, b);
        CT_HIPCHK(hipGetLastError());
        if ((rc = m->h_stage.read(m->stream, m->ctr.p + kCtrFill, 1))) return rc;
        if (from < m->fold_from) m->fold_from = from;
        return NTK_OK;
    };
    if ((rc = take(lo, hi))) return rc;
    if (m->h_stage.p[0] <= m->cap) { m->fill = m->h_stage.p[0]; return NTK_OK; }
    // it did not fit: its appends are dropped (m->fill still says what was there before) and the range is redone
    m->n_redone++;
    m->h_stage.p[0] = m->fill;
    if ((rc = m->h_stage.write(m->stream, m->ctr.p + kCtrFill, 1)) || (rc = fold(m, n_records))) return rc;
    for (uint64_t a = lo; a < hi; a += m->cap) {
        if ((rc = take(a, hi - a < m->cap ? hi : a + m->cap))) return rc;
        if (m->h_stage.p[0] > m->cap) return NTK_ERR_HIP;   // cannot happen
        m->fill = m->h_stage.p[0];
        if ((rc = fold(m, n_records))) return rc;
    }
    return NTK_OK;
}

Scan scan_of(Handle *m, const Chunk &c, const uint64_t *d_offsets, uint64_t n_records, uint64_t n_bytes)
{
    Scan s;
    s.values = m->scratch.d_values.p; s.valid16 = m->scratch.d_valid16.p; s.base = c.base;
    s.offsets = d_offsets; s.n_records = n_records; s.n_bytes = n_bytes; s.k = m->k;
    s.lo = m->lo.p; s.tau = m->tau.p;
    s.b.hash = m->b_hash.p; s.b.rec = m->b_rec.p; s.b.cap = m->cap; s.b.fill = m->ctr.p + kCtrFill;
    return s;
}

// the whole run; a failure in here marks the handle
int run(Handle *m, const uint8_t *d_seq, const uint8_t *d_qual, uint64_t n_bytes, const uint64_t *d_offsets, uint64_t n_records,
        const ntk_params *p)
{
    int rc;
    hipStream_t st = m->stream;
    CT_HIPCHK(hipSetDevice(m->device));
    try {
        m->h_offsets.resize(n_records + 1);
    } catch (const std::bad_alloc &) {
        return NTK_ERR_NOMEM;
    }
    CT_HIPCHK(hipMemcpyAsync(m->h_offsets.data(), d_offsets, (n_records + 1) * sizeof(uint64_t), hipMemcpyDeviceToHost, st));
    if ((rc = m->ctr.ensure(st, kCtrWords, grow_exact)) || (rc = m->b_hash.ensure(st, m->cap, grow_exact)) ||
        (rc = m->b_rec.ensure(st, m->cap, grow_exact)))
        return rc;
    for (DeviceArray<uint64_t> *d : {&m->lo, &m->tau, &m->windows, &m->start, &m->seg_start, &m->len})
        if ((rc = d->ensure(st, n_records + 1, grow_half_again))) return rc;
    if (m->num && ((rc = m->list_a.ensure(st, n_records, grow_half_again)) || (rc = m->list_b.ensure(st, n_records, grow_half_again))))
        return rc;
    CT_HIPCHK(hipMemsetAsync(m->ctr.p, 0, kCtrWords * sizeof(uint64_t), st));
    CT_HIPCHK(hipMemsetAsync(m->lo.p, 0, n_records * sizeof(uint64_t), st));
    CT_HIPCHK(hipMemsetAsync(m->windows.p, 0, n_records * sizeof(uint64_t), st));
    CT_HIPCHK(hipMemsetAsync(m->start.p, 0, (n_records + 1) * sizeof(uint64_t), st));
    CT_HIPCHK(hipStreamSynchronize(st));   // the offsets are here
    // the first thresholds, from the host's copy of the offsets
    {
        std::vector<uint64_t> tau;
        try {
            tau.resize(n_records);
        } catch (const std::bad_alloc &) {
            return NTK_ERR_NOMEM;
        }
        for (uint64_t r = 0; r < n_records; r++) {
            uint64_t b = m->h_offsets[r], e = m->h_offsets[r + 1];
            if (e > n_bytes) e = n_bytes;
            if (b > e) b = e;
            const uint64_t hi = e ? e - 1 : 0, lo = b + m->k - 1 > hi ? hi : b + m->k - 1;   // record_span
            tau[r] = m->num ? rmh_guess(hi - lo, m->num) : m->max_hash;
        }
        CT_HIPCHK(hipMemcpyAsync(m->tau.p, tau.data(), n_records * sizeof(uint64_t), hipMemcpyHostToDevice, st));
        CT_HIPCHK(hipStreamSynchronize(st));
    }
    m->on_device = true;
    const unsigned resident = (unsigned)m->n_cu * kBlocksPerCu;
    // round 0: every window of every chunk; of a chunk only the windows ending at or after its start are taken
    rc = for_each_chunk(*m, m->scratch, d_seq, d_qual, n_bytes, p, [&](const Chunk &c) -> int {
        const uint64_t r0 = record_at(m, n_records, n_bytes, c.start), r1 = record_at(m, n_records, n_bytes, c.end - 1) + 1;
        WindowsArgs w;
        w.valid16 = m->scratch.d_valid16.p; w.base = c.base; w.lo = c.start; w.hi = c.end;
        w.offsets = d_offsets; w.n_bytes = n_bytes; w.r0 = r0; w.r1 = r1 < n_records ? r1 : n_records; w.k = m->k;
        w.windows = m->windows.p;
        hipLaunchKernelGGL(rmh_windows_kernel, dim3(grid_for(w.r1 - w.r0, 1, resident)), dim3(kThreads), 0, st, w);
        CT_HIPCHK(hipGetLastError());
        StreamArgs a;
        a.s = scan_of(m, c, d_offsets, n_records, n_bytes);
        return run_range(m, n_records, c.start, c.end, r0, [&](uint64_t lo, uint64_t hi) {
            a.lo = lo; a.hi = hi;
            const uint64_t tiles = (hi - lo + kTile - 1) / kTile;
            hipLaunchKernelGGL(rmh_filter_kernel, dim3(grid_for(tiles, kFilterThreads / 64, resident)), dim3(kFilterThreads), 0, st, a);
        });
    });
    if (rc || (rc = fold(m, n_records))) return rc;
    m->n_rounds = 1;
    // bottom-s: verify, raise, scan the records that were not accepted again
    uint32_t *list = nullptr, *next = m->list_a.p;
    uint64_t n_list = n_records;
    while (m->num && n_list) {
        m->h_stage.p[0] = 0; m->h_stage.p[1] = kAll;
        CT_HIPCHK(hipMemcpyAsync(m->ctr.p + kCtrList, m->h_stage.p, 2 * sizeof(uint64_t), hipMemcpyHostToDevice, st));
        AcceptArgs q;
        q.list = list; q.n = n_list; q.num = m->num; q.start = m->start.p; q.lo = m->lo.p; q.tau = m->tau.p; q.next = next; q.ctr = m->ctr.p;
        hipLaunchKernelGGL(rmh_accept_kernel, dim3(blocks_for(n_list)), dim3(kThreads), 0, st, q);
        CT_HIPCHK(hipGetLastError());
        if ((rc = m->h_stage.read(st, m->ctr.p + kCtrList, 2))) return rc;
        n_list = m->h_stage.p[0];
        if (n_list == 0) break;
        const uint64_t from = m->h_stage.p[1];
        if (m->n_rounds == 1) m->n_retried = n_list;
        m->n_rounds++;
        list = next;
        next = list == m->list_a.p ? m->list_b.p : m->list_a.p;
        auto body = [&](const Chunk &c) -> int {
            RetryArgs a;
            a.s = scan_of(m, c, d_offsets, n_records, n_bytes);
            a.list = list; a.n_list = n_list;
            return run_range(m, n_records, c.start, c.end, from, [&](uint64_t lo, uint64_t hi) {
                a.lo = lo; a.hi = hi;
                hipLaunchKernelGGL(rmh_retry_kernel, dim3(resident), dim3(kFilterThreads), 0, st, a);
            });
        };
        // a batch of one chunk is still in the scratch
        rc = n_bytes <= kChunkBases ? body(chunk_at(n_bytes, m->k, 0)) : for_each_chunk(*m, m->scratch, d_seq, d_qual, n_bytes, p, body);
        if (rc || (rc = fold(m, n_records))) return rc;
    }
    // the sum of the window counts, for stats
    std::vector<uint64_t> &w = m->h_offsets;   // (free again)
    CT_HIPCHK(hipMemcpyAsync(w.data(), m->windows.p, n_records * sizeof(uint64_t), hipMemcpyDeviceToHost, st));
    CT_HIPCHK(hipStreamSynchronize(st));
    m->sum_windows = 0;
    for (uint64_t r = 0; r < n_records; r++) m->sum_windows += w[r];
    return NTK_OK;
}

}  // namespace

extern "C" {

int ntk_record_minhash_create(ntk_ctx *ctx, uint32_t k, uint32_t path, uint64_t num, uint64_t scaled, uint64_t buffer_entries,
                              ntk_record_minhash **out)
{
    if (!ctx || !out) return NTK_ERR_BAD_ARG;
    *out = nullptr;
    if (k < 1 || k > 32) return NTK_ERR_BAD_K;
    if (path > NTK_PATH_BITS_CANONICAL) return NTK_ERR_BAD_ARG;
    if ((num == 0) == (scaled == 0) || num > NTK_RECORD_MINHASH_MAX_NUM) return NTK_ERR_BAD_ARG;
    if (buffer_entries == 0) buffer_entries = NTK_RECORD_MINHASH_BUFFER_DEFAULT;
    if (buffer_entries < NTK_RECORD_MINHASH_BUFFER_MIN || buffer_entries > NTK_RECORD_MINHASH_BUFFER_MAX) return NTK_ERR_BAD_ARG;
    ntk_record_minhash *m = new (std::nothrow) ntk_record_minhash();
    if (!m) return NTK_ERR_NOMEM;
    int rc = m->bind(ctx, k, path);
    if (rc) { delete m; return rc; }
    m->num = num; m->scaled = scaled; m->max_hash = scaled ? kAll / scaled : kAll; m->limit = num ? num : kAll;
    m->cap = buffer_entries;
    if ((rc = m->h_stage.alloc(kCtrWords))) { delete m; return rc; }
    *out = m;
    return NTK_OK;
}

int ntk_record_minhash_trim(ntk_record_minhash *m)
{
    if (!m) return NTK_ERR_BAD_ARG;
    CT_HIPCHK(hipSetDevice(m->device));
    CT_HIPCHK(hipStreamSynchronize(m->stream));
    m->release_all();
    (void)hipGetLastError();
    m->held = m->on_device = false;
    m->n_records = m->n_kept = m->fill = m->sum_windows = 0;
    m->failed = 0;
    return NTK_OK;
}

void ntk_record_minhash_destroy(ntk_record_minhash *m)
{
    if (!m) return;
    (void)ntk_record_minhash_trim(m);
    m->h_stage.release();
    (void)hipGetLastError();
    delete m;
}

int ntk_record_minhash_run_device(ntk_record_minhash *m, const uint8_t *d_seq, const uint8_t *d_qual, uint64_t n_bytes,
                                  const uint64_t *d_offsets, uint64_t n_records, const ntk_params *p)
{
    int rc = check_batch_params(m, p);
    if (rc) return rc;
    if (n_records >> 32) return NTK_ERR_BAD_ARG;
    const bool empty = n_records == 0 || n_bytes == 0;
    if (!empty) {
        if ((rc = check_batch_pointers(d_seq, d_qual))) return rc;
        if (!d_offsets || ((uintptr_t)d_offsets & 7)) return NTK_ERR_BAD_ARG;
    }
    // the run starts over: nothing of the result held so far is part of the new one
    m->held = true; m->on_device = false; m->failed = 0;
    m->n_records = n_records;
    m->n_kept = m->fill = m->sum_windows = 0; m->fold_from = kAll;
    m->n_rounds = m->n_retried = m->n_redone = 0;
    if (empty) return NTK_OK;
    rc = run(m, d_seq, d_qual, n_bytes, d_offsets, n_records, p);
    if (rc) m->failed = rc;
    return rc;
}

int ntk_record_minhash_read(ntk_record_minhash *m, uint64_t *offsets, uint64_t *n_windows, uint64_t *hashes, uint64_t *counts, uint64_t cap,
                            uint64_t *n)
{
    if (!m || !n || (cap && (!hashes || !counts))) return NTK_ERR_BAD_ARG;
    if (m->failed) return m->failed;
    *n = m->held ? m->n_kept : 0;
    if (!m->held) return NTK_OK;
    if (m->n_kept > cap) return NTK_ERR_CAPACITY;
    if (!offsets) return NTK_OK;   // the size alone
    if (!m->on_device) {
        for (uint64_t r = 0; r <= m->n_records; r++) offsets[r] = 0;
        for (uint64_t r = 0; n_windows && r < m->n_records; r++) n_windows[r] = 0;
        return NTK_OK;
    }
    CT_HIPCHK(hipSetDevice(m->device));
    CT_HIPCHK(hipMemcpyAsync(offsets, m->start.p, (m->n_records + 1) * sizeof(uint64_t), hipMemcpyDeviceToHost, m->stream));
    if (n_windows)
        CT_HIPCHK(hipMemcpyAsync(n_windows, m->windows.p, m->n_records * sizeof(uint64_t), hipMemcpyDeviceToHost, m->stream));
    if (m->n_kept) {
        CT_HIPCHK(hipMemcpyAsync(hashes, m->k_hash.p, m->n_kept * sizeof(uint64_t), hipMemcpyDeviceToHost, m->stream));
        CT_HIPCHK(hipMemcpyAsync(counts, m->k_cnt.p, m->n_kept * sizeof(uint64_t), hipMemcpyDeviceToHost, m->stream));
    }
    CT_HIPCHK(hipStreamSynchronize(m->stream));
    return NTK_OK;
}

int ntk_record_minhash_stats(ntk_record_minhash *m, struct ntk_record_minhash_stats *out)
{
    if (!m || !out) return NTK_ERR_BAD_ARG;
    if (m->failed) return m->failed;
    out->n_records = m->held ? m->n_records : 0;
    out->n_entries = m->held ? m->n_kept : 0;
    out->n_windows = m->held ? m->sum_windows : 0;
    out->num = m->num; out->scaled = m->scaled;
    out->buffer_entries = m->cap;
    out->n_rounds = m->n_rounds; out->n_retried_records = m->n_retried; out->n_redone = m->n_redone;
    out->device_bytes = m->scratch.device_bytes();   // values, and two planes of 2 B per 16 bases
    m->each_array([&](const auto &d) { out->device_bytes += d.bytes(); });
    out->k = m->k; out->path = m->path;
    return NTK_OK;
}

}  // extern "C"
