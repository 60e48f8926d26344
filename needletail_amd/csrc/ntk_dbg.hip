// The compacted de Bruijn graph of a k-mer list (include/needletail_amd_dbg.h).  A consumer of the core's public ABI like the other
// libraries (it takes the context's device and stream and nothing else), and of no other library: it works on the format the count
// tables' extract and the k-mer sets library write and never touches a table.  ntk_dbg_rule.hpp has the rule and every per-element
// step; the kernels here hand elements to it:
//
//   dbg_dir_mark_kernel   the first key of every prefix bucket marks the reversed directory; rocPRIM's running minimum fills the
//                         empty buckets, so that a lookup is two directory words and a search inside one bucket.
//   dbg_adjacency_kernel  one lane per k-mer: the edge byte and, per side with exactly one bit, the target's index.  The degree bins
//                         are added up in LDS and flushed with one agent-scope add per non-zero bin and block.
//   dbg_link_kernel       one lane per (k-mer, side): next[2 i + side].
//   dbg_rank_*_kernel     pointer doubling over the 2 n states, (pointer, hops) in one word and the smallest key index beside it,
//                         between two buffers; a round that moves a pointer raises the round's agent-scope flag.  Cycles are what has
//                         not reached a terminal; dbg_rank_cut_kernel cuts them and the rounds run again.
//   dbg_resolve_kernel    one lane per k-mer: its unitig's first k-mer, its position and orientation.  rocPRIM's exclusive scan over
//                         the start k-mers numbers the unitigs and lays their k-mers out; dbg_perm_kernel writes that order down, a
//                         second scan over the counts in that order gives every unitig's sum as a difference (no atomic per k-mer),
//                         and dbg_rows_kernel writes both kinds of rows.
//   dbg_spell_kernel      one lane per k-mer: its first base at its place of the record; the lane of a unitig's last k-mer adds the
//                         k - 1 bases behind it and the break byte.  Work is per k-mer, so a long unitig is no long task.
// DESIGN.md section 20.
#include "../../include/needletail_amd_dbg.h"
#include "ntk_consumer.hpp"
#include "ntk_dbg_rule.hpp"

#include <rocprim/device/device_scan.hpp>
#include <rocprim/iterator/counting_iterator.hpp>
#include <rocprim/iterator/transform_iterator.hpp>

#include <cstring>
#include <new>

namespace {

constexpr unsigned kBlocksPerCu = 16;               // grid-stride launches: at most this many blocks per CU
constexpr uint32_t kSmallWords = 128;               // the handle's small device words: the sums, then one flag per ranking round
constexpr uint32_t kFlagAt = 32, kCycleFlag = 0;    // flag 0: a state is on a cycle; flags 1 ..: a pointer moved in round r
constexpr uint32_t kBinWords = 32;                  // LDS bins of dbg_adjacency_kernel: the 25 degree bins and the self loops

static_assert(DBG_K_MIN == NTK_DBG_K_MIN && DBG_K_MAX == NTK_DBG_K_MAX && DBG_N_MAX == NTK_DBG_N_MAX, "the rule's limits are the header's");
static_assert(sizeof(ntk_dbg_totals) == DBG_N_TOTALS * sizeof(uint64_t), "dbg_totals fills thirty-one words");
static_assert(sizeof(ntk_dbg_kmer_row) == 8 && sizeof(ntk_dbg_unitig_row) == 32, "the header states the rows");
static_assert(DBG_N_SUMS <= kFlagAt && DBG_SUM_SELF < kBinWords && kFlagAt + 2 * 33 + 2 <= kSmallWords, "the sums and the flags fit their words");
static_assert(NTK_DBG_UNITIG_BYTES_PER_KMER == 8 + 2 * 16 + 2 * 8 + 8 + 4 + 16 + 4 + 8, "next, two state buffers, place, length, scan, order, sums");

struct ScanItem {
    uint64_t units, kmers;   // unitigs that start, and k-mers they hold, before this k-mer
};

struct ScanAdd {
    __host__ __device__ ScanItem operator()(const ScanItem &x, const ScanItem &y) const
    {
        return ScanItem{x.units + y.units, x.kmers + y.kmers};
    }
};

// what k-mer i adds to the scan; nothing for i = n, whose scanned item is the total
struct StartItem {
    const uint32_t *len;
    uint64_t n;
    __device__ ScanItem operator()(uint64_t i) const
    {
        const uint32_t l = i < n ? len[i] : 0;
        return l ? ScanItem{1, l & ~DBG_CYCLE_BIT} : ScanItem{0, 0};
    }
};

// the count of the j-th k-mer in unitig order; 0 for j = n
struct OrderedCount {
    const uint32_t *perm;
    const uint64_t *counts;
    uint64_t n;
    __device__ uint64_t operator()(uint64_t j) const
    {
        if (j >= n) return 0;
        const uint32_t i = perm[j] >> 1;
        return i < n ? counts[i] : 0;
    }
};

// the bytes of record u; 0 for u = n_unitigs
struct RecordBytes {
    const ntk_dbg_unitig_row *rows;
    uint64_t n_unitigs, n, k;
    __device__ uint64_t operator()(uint64_t u) const
    {
        if (u >= n_unitigs) return 0;
        const uint64_t l = rows[u].n_kmers;
        return (l < n ? l : n) + k;
    }
};

__global__ __launch_bounds__(kThreads) void dbg_dir_mark_kernel(const uint64_t *keys, uint32_t n, uint32_t k, uint32_t b, uint32_t *rdir)
{
    const uint64_t stride = (uint64_t)gridDim.x * kThreads;
    for (uint64_t i = (uint64_t)blockIdx.x * kThreads + threadIdx.x; i < n; i += stride) {
        uint64_t slot = 0;
        if (dbg_dir_mark(keys, k, b, (uint32_t)i, slot)) atomicMin(rdir + slot, (uint32_t)i);   // (one writer per slot on a k-mer list)
        if (i == 0) rdir[0] = n;
    }
}

__global__ __launch_bounds__(kThreads) void dbg_adjacency_kernel(const uint64_t *keys, uint32_t n, const uint32_t *rdir, uint32_t k, uint32_t b,
                                                                 uint8_t *edges, uint32_t *tgt, uint64_t *sums)
{
    __shared__ uint32_t bins[kBinWords];
    if (threadIdx.x < kBinWords) bins[threadIdx.x] = 0;
    __syncthreads();
    const uint64_t stride = (uint64_t)gridDim.x * kThreads;   // a block takes fewer than 2^32 k-mers: its u32 bins cannot overflow
    for (uint64_t i = (uint64_t)blockIdx.x * kThreads + threadIdx.x; i < n; i += stride) {
        const DbgAdj a = dbg_adjacency(keys, n, rdir, k, b, (uint32_t)i);
        edges[i] = (uint8_t)a.edges;
        tgt[2 * i] = a.tgt[0];
        tgt[2 * i + 1] = a.tgt[1];
        atomicAdd(&bins[dbg_deg_bin(a.edges)], 1u);
        if (a.n_self) atomicAdd(&bins[DBG_SUM_SELF], a.n_self);
    }
    __syncthreads();
    if (threadIdx.x < kBinWords && bins[threadIdx.x]) add_agent(sums + threadIdx.x, bins[threadIdx.x]);
}

// next may be NULL: the links are only counted
__global__ __launch_bounds__(kThreads) void dbg_link_kernel(const uint64_t *keys, const uint8_t *edges, const uint32_t *tgt, uint32_t n, uint32_t k,
                                                            uint32_t *next, uint64_t *sums)
{
    const uint64_t stride = (uint64_t)gridDim.x * kThreads, states = 2 * (uint64_t)n;
    uint64_t links = 0;
    for (uint64_t d = (uint64_t)blockIdx.x * kThreads + threadIdx.x; d < states; d += stride) {
        const uint32_t nx = dbg_link(keys, edges, tgt, n, k, (uint32_t)(d >> 1), (uint32_t)(d & 1));
        if (next) next[d] = nx;
        links += nx != DBG_NONE;
    }
    links = wave_sum(links);
    if ((threadIdx.x & 63) == 0 && links) add_agent(sums + DBG_SUM_LINKS, links);
}

__global__ __launch_bounds__(kThreads) void dbg_rank_init_kernel(const uint32_t *next, uint64_t states, uint64_t *pd, uint32_t *mn)
{
    const uint64_t stride = (uint64_t)gridDim.x * kThreads;
    for (uint64_t d = (uint64_t)blockIdx.x * kThreads + threadIdx.x; d < states; d += stride) dbg_rank_init(next, (uint32_t)d, pd[d], mn[d]);
}

__global__ __launch_bounds__(kThreads) void dbg_rank_round_kernel(const uint64_t *pd_in, const uint32_t *mn_in, uint64_t *pd_out, uint32_t *mn_out,
                                                                  uint64_t states, uint64_t *flag)
{
    const uint64_t stride = (uint64_t)gridDim.x * kThreads;
    bool moved = false;
    for (uint64_t d = (uint64_t)blockIdx.x * kThreads + threadIdx.x; d < states; d += stride)
        moved |= dbg_rank_round(pd_in, mn_in, pd_out, mn_out, (uint32_t)d);
    if (__ballot(moved) && (threadIdx.x & 63) == 0) __hip_atomic_store(flag, (uint64_t)1, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}

__global__ __launch_bounds__(kThreads) void dbg_rank_cut_kernel(const uint32_t *next, uint64_t *pd, const uint32_t *mn, uint64_t states,
                                                                uint64_t *flag)
{
    const uint64_t stride = (uint64_t)gridDim.x * kThreads;
    bool cycle = false;
    for (uint64_t d = (uint64_t)blockIdx.x * kThreads + threadIdx.x; d < states; d += stride) cycle |= dbg_rank_cut(next, pd, mn, (uint32_t)d);
    if (__ballot(cycle) && (threadIdx.x & 63) == 0) __hip_atomic_store(flag, (uint64_t)1, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}

__global__ __launch_bounds__(kThreads) void dbg_resolve_kernel(const uint32_t *next, const uint64_t *pd, const uint32_t *mn, uint32_t n, uint2 *place,
                                                               uint32_t *len)
{
    const uint64_t stride = (uint64_t)gridDim.x * kThreads;
    for (uint64_t i = (uint64_t)blockIdx.x * kThreads + threadIdx.x; i < n; i += stride) {
        const DbgPlace r = dbg_resolve(next, pd, mn, (uint32_t)i);
        place[i] = make_uint2(r.start < n ? r.start : (uint32_t)i, r.pos_flip);
        len[i] = r.len;
    }
}

// perm[the unitig's first slot + position] = i << 1 | flipped
__global__ __launch_bounds__(kThreads) void dbg_perm_kernel(const uint2 *place, const ScanItem *scan, uint32_t n, uint32_t *perm)
{
    const uint64_t stride = (uint64_t)gridDim.x * kThreads;
    for (uint64_t i = (uint64_t)blockIdx.x * kThreads + threadIdx.x; i < n; i += stride) {
        const uint2 p = place[i];
        const uint64_t at = scan[p.x].kmers + (p.y >> 1);
        if (at < n) perm[at] = ((uint32_t)i << 1) | (p.y & 1);
    }
}

struct RowsArgs {
    const uint2 *place;
    const uint32_t *len, *perm;
    const ScanItem *scan;
    const uint64_t *prefix;    // n + 1: the counts before slot j of the unitig order
    const uint8_t *edges;
    uint32_t n;
    uint64_t n_unitigs;
    ntk_dbg_kmer_row *kmer_rows;
    ntk_dbg_unitig_row *unitig_rows;
};

__global__ __launch_bounds__(kThreads) void dbg_rows_kernel(RowsArgs a)
{
    const uint64_t stride = (uint64_t)gridDim.x * kThreads;
    for (uint64_t i = (uint64_t)blockIdx.x * kThreads + threadIdx.x; i < a.n; i += stride) {
        const uint2 p = a.place[i];
        ntk_dbg_kmer_row kr;
        kr.unitig = (uint32_t)a.scan[p.x].units;
        kr.pos_flip = p.y;
        a.kmer_rows[i] = kr;
        const uint32_t l = a.len[i];
        if (!l) continue;
        const ScanItem s = a.scan[i];
        if (s.units >= a.n_unitigs) continue;
        const uint64_t L = l & ~DBG_CYCLE_BIT;
        const uint64_t first = s.kmers < a.n ? s.kmers : a.n, end = first + L < a.n ? first + L : a.n;   // end > first on a k-mer list
        const uint32_t last = a.perm[end ? end - 1 : 0], li = (last >> 1) < a.n ? last >> 1 : (uint32_t)i;
        ntk_dbg_unitig_row ur;
        ur.start_index = i;
        ur.n_kmers = L;
        ur.sum_counts = a.prefix[end] - a.prefix[first];
        ur.flags = dbg_row_flags((l & DBG_CYCLE_BIT) != 0, a.edges[i], p.y & 1, a.edges[li], last & 1);
        a.unitig_rows[s.units] = ur;
    }
}

struct SpellArgs {
    const uint64_t *keys;
    const ntk_dbg_kmer_row *kmer_rows;
    const ntk_dbg_unitig_row *unitig_rows;
    const uint64_t *offsets;   // n_unitigs + 1
    uint32_t n, k;
    uint64_t n_unitigs, total;
    uint8_t *out;
};

__global__ __launch_bounds__(kThreads) void dbg_spell_kernel(SpellArgs a)
{
    if (blockIdx.x == 0 && threadIdx.x < 16 && a.total + threadIdx.x < ((a.total + 15) & ~(uint64_t)15)) a.out[a.total + threadIdx.x] = (uint8_t)'\n';
    const uint64_t stride = (uint64_t)gridDim.x * kThreads;
    for (uint64_t i = (uint64_t)blockIdx.x * kThreads + threadIdx.x; i < a.n; i += stride) {
        const ntk_dbg_kmer_row r = a.kmer_rows[i];
        if (r.unitig >= a.n_unitigs) continue;
        const uint64_t L = a.unitig_rows[r.unitig].n_kmers, pos = r.pos_flip >> 1;
        if (pos >= L) continue;
        const uint64_t at = a.offsets[r.unitig] + pos, end = a.offsets[r.unitig + 1];   // end <= total
        const uint64_t x = a.keys[i] & dbg_mask(a.k), v = (r.pos_flip & 1) ? dbg_rc(x, a.k) : x;
        if (pos + 1 < L) {
            if (at < end) a.out[at] = dbg_base(v, a.k, 0);
        } else if (at + a.k < end) {
            for (uint32_t j = 0; j < a.k; j++) a.out[at + j] = dbg_base(v, a.k, j);
            a.out[at + a.k] = (uint8_t)'\n';
        }
    }
}

}  // namespace

struct ntk_dbg : Consumer {
    DeviceArray<uint64_t> d_small;         // kSmallWords: the sums and the flags
    Pinned<uint64_t> h_stage;              // likewise
    // adjacency
    DeviceArray<uint32_t> d_rdir;          // the reversed prefix directory: dbg_dir_words
    DeviceArray<uint8_t> d_edges;          // n, where the caller keeps none
    DeviceArray<uint32_t> d_tgt;           // 2 n
    // unitigs
    DeviceArray<uint32_t> d_next;          // 2 n
    DeviceArray<uint64_t> d_pd[2];         // 2 n each
    DeviceArray<uint32_t> d_mn[2];         // 2 n each
    DeviceArray<uint2> d_place;            // n
    DeviceArray<uint32_t> d_len, d_perm;   // n each
    DeviceArray<ScanItem> d_scan;          // n + 1
    DeviceArray<uint64_t> d_prefix;        // n + 1
    // spell
    DeviceArray<uint64_t> d_offsets;       // n_unitigs + 1
    DeviceArray<char> d_scan_tmp;          // rocPRIM's temporary storage
    uint64_t n_launches = 0, n_calls = 0, n_rounds = 0;

    void release_scratch()
    {
        d_rdir.release(); d_edges.release(); d_tgt.release(); d_next.release();
        for (int q = 0; q < 2; q++) { d_pd[q].release(); d_mn[q].release(); }
        d_place.release(); d_len.release(); d_perm.release(); d_scan.release(); d_prefix.release(); d_offsets.release(); d_scan_tmp.release();
    }

    uint64_t device_bytes() const
    {
        return d_small.bytes() + d_rdir.bytes() + d_edges.bytes() + d_tgt.bytes() + d_next.bytes() + d_pd[0].bytes() + d_pd[1].bytes() +
               d_mn[0].bytes() + d_mn[1].bytes() + d_place.bytes() + d_len.bytes() + d_perm.bytes() + d_scan.bytes() + d_prefix.bytes() +
               d_offsets.bytes() + d_scan_tmp.bytes();
    }

    unsigned grid(uint64_t items) const { return grid_for(items, kThreads, (unsigned)n_cu * kBlocksPerCu); }
};

namespace {

#define DBG_LAUNCH(h, kernel, items, ...)                                                                   \
    do {                                                                                                    \
        hipLaunchKernelGGL(kernel, dim3((h)->grid(items)), dim3(kThreads), 0, (h)->stream, __VA_ARGS__);    \
        CT_HIPCHK(hipGetLastError());                                                                       \
        (h)->n_launches++;                                                                                  \
    } while (0)

// the running minimum over the marked directory, in place
hipError_t fill_directory(ntk_dbg *h, void *tmp, size_t &tmp_bytes, uint64_t words)
{
    return rocprim::inclusive_scan(tmp, tmp_bytes, h->d_rdir.p, h->d_rdir.p, (size_t)words, rocprim::minimum<uint32_t>(), h->stream);
}

hipError_t scan_starts(ntk_dbg *h, void *tmp, size_t &tmp_bytes, uint64_t n)
{
    auto items = rocprim::make_transform_iterator(rocprim::counting_iterator<uint64_t>(0), StartItem{h->d_len.p, n});
    return rocprim::exclusive_scan(tmp, tmp_bytes, items, h->d_scan.p, ScanItem{0, 0}, (size_t)(n + 1), ScanAdd(), h->stream);
}

hipError_t scan_counts(ntk_dbg *h, void *tmp, size_t &tmp_bytes, const uint64_t *d_counts, uint64_t n)
{
    auto items = rocprim::make_transform_iterator(rocprim::counting_iterator<uint64_t>(0), OrderedCount{h->d_perm.p, d_counts, n});
    return rocprim::exclusive_scan(tmp, tmp_bytes, items, h->d_prefix.p, (uint64_t)0, (size_t)(n + 1), rocprim::plus<uint64_t>(), h->stream);
}

hipError_t scan_records(ntk_dbg *h, void *tmp, size_t &tmp_bytes, const ntk_dbg_unitig_row *rows, uint64_t n_unitigs, uint64_t n)
{
    auto items = rocprim::make_transform_iterator(rocprim::counting_iterator<uint64_t>(0), RecordBytes{rows, n_unitigs, n, h->k});
    return rocprim::exclusive_scan(tmp, tmp_bytes, items, h->d_offsets.p, (uint64_t)0, (size_t)(n_unitigs + 1), rocprim::plus<uint64_t>(),
                                   h->stream);
}

// The directory, the edge bytes into `edges`, the targets into d_tgt and, with `count_links` or `next`, the links; the sums are on the
// device afterwards.  0 < n <= DBG_N_MAX.
int run_adjacency(ntk_dbg *h, const uint64_t *d_keys, uint32_t n, uint8_t *edges, uint32_t *next, bool count_links)
{
    const uint32_t b = dbg_dir_bits(h->k, n);
    const uint64_t words = dbg_dir_words(h->k, n);
    int rc = h->d_rdir.ensure(h->stream, words, grow_exact);
    if (!rc) rc = h->d_tgt.ensure(h->stream, 2 * (uint64_t)n, grow_exact);
    if (rc) return rc;
    CT_HIPCHK(hipMemsetAsync(h->d_small.p, 0, kSmallWords * sizeof(uint64_t), h->stream));
    CT_HIPCHK(hipMemsetAsync(h->d_rdir.p, 0xFF, words * sizeof(uint32_t), h->stream));
    DBG_LAUNCH(h, dbg_dir_mark_kernel, n, d_keys, n, h->k, b, h->d_rdir.p);
    rc = with_tmp(h->d_scan_tmp, h->stream, grow_exact, [&](void *tmp, size_t &tmp_bytes) { return fill_directory(h, tmp, tmp_bytes, words); });
    if (rc) return rc;
    DBG_LAUNCH(h, dbg_adjacency_kernel, n, d_keys, n, h->d_rdir.p, h->k, b, edges, h->d_tgt.p, h->d_small.p);
    if (next || count_links) DBG_LAUNCH(h, dbg_link_kernel, 2 * (uint64_t)n, d_keys, edges, h->d_tgt.p, n, h->k, next, h->d_small.p);
    return NTK_OK;
}

// Pointer doubling from buffer `cur` until no pointer moves, at most dbg_rounds_max(n) rounds; `cur` is the settled buffer afterwards.
// flag_at: the first of the rounds' flags.
int run_rounds(ntk_dbg *h, uint32_t n, int &cur, uint32_t flag_at)
{
    const uint64_t states = 2 * (uint64_t)n;
    const uint32_t cap = dbg_rounds_max(n);
    for (uint32_t r = 0; r < cap; r++) {
        uint64_t *flag = h->d_small.p + flag_at + r;
        DBG_LAUNCH(h, dbg_rank_round_kernel, states, h->d_pd[cur].p, h->d_mn[cur].p, h->d_pd[cur ^ 1].p, h->d_mn[cur ^ 1].p, states, flag);
        cur ^= 1;
        h->n_rounds++;
        const int rc = h->h_stage.read(h->stream, flag, 1);
        if (rc) return rc;
        if (!h->h_stage.p[0]) break;
    }
    return NTK_OK;
}

bool aligned8(const void *p) { return ((uintptr_t)p & 7) == 0; }

}  // namespace

extern "C" {

int ntk_dbg_create(ntk_ctx *ctx, uint32_t k, ntk_dbg **out)
{
    if (!ctx || !out) return NTK_ERR_BAD_ARG;
    *out = nullptr;
    if (!dbg_k_ok(k)) return NTK_ERR_BAD_K;
    ntk_dbg *h = new (std::nothrow) ntk_dbg();
    if (!h) return NTK_ERR_NOMEM;
    int rc = h->bind(ctx, k, 0);
    if (rc) { delete h; return rc; }
    if ((rc = h->d_small.ensure(h->stream, kSmallWords, grow_exact)) || (rc = h->h_stage.alloc(kSmallWords))) {
        ntk_dbg_destroy(h);
        return rc;
    }
    *out = h;
    return NTK_OK;
}

void ntk_dbg_destroy(ntk_dbg *h)
{
    if (!h) return;
    (void)hipSetDevice(h->device);
    (void)hipStreamSynchronize(h->stream);
    h->release_scratch();
    h->d_small.release();
    h->h_stage.release();
    (void)hipGetLastError();
    delete h;
}

int ntk_dbg_release(ntk_dbg *h)
{
    if (!h) return NTK_ERR_BAD_ARG;
    CT_HIPCHK(hipSetDevice(h->device));
    CT_HIPCHK(hipStreamSynchronize(h->stream));
    h->release_scratch();
    return NTK_OK;
}

int ntk_dbg_stats(ntk_dbg *h, struct ntk_dbg_stats *out)
{
    if (!h || !out) return NTK_ERR_BAD_ARG;
    out->k = h->k;
    out->device_bytes = h->device_bytes();
    out->n_launches = h->n_launches;
    out->n_calls = h->n_calls;
    out->n_rounds = h->n_rounds;
    return NTK_OK;
}

int ntk_dbg_adjacency_device(ntk_dbg *h, const uint64_t *d_keys, uint64_t n, uint8_t *d_edges, struct ntk_dbg_totals *totals)
{
    if (!h || (n && !d_keys) || !aligned8(d_keys)) return NTK_ERR_BAD_ARG;
    if (n > DBG_N_MAX) return NTK_ERR_UNSUPPORTED;
    if (n == 0) {
        if (totals) memset(totals, 0, sizeof *totals);
        return NTK_OK;
    }
    CT_HIPCHK(hipSetDevice(h->device));
    int rc = d_edges ? NTK_OK : h->d_edges.ensure(h->stream, n, grow_exact);
    if (!rc) rc = run_adjacency(h, d_keys, (uint32_t)n, d_edges ? d_edges : h->d_edges.p, nullptr, totals != nullptr);
    if (rc) return rc;
    h->n_calls++;
    if ((rc = h->h_stage.read(h->stream, h->d_small.p, DBG_N_SUMS))) return rc;   // synchronises
    if (totals) dbg_totals(h->h_stage.p, &totals->n_half_edges);
    return NTK_OK;
}

int ntk_dbg_unitigs_device(ntk_dbg *h, const uint64_t *d_keys, const uint64_t *d_counts, uint64_t n, struct ntk_dbg_kmer_row *d_kmer_rows,
                           struct ntk_dbg_unitig_row *d_unitig_rows, uint64_t cap_unitigs, uint64_t *n_unitigs, uint64_t *n_bases)
{
    if (!h || !n_unitigs || !n_bases || (n && (!d_keys || !d_counts))) return NTK_ERR_BAD_ARG;
    if (!aligned8(d_keys) || !aligned8(d_counts) || !aligned8(d_kmer_rows) || !aligned8(d_unitig_rows)) return NTK_ERR_BAD_ARG;
    if (cap_unitigs && n && (!d_kmer_rows || !d_unitig_rows)) return NTK_ERR_BAD_ARG;
    if (n > DBG_N_MAX) return NTK_ERR_UNSUPPORTED;
    *n_unitigs = 0;
    *n_bases = 0;
    if (n == 0) return NTK_OK;
    CT_HIPCHK(hipSetDevice(h->device));
    const uint32_t n32 = (uint32_t)n;
    const uint64_t states = 2 * n;
    int rc = h->d_edges.ensure(h->stream, n, grow_exact);
    if (!rc) rc = h->d_next.ensure(h->stream, states, grow_exact);
    for (int q = 0; q < 2 && !rc; q++) {
        rc = h->d_pd[q].ensure(h->stream, states, grow_exact);
        if (!rc) rc = h->d_mn[q].ensure(h->stream, states, grow_exact);
    }
    if (!rc) rc = h->d_place.ensure(h->stream, n, grow_exact);
    if (!rc) rc = h->d_len.ensure(h->stream, n, grow_exact);
    if (!rc) rc = h->d_perm.ensure(h->stream, n, grow_exact);
    if (!rc) rc = h->d_scan.ensure(h->stream, n + 1, grow_exact);
    if (!rc) rc = h->d_prefix.ensure(h->stream, n + 1, grow_exact);
    if (!rc) rc = run_adjacency(h, d_keys, n32, h->d_edges.p, h->d_next.p, true);
    if (rc) return rc;
    h->n_calls++;
    h->n_rounds = 0;

    // the ranking: every state towards its terminal; what is left is on cycles, which are cut and ranked again
    int cur = 0;
    DBG_LAUNCH(h, dbg_rank_init_kernel, states, h->d_next.p, states, h->d_pd[0].p, h->d_mn[0].p);
    if ((rc = run_rounds(h, n32, cur, kFlagAt + 1))) return rc;
    DBG_LAUNCH(h, dbg_rank_cut_kernel, states, h->d_next.p, h->d_pd[cur].p, h->d_mn[cur].p, states, h->d_small.p + kFlagAt + kCycleFlag);
    if ((rc = h->h_stage.read(h->stream, h->d_small.p + kFlagAt + kCycleFlag, 1))) return rc;
    if (h->h_stage.p[0] && (rc = run_rounds(h, n32, cur, kFlagAt + 1 + 33))) return rc;

    // the unitigs: numbered and laid out by one scan over the start k-mers
    DBG_LAUNCH(h, dbg_resolve_kernel, n, h->d_next.p, h->d_pd[cur].p, h->d_mn[cur].p, n32, h->d_place.p, h->d_len.p);
    rc = with_tmp(h->d_scan_tmp, h->stream, grow_exact, [&](void *tmp, size_t &tmp_bytes) { return scan_starts(h, tmp, tmp_bytes, n); });
    if (rc) return rc;
    ScanItem *total = reinterpret_cast<ScanItem *>(h->h_stage.p);
    CT_HIPCHK(hipMemcpyAsync(total, h->d_scan.p + n, sizeof *total, hipMemcpyDeviceToHost, h->stream));
    CT_HIPCHK(hipStreamSynchronize(h->stream));
    const uint64_t units = total->units;
    *n_unitigs = units;
    *n_bases = n + units * (h->k - 1);
    if (units > cap_unitigs) return NTK_ERR_CAPACITY;

    DBG_LAUNCH(h, dbg_perm_kernel, n, h->d_place.p, h->d_scan.p, n32, h->d_perm.p);
    rc = with_tmp(h->d_scan_tmp, h->stream, grow_exact, [&](void *tmp, size_t &tmp_bytes) { return scan_counts(h, tmp, tmp_bytes, d_counts, n); });
    if (rc) return rc;
    RowsArgs g;
    g.place = h->d_place.p; g.len = h->d_len.p; g.perm = h->d_perm.p; g.scan = h->d_scan.p; g.prefix = h->d_prefix.p; g.edges = h->d_edges.p;
    g.n = n32; g.n_unitigs = units;
    g.kmer_rows = d_kmer_rows; g.unitig_rows = d_unitig_rows;
    DBG_LAUNCH(h, dbg_rows_kernel, n, g);
    CT_HIPCHK(hipStreamSynchronize(h->stream));
    return NTK_OK;
}

int ntk_dbg_spell_device(ntk_dbg *h, const uint64_t *d_keys, uint64_t n, const struct ntk_dbg_kmer_row *d_kmer_rows,
                         const struct ntk_dbg_unitig_row *d_unitig_rows, uint64_t n_unitigs, uint8_t *d_seq_out, uint64_t cap_bytes,
                         uint64_t *d_offsets_out, uint64_t cap_records, uint64_t *out_n_bytes, uint64_t *out_n_records)
{
    if (!h || !out_n_bytes || !out_n_records) return NTK_ERR_BAD_ARG;
    if (!aligned8(d_keys) || !aligned8(d_kmer_rows) || !aligned8(d_unitig_rows) || !aligned8(d_offsets_out) || ((uintptr_t)d_seq_out & 15))
        return NTK_ERR_BAD_ARG;
    if ((cap_bytes && !d_seq_out) || (cap_records && !d_offsets_out)) return NTK_ERR_BAD_ARG;
    if (n > DBG_N_MAX) return NTK_ERR_UNSUPPORTED;
    if (n_unitigs > n) return NTK_ERR_BAD_ARG;
    if (n_unitigs && (!d_keys || !d_kmer_rows || !d_unitig_rows)) return NTK_ERR_BAD_ARG;
    *out_n_bytes = 0;
    *out_n_records = 0;
    CT_HIPCHK(hipSetDevice(h->device));
    if (n_unitigs == 0) {
        if (d_offsets_out) CT_HIPCHK(hipMemsetAsync(d_offsets_out, 0, sizeof(uint64_t), h->stream));
        CT_HIPCHK(hipStreamSynchronize(h->stream));
        return NTK_OK;
    }
    int rc = h->d_offsets.ensure(h->stream, n_unitigs + 1, grow_exact);
    if (!rc) rc = with_tmp(h->d_scan_tmp, h->stream, grow_exact,
                           [&](void *tmp, size_t &tmp_bytes) { return scan_records(h, tmp, tmp_bytes, d_unitig_rows, n_unitigs, n); });
    if (rc || (rc = h->h_stage.read(h->stream, h->d_offsets.p + n_unitigs, 1))) return rc;
    h->n_calls++;
    const uint64_t total = h->h_stage.p[0];
    *out_n_bytes = total;
    *out_n_records = n_unitigs;
    if (((total + 15) & ~(uint64_t)15) > cap_bytes || n_unitigs > cap_records) return NTK_ERR_CAPACITY;
    CT_HIPCHK(hipMemcpyAsync(d_offsets_out, h->d_offsets.p, (n_unitigs + 1) * sizeof(uint64_t), hipMemcpyDeviceToDevice, h->stream));
    SpellArgs g;
    g.keys = d_keys; g.kmer_rows = d_kmer_rows; g.unitig_rows = d_unitig_rows; g.offsets = h->d_offsets.p;
    g.n = (uint32_t)n; g.k = h->k; g.n_unitigs = n_unitigs; g.total = total;
    g.out = d_seq_out;
    DBG_LAUNCH(h, dbg_spell_kernel, n, g);
    CT_HIPCHK(hipStreamSynchronize(h->stream));
    return NTK_OK;
}

}  // extern "C"
