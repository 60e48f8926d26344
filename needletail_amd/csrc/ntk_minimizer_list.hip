// The windowed minimizers of every record of a device batch as lists (include/needletail_amd/minimizer_list.h): per record the
// positions, values and strands of its (w, k) minimizers, each with the number of consecutive windows it won.  A consumer of the core's
// public ABI alone, on the shared scaffold (ntk_consumer.hpp): k <= 32, the values ntk_materialize_device_quality emits, chunk by chunk.
//
// The chunks are walked here and not by for_each_chunk: the halo in front of a chunk is that of k + w (chunk_at(n_bytes, k + w, start): a
// multiple of 16 and at least k + w - 1 bytes, so the window that ends one position before the chunk is whole in it and its choice decides
// whether the chunk's first window opens an entry), and a chunk is materialised w - 1 window ends further than its own (the tail), so
// an entry that opens in its last ends finds its whole span in the same pass.  Per chunk: ml_select_kernel writes a 2-byte word per
// window end (ntk_ml_rule.hpp) and counts the opening ends per tile; ml_scan_kernel scans the counts; the held list grows to take them (the
// entries of the chunks before stay); ml_scatter_kernel writes the entries in ascending order of first window end.  After the last chunk
// ml_offsets_kernel searches the record starts in the first-window-end list.  DESIGN.md section 22.
#include "../../include/needletail_amd/minimizer_list.h"
#include "ntk_consumer.hpp"
#include "ntk_ml_rule.hpp"

#include <new>

namespace {

constexpr int kCtrWindows = 0, kCtrWords = 2;

static_assert(ML_W_MAX == NTK_MINIMIZER_LIST_W_MAX && ML_XOR == NTK_MINIMIZER_LIST_XOR, "the header states the rule's constants");
static_assert(ML_ORDER_LEX == NTK_MINIMIZER_LIST_LEX && ML_ORDER_HASH == NTK_MINIMIZER_LIST_HASH, "the header states the orders");
static_assert(ML_THREADS == kThreads, "block_sum_u32 sums a block of kThreads");

__device__ inline bool plane_bit(uint16_t word, uint64_t x) { return (word >> (15 - (x & 15))) & 1u; }

struct TileArgs {
    const uint64_t *values;    // materialised values of the chunk, indexed by window end - base
    const uint16_t *valid16;   // bit (15 - x % 16) of word x / 16: the window ending at base + x is emitted
    const uint16_t *rc16;      // ... and its strand flag
    uint64_t base;             // the chunk was materialised from this byte of the batch (a multiple of 16)
    uint64_t lo, hi;           // the chunk's own window ends: their entries are counted and written
    uint64_t limit;            // the ends [lo, limit) have a word: hi and the tail
    uint32_t k, w, order;
    uint16_t *sel;             // the word of end x at sel[x - base]
    uint32_t *count;           // per tile of [lo, limit): its opening ends below hi
    uint64_t *ctr;             // kCtrWindows: whole windows below hi, added to
    // the scatter's
    const uint32_t *tile_base; // the exclusive scan of count
    const uint64_t *offsets;   // n_records + 1 record starts
    uint64_t n_records, n_bytes;
    uint64_t held;             // entries of the chunks before
    uint64_t *pos, *value, *end;
    uint32_t *info;
};

// record start j (j <= n_records) as the rule reads it: beyond the batch is its end
__device__ inline uint64_t start_of(const uint64_t *offsets, uint64_t n_bytes, uint64_t j)
{
    const uint64_t o = offsets[j];
    return o > n_bytes ? n_bytes : o;
}

// |{j in [lo, hi) : start_of(j) <= x}| + lo, the starts non-decreasing
__device__ inline uint64_t starts_at_or_before(const uint64_t *offsets, uint64_t n_bytes, uint64_t lo, uint64_t hi, uint64_t x)
{
    while (lo < hi) {
        const uint64_t mid = lo + (hi - lo) / 2;
        if (start_of(offsets, n_bytes, mid) <= x) lo = mid + 1; else hi = mid;
    }
    return lo;
}

// starts_at_or_before(0, n_records + 1, x), searched from `from` on, of which it is known that every start before it is <= x: doubling
// steps, then the search between the last two.  A block walks its tiles from left to right, so from one tile to the next this is a few
// loads near the last ones, not a search of all the record starts.
__device__ inline uint64_t starts_from(const uint64_t *offsets, uint64_t n_bytes, uint64_t n_records, uint64_t from, uint64_t x)
{
    uint64_t lo = from, hi = from, step = 1;
    while (hi <= n_records && start_of(offsets, n_bytes, hi) <= x) {
        lo = hi + 1;
        hi += step;
        step *= 2;
    }
    return starts_at_or_before(offsets, n_bytes, lo, hi <= n_records ? hi : n_records + 1, x);
}

// A tile of ML_TILE window ends from t0 on, with the w ends in front of it: slot i is end t0 - w + i.  Staged as (key, slot) pairs,
// doubled to ranges of Q = ml_top_q(w), every window taken as two of them; then the word of every end of the tile.  The ends in front of
// the chunk's base and the ends that are not valid make their windows not whole.
__global__ __launch_bounds__(ML_THREADS) void ml_select_kernel(TileArgs a)
{
    __shared__ uint64_t s_key[ML_SLOTS];
    __shared__ uint16_t s_pos[ML_SLOTS], s_win[ML_SLOTS];
    __shared__ uint32_t s_sum[ML_THREADS / 64];
    const uint32_t top = ml_top_q(a.w);
    auto range = [&](uint32_t i) { return MlPair{s_key[i], s_pos[i]}; };
    auto window = [&](uint32_t i) { return MlPair{0, s_win[i]}; };
    const uint64_t tiles = (a.limit - a.lo + ML_TILE - 1) / ML_TILE;
    for (uint64_t t = blockIdx.x; t < tiles; t += gridDim.x) {
        const uint64_t t0 = a.lo + t * ML_TILE;
        const uint32_t own = a.limit - t0 < ML_TILE ? (uint32_t)(a.limit - t0) : ML_TILE, n = a.w + own;
#pragma unroll
        for (uint32_t j = 0; j < ML_PER_THREAD; j++) {
            const uint32_t i = threadIdx.x + j * ML_THREADS;
            if (i >= n) continue;
            bool ok = t0 + i >= a.base + a.w;   // the end is at or behind the chunk's base
            const uint64_t at = ok ? t0 + i - a.w - a.base : 0;
            ok = ok && plane_bit(a.valid16[at >> 4], at);
            const MlPair p = ml_pair(ok ? ml_key(a.order, a.values[at]) : 0, i, ok);
            s_key[i] = p.key; s_pos[i] = (uint16_t)p.pos;
        }
        __syncthreads();
        for (uint32_t q = 1; q < top; q *= 2) {
            MlPair r[ML_PER_THREAD];
#pragma unroll
            for (uint32_t j = 0; j < ML_PER_THREAD; j++) {
                const uint32_t i = threadIdx.x + j * ML_THREADS;
                if (i < n) r[j] = ml_double_at(range, i, q);
            }
            __syncthreads();
#pragma unroll
            for (uint32_t j = 0; j < ML_PER_THREAD; j++) {
                const uint32_t i = threadIdx.x + j * ML_THREADS;
                if (i < n) { s_key[i] = r[j].key; s_pos[i] = (uint16_t)r[j].pos; }
            }
            __syncthreads();
        }
#pragma unroll
        for (uint32_t j = 0; j < ML_PER_THREAD; j++) {
            const uint32_t i = threadIdx.x + j * ML_THREADS;
            if (i < n && i + 1 >= a.w) s_win[i] = (uint16_t)ml_window_at(range, i, a.w, top).pos;
        }
        __syncthreads();
        uint32_t opens = 0, wholes = 0;
#pragma unroll
        for (uint32_t j = 0; j < ML_PER_THREAD; j++) {
            const uint32_t i = threadIdx.x + j * ML_THREADS;
            if (i >= n || i < a.w) continue;
            const uint32_t word = ml_sel_word(i, window(i - 1), window(i));
            const uint64_t x = t0 + i - a.w;
            a.sel[x - a.base] = (uint16_t)word;
            if (x < a.hi) { opens += (word & ML_SEL_OPEN) != 0; wholes += (word & ML_SEL_WHOLE) != 0; }
        }
        opens = block_sum_u32(opens, s_sum);
        __syncthreads();
        wholes = block_sum_u32(wholes, s_sum);
        if (threadIdx.x == 0) {
            a.count[t] = opens;
            if (wholes) add_agent(a.ctr + kCtrWindows, wholes);
        }
        __syncthreads();   // the LDS is free again
    }
}

// The entries of the tiles of [lo, hi), in ascending order of first window end: a tile's opening ends are ranked in rounds of a block
// (ballot inside a wave, the waves' totals through LDS) behind the entries of the tiles before it.  A block takes a run of consecutive
// tiles, so the record starts are walked along with them: an entry's record is searched among the starts that lie in its tile (found
// from those of the tile before, then a short search per entry).  A tile without an entry costs two loads.
__global__ __launch_bounds__(ML_THREADS) void ml_scatter_kernel(TileArgs a)
{
    __shared__ uint32_t s_wave[ML_THREADS / 64];
    const uint32_t lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    auto sel = [&](uint64_t x) { return (uint32_t)a.sel[x - a.base]; };
    const uint64_t tiles = (a.hi - a.lo + ML_TILE - 1) / ML_TILE;
    const uint64_t per = (tiles + gridDim.x - 1) / gridDim.x, t_begin = blockIdx.x * per, t_end = t_begin + per < tiles ? t_begin + per : tiles;
    uint64_t j_hi = 0;   // record starts known to lie at or before the tile at hand
    for (uint64_t t = t_begin; t < t_end; t++) {
        if (a.tile_base[t + 1] == a.tile_base[t]) continue;   // (the same for the whole block)
        const uint64_t t0 = a.lo + t * ML_TILE, t1 = a.hi - t0 < ML_TILE ? a.hi : t0 + ML_TILE;
        // the record starts at or before the tile's first end and its last: an entry's own lies between them
        const uint64_t j_lo = starts_from(a.offsets, a.n_bytes, a.n_records, j_hi, t0);
        j_hi = starts_from(a.offsets, a.n_bytes, a.n_records, j_lo, t1 - 1);
        uint64_t at = a.held + a.tile_base[t];
        for (uint64_t x0 = t0; x0 < t1; x0 += ML_THREADS) {
            const uint64_t x = x0 + threadIdx.x;
            const uint32_t word = x < t1 ? sel(x) : 0;
            const bool open = (word & ML_SEL_OPEN) != 0;
            const uint64_t mask = __ballot(open);
            if (lane == 0) s_wave[wave] = (uint32_t)__popcll(mask);
            __syncthreads();
            uint32_t before = 0, total = 0;
            for (uint32_t v = 0; v < ML_THREADS / 64; v++) {
                if (v < wave) before += s_wave[v];
                total += s_wave[v];
            }
            __syncthreads();   // the totals are free again
            if (open) {
                const uint64_t idx = at + before + (uint32_t)__popcll(mask & (((uint64_t)1 << lane) - 1));
                const uint64_t picked = x - (word & ML_SEL_DELTA), p = picked - a.base;
                const uint64_t j = starts_at_or_before(a.offsets, a.n_bytes, j_lo, j_hi, x);
                const uint64_t start = j ? start_of(a.offsets, a.n_bytes, j - 1) : 0;
                a.pos[idx] = picked - (a.k - 1) - start;
                a.value[idx] = a.values[p];
                a.info[idx] = ml_info(plane_bit(a.rc16[p >> 4], p), ml_span(sel, x, a.limit, a.w));
                a.end[idx] = x;
            }
            at += total;
        }
    }
}

// tile_base = the exclusive scan of the n counts (n: one chunk's tiles and one more, 65 538 at most): one block, ML_THREADS counts at a time
__global__ __launch_bounds__(ML_THREADS) void ml_scan_kernel(const uint32_t *count, uint32_t *tile_base, uint64_t n)
{
    __shared__ uint32_t s_wave[ML_THREADS / 64];
    const uint32_t lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    uint32_t running = 0;
    for (uint64_t i0 = 0; i0 < n; i0 += ML_THREADS) {
        const uint64_t i = i0 + threadIdx.x;
        const uint32_t own = i < n ? count[i] : 0;
        uint32_t v = own;   // the inclusive scan inside the wave
        for (int off = 1; off < 64; off <<= 1) {
            const uint32_t u = __shfl_up(v, off, 64);
            if ((int)lane >= off) v += u;
        }
        if (lane == 63) s_wave[wave] = v;
        __syncthreads();
        uint32_t before = 0, total = 0;
        for (uint32_t u = 0; u < ML_THREADS / 64; u++) {
            if (u < wave) before += s_wave[u];
            total += s_wave[u];
        }
        __syncthreads();   // the totals are free again
        if (i < n) tile_base[i] = running + before + v - own;
        running += total;
    }
}

// offsets_out[r], r <= n_records: the held entries whose first window end is below record start r
__global__ void ml_offsets_kernel(const uint64_t *offsets, uint64_t n_records, uint64_t n_bytes, const uint64_t *end, uint64_t n,
                                  uint64_t *offsets_out)
{
    const uint64_t r = (uint64_t)blockIdx.x * kThreads + threadIdx.x;
    if (r > n_records) return;
    const uint64_t target = start_of(offsets, n_bytes, r);
    uint64_t lo = 0, hi = n;
    while (lo < hi) {
        const uint64_t mid = lo + (hi - lo) / 2;
        if (end[mid] < target) lo = mid + 1; else hi = mid;
    }
    offsets_out[r] = lo;
}

}  // namespace

struct ntk_minimizer_list : Consumer {
    uint32_t w = 0, order = 0;
    Pinned<uint64_t> h_stage;                   // kCtrWords words
    MaterialiseScratch scratch;
    DeviceArray<uint64_t> d_pos, d_value;       // the held list ...
    DeviceArray<uint32_t> d_info;
    DeviceArray<uint64_t> d_offsets_out;        // ... and its n_records + 1 record ranges
    DeviceArray<uint64_t> d_end;                // the entries' first window ends
    DeviceArray<uint16_t> d_sel;                // the words of one chunk's window ends
    DeviceArray<uint32_t> d_count, d_tile_base; // one chunk's tiles, and one more
    DeviceArray<uint64_t> d_ctr;                // kCtrWords words
    uint64_t n_records = 0, n_entries = 0, n_windows = 0, n_chunks = 0;   // of the held result
    bool held = false;                          // a result is held (n_records may be 0)
    int failed = 0;                             // the status of a run that failed halfway

    uint64_t device_bytes() const
    {
        return scratch.device_bytes() + d_pos.bytes() + d_value.bytes() + d_info.bytes() + d_offsets_out.bytes() + d_end.bytes() + d_sel.bytes() +
               d_count.bytes() + d_tile_base.bytes() + d_ctr.bytes();
    }

    void release_all()
    {
        scratch.release();
        d_pos.release(); d_value.release(); d_info.release(); d_offsets_out.release(); d_end.release(); d_sel.release();
        d_count.release(); d_tile_base.release(); d_ctr.release();
    }
};

namespace {

using Handle = ntk_minimizer_list;

inline unsigned blocks_for(uint64_t n) { return (unsigned)((n + kThreads - 1) / kThreads); }

// the window ends a chunk is materialised beyond its own
inline uint64_t tail_of(const Chunk &c, uint64_t n_bytes, uint32_t w) { return n_bytes - c.end < w - 1 ? n_bytes - c.end : w - 1; }

// n_records empty ranges on the device
int hold_empty(Handle *m, uint64_t n_records)
{
    CT_HIPCHK(hipSetDevice(m->device));
    int rc = m->d_offsets_out.ensure(m->stream, n_records + 1, grow_half_again);
    if (rc) return rc;
    CT_HIPCHK(hipMemsetAsync(m->d_offsets_out.p, 0, (n_records + 1) * sizeof(uint64_t), m->stream));
    CT_HIPCHK(hipStreamSynchronize(m->stream));
    return NTK_OK;
}

// the whole run; a failure in here marks the handle
int run(Handle *m, const uint8_t *d_seq, const uint8_t *d_qual, uint64_t n_bytes, const uint64_t *d_offsets, uint64_t n_records,
        const ntk_params *p)
{
    int rc;
    hipStream_t st = m->stream;
    CT_HIPCHK(hipSetDevice(m->device));
    const uint32_t reach = m->k + m->w;   // the halo is that of a k-mer this long: k + w - 1 bytes at least
    const uint64_t bases = chunk_scratch_bases(n_bytes, reach) + (n_bytes > kChunkBases ? m->w - 1 : 0);
    const uint64_t tiles_max = (chunk_bases(n_bytes) + m->w - 1 + ML_TILE - 1) / ML_TILE;
    if ((rc = m->d_ctr.ensure(st, kCtrWords, grow_exact)) || (rc = m->d_offsets_out.ensure(st, n_records + 1, grow_half_again)) ||
        (rc = m->scratch.ensure(st, bases)) || (rc = m->d_sel.ensure(st, (bases + 15) & ~(uint64_t)15, grow_exact)) ||
        (rc = m->d_count.ensure(st, tiles_max + 1, grow_exact)) || (rc = m->d_tile_base.ensure(st, tiles_max + 1, grow_exact)))
        return rc;
    CT_HIPCHK(hipMemsetAsync(m->d_ctr.p, 0, kCtrWords * sizeof(uint64_t), st));
    const unsigned resident = (unsigned)m->n_cu * ML_BLOCKS_PER_CU;
    for (uint64_t start = 0; start < n_bytes; start += kChunkBases) {
        const Chunk c = chunk_at(n_bytes, reach, start);
        const uint64_t limit = c.end + tail_of(c, n_bytes, m->w);
        rc = ntk_materialize_device_quality(m->ctx, d_seq + c.base, d_qual ? d_qual + c.base : nullptr, limit - c.base, p,
                                            m->scratch.d_values.p, m->scratch.d_valid16.p, m->scratch.d_rc16.p);
        if (rc) return rc;
        CT_HIPCHK(hipSetDevice(m->device));
        m->n_chunks++;
        TileArgs a;
        a.values = m->scratch.d_values.p; a.valid16 = m->scratch.d_valid16.p; a.rc16 = m->scratch.d_rc16.p;
        a.base = c.base; a.lo = c.start; a.hi = c.end; a.limit = limit;
        a.k = m->k; a.w = m->w; a.order = m->order;
        a.sel = m->d_sel.p; a.count = m->d_count.p; a.ctr = m->d_ctr.p; a.tile_base = m->d_tile_base.p;
        a.offsets = d_offsets; a.n_records = n_records; a.n_bytes = n_bytes;
        const uint64_t tiles = (limit - c.start + ML_TILE - 1) / ML_TILE;
        CT_HIPCHK(hipMemsetAsync(m->d_count.p + tiles, 0, sizeof(uint32_t), st));   // the scan's last entry is the chunk's total
        hipLaunchKernelGGL(ml_select_kernel, dim3(grid_for(tiles, 1, resident)), dim3(ML_THREADS), 0, st, a);
        CT_HIPCHK(hipGetLastError());
        hipLaunchKernelGGL(ml_scan_kernel, dim3(1), dim3(ML_THREADS), 0, st, m->d_count.p, m->d_tile_base.p, tiles + 1);
        CT_HIPCHK(hipGetLastError());
        CT_HIPCHK(hipMemcpyAsync(m->h_stage.p, m->d_tile_base.p + tiles, sizeof(uint32_t), hipMemcpyDeviceToHost, st));
        CT_HIPCHK(hipStreamSynchronize(st));
        const uint64_t fresh = *(const uint32_t *)m->h_stage.p, need = m->n_entries + fresh;
        if (fresh == 0) continue;
        if ((rc = m->d_pos.ensure(st, need, grow_half_again, m->n_entries)) || (rc = m->d_value.ensure(st, need, grow_half_again, m->n_entries)) ||
            (rc = m->d_info.ensure(st, need, grow_half_again, m->n_entries)) || (rc = m->d_end.ensure(st, need, grow_half_again, m->n_entries)))
            return rc;
        a.held = m->n_entries;
        a.pos = m->d_pos.p; a.value = m->d_value.p; a.info = m->d_info.p; a.end = m->d_end.p;
        const uint64_t own_tiles = (c.end - c.start + ML_TILE - 1) / ML_TILE;
        hipLaunchKernelGGL(ml_scatter_kernel, dim3(grid_for(own_tiles, 1, resident)), dim3(ML_THREADS), 0, st, a);
        CT_HIPCHK(hipGetLastError());
        m->n_entries = need;
    }
    hipLaunchKernelGGL(ml_offsets_kernel, dim3(blocks_for(n_records + 1)), dim3(kThreads), 0, st, d_offsets, n_records, n_bytes, m->d_end.p,
                       m->n_entries, m->d_offsets_out.p);
    CT_HIPCHK(hipGetLastError());
    if ((rc = m->h_stage.read(st, m->d_ctr.p, kCtrWords))) return rc;
    m->n_windows = m->h_stage.p[kCtrWindows];
    return NTK_OK;
}

}  // namespace

extern "C" {

int ntk_minimizer_list_create(ntk_ctx *ctx, uint32_t k, uint32_t path, uint32_t w, uint32_t order, ntk_minimizer_list **out)
{
    if (!ctx || !out) return NTK_ERR_BAD_ARG;
    *out = nullptr;
    if (k < 1 || k > 32) return NTK_ERR_BAD_K;
    if (path > NTK_PATH_BITS_CANONICAL || w < 1 || w > NTK_MINIMIZER_LIST_W_MAX || order > NTK_MINIMIZER_LIST_HASH) return NTK_ERR_BAD_ARG;
    ntk_minimizer_list *m = new (std::nothrow) ntk_minimizer_list();
    if (!m) return NTK_ERR_NOMEM;
    int rc = m->bind(ctx, k, path);
    if (rc) { delete m; return rc; }
    m->w = w; m->order = order;
    if ((rc = m->h_stage.alloc(kCtrWords))) { delete m; return rc; }
    *out = m;
    return NTK_OK;
}

int ntk_minimizer_list_trim(ntk_minimizer_list *m)
{
    if (!m) return NTK_ERR_BAD_ARG;
    CT_HIPCHK(hipSetDevice(m->device));
    CT_HIPCHK(hipStreamSynchronize(m->stream));
    m->release_all();
    (void)hipGetLastError();
    m->held = false;
    m->n_records = m->n_entries = m->n_windows = m->n_chunks = 0;
    m->failed = 0;
    return NTK_OK;
}

void ntk_minimizer_list_destroy(ntk_minimizer_list *m)
{
    if (!m) return;
    (void)ntk_minimizer_list_trim(m);
    m->h_stage.release();
    (void)hipGetLastError();
    delete m;
}

int ntk_minimizer_list_run_device(ntk_minimizer_list *m, const uint8_t *d_seq, const uint8_t *d_qual, uint64_t n_bytes,
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
    m->held = true; m->failed = 0;
    m->n_records = n_records;
    m->n_entries = m->n_windows = m->n_chunks = 0;
    rc = empty ? hold_empty(m, n_records) : run(m, d_seq, d_qual, n_bytes, d_offsets, n_records, p);
    if (rc) m->failed = rc;
    return rc;
}

int ntk_minimizer_list_read(ntk_minimizer_list *m, uint64_t *offsets, uint64_t *pos, uint64_t *values, uint32_t *info, uint64_t cap,
                            uint64_t *n)
{
    if (!m || !n || (cap && (!pos || !values || !info))) return NTK_ERR_BAD_ARG;
    if (m->failed) return m->failed;
    *n = m->held ? m->n_entries : 0;
    if (!m->held) return NTK_OK;
    if (m->n_entries > cap) return NTK_ERR_CAPACITY;
    if (!offsets) return NTK_OK;   // the size alone
    CT_HIPCHK(hipSetDevice(m->device));
    CT_HIPCHK(hipMemcpyAsync(offsets, m->d_offsets_out.p, (m->n_records + 1) * sizeof(uint64_t), hipMemcpyDeviceToHost, m->stream));
    if (m->n_entries) {
        CT_HIPCHK(hipMemcpyAsync(pos, m->d_pos.p, m->n_entries * sizeof(uint64_t), hipMemcpyDeviceToHost, m->stream));
        CT_HIPCHK(hipMemcpyAsync(values, m->d_value.p, m->n_entries * sizeof(uint64_t), hipMemcpyDeviceToHost, m->stream));
        CT_HIPCHK(hipMemcpyAsync(info, m->d_info.p, m->n_entries * sizeof(uint32_t), hipMemcpyDeviceToHost, m->stream));
    }
    CT_HIPCHK(hipStreamSynchronize(m->stream));
    return NTK_OK;
}

int ntk_minimizer_list_result_device(ntk_minimizer_list *m, const uint64_t **d_offsets, const uint64_t **d_pos, const uint64_t **d_values,
                                     const uint32_t **d_info, uint64_t *n)
{
    if (!m || !d_offsets || !d_pos || !d_values || !d_info || !n) return NTK_ERR_BAD_ARG;
    if (m->failed) return m->failed;
    const bool any = m->held && m->n_entries;
    *d_offsets = m->held ? m->d_offsets_out.p : nullptr;
    *d_pos = any ? m->d_pos.p : nullptr;
    *d_values = any ? m->d_value.p : nullptr;
    *d_info = any ? m->d_info.p : nullptr;
    *n = m->held ? m->n_entries : 0;
    return NTK_OK;
}

int ntk_minimizer_list_stats(ntk_minimizer_list *m, struct ntk_minimizer_list_stats *out)
{
    if (!m || !out) return NTK_ERR_BAD_ARG;
    if (m->failed) return m->failed;
    CT_HIPCHK(hipSetDevice(m->device));
    CT_HIPCHK(hipStreamSynchronize(m->stream));
    out->n_records = m->held ? m->n_records : 0;
    out->n_entries = m->held ? m->n_entries : 0;
    out->n_windows = m->held ? m->n_windows : 0;
    out->n_chunks = m->n_chunks;
    out->device_bytes = m->device_bytes();
    out->k = m->k; out->path = m->path; out->w = m->w; out->order = m->order;
    return NTK_OK;
}

}  // extern "C"
