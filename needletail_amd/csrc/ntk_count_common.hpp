// What the two count tables share (ntk_count.hip: k <= 32, one key word; ntk_wide_count.hip: k = 33..63, two key words) on top of what
// every consumer of the core's ABI does (ntk_consumer.hpp): the constants, the extract count / scan and spectrum kernels, and TableCore,
// the host side of a table apart from its key words.  The read-side kernels see a table as its occupancy words (`occ`: the narrow
// keys, the wide hi; EMPTY = free) and its counts.  Everything is in an anonymous namespace, so each library keeps a private copy and
// exports nothing new.  DESIGN.md sections 10 and 11.
#pragma once

#include "ntk_consumer.hpp"

#include <cstring>
#include <initializer_list>

namespace {

constexpr uint64_t kEmpty = ~(uint64_t)0;
constexpr uint32_t kProbeMax = 4096;                     // probe bound: a full or adversarial table never makes a kernel run long
constexpr uint32_t kExtractPerThread = 32;               // slots per thread of the extract count / scatter kernels
constexpr uint64_t kExtractPerBlock = (uint64_t)kThreads * kExtractPerThread;
constexpr uint32_t kMaxBins = 16384;
// stats words on the device that both tables keep
constexpr int kStDistinct = 0, kStTotal = 1, kStDropped = 2;

// extract, step 1: occupied slots with count >= min_count, per block of kExtractPerBlock slots
__global__ __launch_bounds__(kThreads) void ct_extract_count_kernel(const uint64_t *occ, const uint64_t *counts, uint64_t slots,
                                                                    uint64_t min_count, uint32_t *block_counts)
{
    __shared__ uint32_t lds[kThreads / 64];
    const uint64_t base = (uint64_t)blockIdx.x * kExtractPerBlock;
    uint32_t c = 0;
    for (uint32_t j = 0; j < kExtractPerThread; j++) {
        const uint64_t s = base + (uint64_t)j * kThreads + threadIdx.x;
        if (s < slots && occ[s] != kEmpty && counts[s] >= min_count) c++;
    }
    c = block_sum_u32(c, lds);
    if (threadIdx.x == 0) block_counts[blockIdx.x] = c;
}

// extract, step 2: exclusive scan of the block counts (one block); offsets[nb] = the total
__global__ __launch_bounds__(1024) void ct_extract_scan_kernel(const uint32_t *block_counts, uint32_t nb, uint64_t *offsets)
{
    __shared__ uint64_t part[1024];
    const uint32_t per = (nb + 1023) / 1024, lo = threadIdx.x * per, hi = lo + per < nb ? lo + per : nb;
    uint64_t s = 0;
    for (uint32_t b = lo; b < hi; b++) s += block_counts[b];
    part[threadIdx.x] = s;
    __syncthreads();
    for (int off = 1; off < 1024; off <<= 1) {   // Hillis-Steele inclusive scan of the 1024 partial sums
        const uint64_t v = threadIdx.x >= (unsigned)off ? part[threadIdx.x - off] : 0;
        __syncthreads();
        part[threadIdx.x] += v;
        __syncthreads();
    }
    uint64_t run = part[threadIdx.x] - s;
    for (uint32_t b = lo; b < hi; b++) { offsets[b] = run; run += block_counts[b]; }
    if (threadIdx.x == 1023) offsets[nb] = part[1023];
}

// spectrum: a block-private LDS histogram over a grid-stride share of the slots, then one atomic per non-zero bin per block
__global__ __launch_bounds__(kThreads) void ct_spectrum_kernel(const uint64_t *occ, const uint64_t *counts, uint64_t slots,
                                                               uint32_t n_bins, uint64_t *hist)
{
    extern __shared__ uint32_t bins[];
    for (uint32_t b = threadIdx.x; b < n_bins; b += blockDim.x) bins[b] = 0;
    __syncthreads();
    const uint64_t stride = (uint64_t)gridDim.x * blockDim.x;
    for (uint64_t s = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; s < slots; s += stride) {
        if (occ[s] == kEmpty) continue;
        const uint64_t c = counts[s];
        atomicAdd(&bins[c < n_bins - 1 ? (uint32_t)c : n_bins - 1], 1u);
    }
    __syncthreads();
    for (uint32_t b = threadIdx.x; b < n_bins; b += blockDim.x)
        if (bins[b]) add_agent(hist + b, bins[b]);
}

// The host side of a table apart from its key words, which the table adds (keys; hi, lo) and hands to the helpers that set up, clear
// or free every slot array.  `stat_words`: the length of the table's stats array.
struct TableCore : Consumer {
    using KeyWords = std::initializer_list<DeviceArray<uint64_t> *>;
    uint32_t probe_max = kProbeMax;
    uint64_t slots = 0;
    DeviceArray<uint64_t> d_counts, d_stats, d_hist, d_offsets;
    DeviceArray<uint32_t> d_block_counts;
    Pinned<uint64_t> h_stage;   // stats and spectrum read-backs

    uint64_t extract_blocks() const { return (slots + kExtractPerBlock - 1) / kExtractPerBlock; }

    // the context's device and stream, the table's size and probe bound; no allocation yet
    int init(ntk_ctx *c, uint32_t k_, uint32_t path_, uint64_t capacity)
    {
        slots = 2;
        while (capacity * 4 > slots * 3) slots <<= 1;   // capacity <= 0.75 * slots
        probe_max = slots < kProbeMax ? (uint32_t)slots : kProbeMax;
        return bind(c, k_, path_);
    }

    // the key words (one u64 per slot each), then the counts and the buffers of stats, extract and spectrum
    int alloc(KeyWords key_words, int stat_words)
    {
        int rc = NTK_OK;
        for (DeviceArray<uint64_t> *w : key_words)
            if ((rc = w->ensure(stream, slots, grow_exact))) return rc;
        const uint64_t nb = extract_blocks();
        if ((rc = d_counts.ensure(stream, slots, grow_exact)) || (rc = d_stats.ensure(stream, stat_words, grow_exact)) ||
            (rc = d_hist.ensure(stream, kMaxBins, grow_exact)) || (rc = d_offsets.ensure(stream, nb + 1, grow_exact)) ||
            (rc = d_block_counts.ensure(stream, nb, grow_exact)))
            return rc;
        return h_stage.alloc(kMaxBins);
    }

    // queued: every key word EMPTY, the counts and stats 0
    int reset(KeyWords key_words, int stat_words)
    {
        CT_HIPCHK(hipSetDevice(device));
        for (DeviceArray<uint64_t> *w : key_words) CT_HIPCHK(hipMemsetAsync(w->p, 0xFF, slots * sizeof(uint64_t), stream));
        CT_HIPCHK(hipMemsetAsync(d_counts.p, 0, slots * sizeof(uint64_t), stream));
        CT_HIPCHK(hipMemsetAsync(d_stats.p, 0, stat_words * sizeof(uint64_t), stream));
        return NTK_OK;
    }

    // once the stream is idle: the table's key words, then the core's buffers; errors are dropped
    void release(KeyWords key_words)
    {
        (void)hipSetDevice(device);
        (void)hipStreamSynchronize(stream);
        for (DeviceArray<uint64_t> *w : key_words) w->release();
        d_counts.release(); d_stats.release(); d_hist.release(); d_offsets.release(); d_block_counts.release();
        h_stage.release();
        (void)hipGetLastError();
    }

    // stats words on the host (synchronises)
    int read_stats(uint64_t *w, int stat_words)
    {
        CT_HIPCHK(hipSetDevice(device));
        const int rc = h_stage.read(stream, d_stats.p, stat_words);
        if (!rc) memcpy(w, h_stage.p, stat_words * sizeof(uint64_t));
        return rc;
    }

    // read_stats for the read side, which refuses an incomplete table: NTK_ERR_CAPACITY once anything was dropped
    int read_complete(uint64_t *w, int stat_words)
    {
        const int rc = read_stats(w, stat_words);
        return rc ? rc : w[kStDropped] ? NTK_ERR_CAPACITY : NTK_OK;
    }

    // extract, steps 1 and 2: block counts and offsets of the occupied slots with count >= min_count; *total = their number
    // (synchronises)
    int extract_offsets(const uint64_t *occ, uint64_t min_count, uint64_t *total)
    {
        const uint64_t nb = extract_blocks();
        hipLaunchKernelGGL(ct_extract_count_kernel, dim3((unsigned)nb), dim3(kThreads), 0, stream, occ, d_counts.p, slots, min_count,
                           d_block_counts.p);
        CT_HIPCHK(hipGetLastError());
        hipLaunchKernelGGL(ct_extract_scan_kernel, dim3(1), dim3(1024), 0, stream, d_block_counts.p, (uint32_t)nb, d_offsets.p);
        CT_HIPCHK(hipGetLastError());
        const int rc = h_stage.read(stream, d_offsets.p + nb, 1);
        if (!rc) *total = h_stage.p[0];
        return rc;
    }

    // extract, step 3 and the sort, on n > 0 pairs in arrays allocated for the call: scatter(tk, tc) queues the table's scatter
    // kernel into them, sort(tmp, tmp_bytes, tk, tc) its rocprim::radix_sort_pairs into the caller's arrays (tmp = nullptr: the size
    // query).  Synchronises, then frees the arrays: a table is large, and this memory goes back at once.
    template <class Key, class Scatter, class Sort>
    int scatter_sort(uint64_t n, Scatter scatter, Sort sort)
    {
        DeviceArray<Key> tk;
        DeviceArray<uint64_t> tc;
        DeviceArray<char> tmp;
        int rc = tk.ensure(stream, n, grow_exact);
        if (!rc) rc = tc.ensure(stream, n, grow_exact);
        if (!rc) {
            scatter(tk.p, tc.p);
            if (hipGetLastError() != hipSuccess) rc = NTK_ERR_HIP;
        }
        if (!rc) rc = with_tmp(tmp, stream, grow_exact, [&](void *t, size_t &t_bytes) { return sort(t, t_bytes, tk.p, tc.p); });
        if (hipStreamSynchronize(stream) != hipSuccess) {
            (void)hipGetLastError();
            if (!rc) rc = NTK_ERR_HIP;
        }
        tk.release(); tc.release(); tmp.release();
        return rc;
    }

    // the spectrum of the occupied slots into hist[0, n_bins) (synchronises)
    int spectrum(const uint64_t *occ, uint64_t *hist, uint32_t n_bins)
    {
        CT_HIPCHK(hipMemsetAsync(d_hist.p, 0, n_bins * sizeof(uint64_t), stream));
        hipLaunchKernelGGL(ct_spectrum_kernel, dim3(grid_for(slots, kThreads, (unsigned)n_cu * 2)), dim3(kThreads),
                           n_bins * sizeof(uint32_t), stream, occ, d_counts.p, slots, n_bins, d_hist.p);
        CT_HIPCHK(hipGetLastError());
        const int rc = h_stage.read(stream, d_hist.p, n_bins);
        if (!rc) memcpy(hist, h_stage.p, n_bins * sizeof(uint64_t));
        return rc;
    }
};

}  // namespace
