// HyperLogLog sketch of the distinct k-mers of device batches (include/needletail_amd_sketch.h): the first pass that sizes a count
// table.  A consumer of the core's public ABI like the two tables, with their two routes: k <= 32 reads the values
// ntk_materialize_device_quality emits (every path's keys are the core's by construction), k = 33..63 walks the batch bytes as the
// wide table's count kernel does (walk_lane_run of ntk_wide_walk.hpp).
//
// THE ONE PLACE that fixes hash, index and rank is sketch_slot / sketch_rank below (fmix64 is ntk_consumer.hpp's, the tables'
// hash); the header states them and tests/_sketch_model.py restates them.
//
// Update scheme: after the first few hundred thousand keys almost no key raises a register (a register holds about log2(n / m)), so
// the common case must cost no atomic.  Each block keeps private registers in LDS (m 32-bit cells, 64 KiB: two blocks per CU), reads
// the cell first and issues the LDS atomic max only for a larger rank; at its end it reads each global register and issues the
// agent-scope atomic max only where its own value is larger.  Registers only grow, so a stale read costs a redundant atomic, never a
// wrong result.  The grid is two blocks per CU with a grid-stride loop: the flush is paid per resident block, not per unit of work.
// DESIGN.md section 12.
#include "../../include/needletail_amd_sketch.h"
#include "ntk_consumer.hpp"
#include "ntk_wide_walk.hpp"

#include <cmath>
#include <cstring>
#include <new>

namespace {

constexpr uint32_t kP = NTK_SKETCH_P, kRegisters = NTK_SKETCH_REGISTERS;
constexpr uint32_t kRankMax = 64 - kP + 1;               // 51: every one of the 50 bits below the index is zero
constexpr uint64_t kXor = 0x9E3779B97F4A7C15ull;         // C: key 0 (AAA...A) must not hash to 0
constexpr int kSketchThreads = 1024;                     // 16 waves per block: two blocks (2 x 64 KiB of LDS) keep 8 waves per SIMD
constexpr uint32_t kPerLane = 4;                         // window ends per lane and round of sk_update_kernel (loads in flight)

static_assert(kRankMax == NTK_SKETCH_MAX_RANK && kXor == NTK_SKETCH_XOR, "the header states the sketch's constants");
static_assert(kRegisters % kSketchThreads == 0, "the clear and the flush walk the registers in whole rounds");

__host__ __device__ inline uint64_t sketch_hash(uint64_t key) { return fmix64(key ^ kXor); }
__host__ __device__ inline uint64_t sketch_hash(uint64_t hi, uint64_t lo) { return fmix64(lo ^ fmix64(hi) ^ kXor); }
// register index: the top kP bits
__host__ __device__ inline uint32_t sketch_slot(uint64_t h) { return (uint32_t)(h >> (64 - kP)); }
// rank: 1 + the leading zeros of the 50 bits below the index; the sentinel bit under them caps it at kRankMax
__host__ __device__ inline uint32_t sketch_rank(uint64_t h) { return (uint32_t)__builtin_clzll((h << kP) | ((uint64_t)1 << (kP - 1))) + 1; }

// one key into the block's registers: the plain read first, the LDS atomic only for a larger rank
__device__ inline void note(uint32_t *cells, uint64_t h)
{
    const uint32_t j = sketch_slot(h), r = sketch_rank(h);
    if (cells[j] < r) atomicMax(&cells[j], r);
}

__device__ inline void clear_cells(uint32_t *cells)
{
    for (uint32_t j = threadIdx.x; j < kRegisters; j += kSketchThreads) cells[j] = 0;
    __syncthreads();
}

// the block's registers into the global ones, then the block's window count (one add per wave)
__device__ inline void flush(const uint32_t *cells, uint32_t *regs, uint64_t windows, uint64_t *n_windows)
{
    __syncthreads();
    for (uint32_t j = threadIdx.x; j < kRegisters; j += kSketchThreads) {
        const uint32_t v = cells[j];
        if (v && regs[j] < v) (void)__hip_atomic_fetch_max(&regs[j], v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    }
    windows = wave_sum(windows);
    if ((threadIdx.x & 63) == 0 && windows) add_agent(n_windows, windows);
}

struct UpdateArgs {
    const uint64_t *values;    // materialised values, indexed by window end
    const uint16_t *valid16;   // bit (15 - e % 16) of word e / 16: window e is emitted
    uint64_t first, n;         // windows ending in [first, n) are taken (first: the chunk's halo)
    uint32_t *regs;
    uint64_t *n_windows;
};

// k <= 32.  Grid-stride over window ends, kPerLane ends per lane and round (each a coalesced 8-byte load across the wave, issued
// before any is used) with the valid plane's bit.  Every lane runs the same number of rounds.
__global__ __launch_bounds__(kSketchThreads) void sk_update_kernel(UpdateArgs a)
{
    __shared__ uint32_t cells[kRegisters];
    clear_cells(cells);
    uint64_t windows = 0;
    const uint64_t step = (uint64_t)gridDim.x * kSketchThreads, span = a.n - a.first;
    const uint64_t rounds = (span + step * kPerLane - 1) / (step * kPerLane);
    uint64_t i = (uint64_t)blockIdx.x * kSketchThreads + threadIdx.x;
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
            if (!take[u]) continue;
            note(cells, sketch_hash(key[u]));
            windows++;
        }
    }
    flush(cells, a.regs, windows, a.n_windows);
}

struct WideArgs {
    const uint8_t *seq, *qual;   // qual: nullptr = no mask
    uint64_t n_bytes;            // windows ending in [0, n_bytes) are taken; no byte at or past it is a base
    uint32_t k, cutoff;
    uint32_t *regs;
    uint64_t *n_windows;
};

// k = 33..63.  Lane r (grid-stride) owns the window ends [r * kLaneRun, (r + 1) * kLaneRun) and walks them as wt_count_kernel does
// (walk_lane_run); 64-bit offsets, no chunking, no scratch.
__global__ __launch_bounds__(kSketchThreads) void sk_wide_update_kernel(WideArgs a)
{
    __shared__ uint32_t cells[kRegisters];
    clear_cells(cells);
    uint64_t windows = 0;
    const uint64_t n_runs = (a.n_bytes + kLaneRun - 1) / kLaneRun, stride = (uint64_t)gridDim.x * kSketchThreads;
    for (uint64_t r = (uint64_t)blockIdx.x * kSketchThreads + threadIdx.x; r < n_runs; r += stride)
        walk_lane_run<kLaneRun, kPrime>(a.seq, a.qual, a.n_bytes, a.k, a.cutoff, r * kLaneRun, [&](uint64_t hi, uint64_t lo) __attribute__((always_inline)) {
            note(cells, sketch_hash(hi, lo));
            windows++;
        });
    flush(cells, a.regs, windows, a.n_windows);
}

// The estimator and the capacity rule of the header, from the register histogram c[0..kRankMax] alone.
void evaluate(const uint64_t *c, uint64_t n_windows, uint32_t k, struct ntk_kmer_sketch_estimate *out)
{
    const double m = (double)kRegisters;
    double z = 0.0;
    for (int r = (int)kRankMax; r >= 0; r--) z += std::ldexp((double)c[r], -r);   // every term exact; this order is the definition
    double e = 0.7213 / (1.0 + 1.079 / m) * m * m / z;
    if (e <= 2.5 * m && c[0]) e = m * std::log(m / (double)c[0]);
    const double want = std::ceil(e * (1.0 + 5.0 * 1.04 / std::sqrt(m)));
    uint64_t cap = want < 0x1p63 ? (uint64_t)want + 8 : ~(uint64_t)0;   // (registers merged in by hand can say more than a word holds)
    if (cap > n_windows) cap = n_windows;
    if (k < 32 && cap > ((uint64_t)1 << (2 * k))) cap = (uint64_t)1 << (2 * k);
    if (cap < 1) cap = 1;
    out->distinct = e;
    out->n_windows = n_windows;
    out->capacity = cap;
    out->zero_registers = (uint32_t)c[0];
}

}  // namespace

struct ntk_kmer_sketch : Consumer {
    DeviceArray<uint32_t> d_regs;     // the registers as the kernels keep them: one 32-bit word each
    DeviceArray<uint64_t> d_windows;  // k-mers added by add_device since reset
    uint64_t merged_windows = 0;      // k-mers of the sketches merged in since reset
    Pinned<uint32_t> h_stage;         // kRegisters words, then the window count (two words)
    MaterialiseScratch scratch;       // k <= 32 only
};

namespace {

// the registers and the device window count on the host (synchronises)
int read_back(ntk_kmer_sketch *s, uint64_t *windows)
{
    CT_HIPCHK(hipSetDevice(s->device));
    CT_HIPCHK(hipMemcpyAsync(s->h_stage.p + kRegisters, s->d_windows.p, sizeof(uint64_t), hipMemcpyDeviceToHost, s->stream));
    const int rc = s->h_stage.read(s->stream, s->d_regs.p, kRegisters);
    if (!rc && windows) memcpy(windows, s->h_stage.p + kRegisters, sizeof(uint64_t));
    return rc;
}

}  // namespace

extern "C" {

int ntk_kmer_sketch_create(ntk_ctx *ctx, uint32_t k, uint32_t path, ntk_kmer_sketch **out)
{
    if (!ctx || !out) return NTK_ERR_BAD_ARG;
    *out = nullptr;
    if (k < 1 || k > kKMax) return NTK_ERR_BAD_K;
    if (path > NTK_PATH_BITS_CANONICAL) return NTK_ERR_BAD_ARG;
    if (k > 32 && path != NTK_PATH_BYTES_CANONICAL) return NTK_ERR_BAD_K;   // the 2-bit iterator stops at k = 32
    ntk_kmer_sketch *s = new (std::nothrow) ntk_kmer_sketch();
    if (!s) return NTK_ERR_NOMEM;
    int rc = s->bind(ctx, k, path);
    if (rc) { delete s; return rc; }
    if ((rc = s->d_regs.ensure(s->stream, kRegisters, grow_exact)) || (rc = s->d_windows.ensure(s->stream, 1, grow_exact)) ||
        (rc = s->h_stage.alloc(kRegisters + 2)) || (rc = ntk_kmer_sketch_reset(s))) {
        ntk_kmer_sketch_destroy(s);
        return rc;
    }
    *out = s;
    return NTK_OK;
}

void ntk_kmer_sketch_destroy(ntk_kmer_sketch *s)
{
    if (!s) return;
    (void)hipSetDevice(s->device);
    (void)hipStreamSynchronize(s->stream);
    s->scratch.release();
    s->d_regs.release(); s->d_windows.release();
    s->h_stage.release();
    (void)hipGetLastError();
    delete s;
}

int ntk_kmer_sketch_reset(ntk_kmer_sketch *s)
{
    if (!s) return NTK_ERR_BAD_ARG;
    CT_HIPCHK(hipSetDevice(s->device));
    CT_HIPCHK(hipMemsetAsync(s->d_regs.p, 0, kRegisters * sizeof(uint32_t), s->stream));
    CT_HIPCHK(hipMemsetAsync(s->d_windows.p, 0, sizeof(uint64_t), s->stream));
    s->merged_windows = 0;
    return NTK_OK;
}

int ntk_kmer_sketch_add_device(ntk_kmer_sketch *s, const uint8_t *d_seq, const uint8_t *d_qual, uint64_t n_bytes, const ntk_params *p)
{
    int rc = check_batch_params(s, p);
    if (rc || n_bytes == 0) return rc;
    if ((rc = check_batch_pointers(d_seq, d_qual))) return rc;
    CT_HIPCHK(hipSetDevice(s->device));
    const unsigned resident = (unsigned)s->n_cu * 2;
    if (s->k > 32) {
        WideArgs a;
        a.seq = d_seq; a.n_bytes = n_bytes; a.k = s->k;
        set_quality(a, p, d_qual);
        a.regs = s->d_regs.p; a.n_windows = s->d_windows.p;
        const uint64_t runs = (n_bytes + kLaneRun - 1) / kLaneRun;
        hipLaunchKernelGGL(sk_wide_update_kernel, dim3(grid_for(runs, kSketchThreads, resident)), dim3(kSketchThreads), 0, s->stream, a);
        CT_HIPCHK(hipGetLastError());
        return NTK_OK;
    }
    // of every chunk only the windows ending at or after its start are taken - the max would not mind a window twice, n_windows does
    return for_each_chunk(*s, s->scratch, d_seq, d_qual, n_bytes, p, [&](const Chunk &c) -> int {
        UpdateArgs a;
        a.values = s->scratch.d_values.p; a.valid16 = s->scratch.d_valid16.p;
        a.first = c.skip(); a.n = c.len();
        a.regs = s->d_regs.p; a.n_windows = s->d_windows.p;
        const uint64_t rounds = (a.n - a.first + kPerLane - 1) / kPerLane;
        hipLaunchKernelGGL(sk_update_kernel, dim3(grid_for(rounds, kSketchThreads, resident)), dim3(kSketchThreads), 0, s->stream, a);
        CT_HIPCHK(hipGetLastError());
        return NTK_OK;
    });
}

int ntk_kmer_sketch_registers(ntk_kmer_sketch *s, uint8_t *regs)
{
    if (!s || !regs) return NTK_ERR_BAD_ARG;
    int rc = read_back(s, nullptr);
    if (rc) return rc;
    for (uint32_t j = 0; j < kRegisters; j++) regs[j] = (uint8_t)s->h_stage.p[j];
    return NTK_OK;
}

int ntk_kmer_sketch_merge(ntk_kmer_sketch *s, const uint8_t *regs, uint64_t n_windows)
{
    if (!s || !regs) return NTK_ERR_BAD_ARG;
    for (uint32_t j = 0; j < kRegisters; j++)
        if (regs[j] > kRankMax) return NTK_ERR_BAD_ARG;
    int rc = read_back(s, nullptr);
    if (rc) return rc;
    for (uint32_t j = 0; j < kRegisters; j++)
        if (regs[j] > s->h_stage.p[j]) s->h_stage.p[j] = regs[j];
    if ((rc = s->h_stage.write(s->stream, s->d_regs.p, kRegisters))) return rc;
    s->merged_windows += n_windows;
    return NTK_OK;
}

int ntk_kmer_sketch_estimate(ntk_kmer_sketch *s, struct ntk_kmer_sketch_estimate *out)
{
    if (!s || !out) return NTK_ERR_BAD_ARG;
    uint64_t windows = 0, c[kRankMax + 1] = {};
    int rc = read_back(s, &windows);
    if (rc) return rc;
    for (uint32_t j = 0; j < kRegisters; j++) c[s->h_stage.p[j] <= kRankMax ? s->h_stage.p[j] : kRankMax]++;
    evaluate(c, windows + s->merged_windows, s->k, out);
    out->k = s->k; out->path = s->path;
    return NTK_OK;
}

}  // extern "C"
