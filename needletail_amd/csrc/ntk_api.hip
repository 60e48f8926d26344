// ntk_api.hip — host side of the C ABI declared in include/needletail_amd.h.
// Everything that computes launches HIP kernels (ntk_kernels.hpp); there is no CPU fallback.
#include "../../include/needletail_amd.h"

#include <hip/hip_runtime.h>
#include <rccl/rccl.h>   // types and prototypes only: the library is loaded at run time (load_rccl)
#include <dlfcn.h>
#include <time.h>

#include <cstdlib>
#include <cstring>
#include <map>
#include <mutex>
#include <new>
#include <utility>
#include <thread>
#include <algorithm>
#include <vector>

#include "ntk_kernels.hpp"
#include "ntk_plan.hpp"
#include "ntk_compat_plan.hpp"

using namespace ntk;

// the sv2 builds (ntk_scan2.hip): nullptr when (k, flags) has none
const void *ntk_pick_scan2(int k, bool tie_rc, bool accept_u);
const void *ntk_pick_scan2_q(int k, bool canonical, bool tie_rc, bool accept_u);
const void *ntk_pick_scan2_min_a(int k, int w, bool tie_rc, bool accept_u, bool quality);   // ntk_scan2_min.o: k = 15..18
const void *ntk_pick_scan2_min_b(int k, int w, bool tie_rc, bool accept_u, bool quality);   // ntk_scan2_min2.o: k = 19..22
const void *ntk_pick_scan2_fwd(int k, bool accept_u);

namespace {

thread_local int g_last_hip = 0;
thread_local int g_last_rccl = 0;

// HIP caps gridDim.x * blockDim.x below 2^32 and silently wraps beyond it: element-wise kernels are grid-stride and are
// launched with at most 2^20 blocks.
inline unsigned grid_for(uint64_t items, unsigned block) { const uint64_t b = (items + block - 1) / block; return (unsigned)(b > (1u << 20) ? (1u << 20) : (b ? b : 1)); }

#define HIPCHK(expr)                                     \
    do {                                                 \
        hipError_t e__ = (expr);                         \
        if (e__ != hipSuccess) {                         \
            g_last_hip = (int)e__;                       \
            (void)hipGetLastError();                     \
            return NTK_ERR_HIP;                          \
        }                                                \
    } while (0)

}  // namespace

// how the core owns device and pinned memory: the shared layer, with the core's check and status - every failed HIP call, out of memory
// included, is recorded for ntk_last_hip_error and answered NTK_ERR_HIP
#define CT_HIPCHK HIPCHK
#include "ntk_device_mem.hpp"

namespace {

int alloc_status(hipError_t e) { HIPCHK(e); return NTK_OK; }   // (only ever called with a failure)

constexpr uint32_t kLutChanged = 0x100, kLutDeleted = 0x200;

// Byte maps, restated from the reference's match arms.
// normalize: reference src/sequence.rs:24-51 (priority order matters only for overlapping arms; none overlap).
void build_normalize_lut(uint16_t *lut, bool iupac)
{
    for (int c = 0; c < 256; c++) {
        uint32_t v;
        switch (c) {
        case 'A': case 'C': case 'G': case 'T': case 'N': case '-': v = (uint32_t)c; break;
        case 'a': v = 'A' | kLutChanged; break;
        case 'c': v = 'C' | kLutChanged; break;
        case 'g': v = 'G' | kLutChanged; break;
        case 't': case 'u': case 'U': v = 'T' | kLutChanged; break;
        case '.': case '~': v = '-' | kLutChanged; break;
        case 'B': case 'D': case 'H': case 'V': case 'R': case 'Y': case 'S': case 'W': case 'K': case 'M':
            v = iupac ? (uint32_t)c : ('N' | kLutChanged); break;
        case 'b': case 'd': case 'h': case 'v': case 'r': case 'y': case 's': case 'w': case 'k': case 'm':
            v = iupac ? ((uint32_t)(c - 32) | kLutChanged) : ('N' | kLutChanged); break;
        case ' ': case '\t': case '\r': case '\n': v = ' ' | kLutChanged | kLutDeleted; break;
        default: v = 'N' | kLutChanged; break;
        }
        lut[c] = (uint16_t)v;
    }
}
// strip_returns: reference src/sequence.rs:165-191.
void build_strip_lut(uint16_t *lut)
{
    for (int c = 0; c < 256; c++) lut[c] = (uint16_t)((c == '\r' || c == '\n') ? (c | kLutChanged | kLutDeleted) : c);
}
// complement: reference src/sequence.rs:68-105.
void build_complement_lut(uint16_t *lut)
{
    for (int c = 0; c < 256; c++) lut[c] = (uint16_t)c;
    const char *pairs = "atcgrykmbvdhATCGRYKMBVDH";  // consecutive pairs swap; s/w/S/W map to themselves
    for (int i = 0; pairs[i]; i += 2) {
        lut[(uint8_t)pairs[i]] = (uint8_t)pairs[i + 1];
        lut[(uint8_t)pairs[i + 1]] = (uint8_t)pairs[i];
    }
}

}  // namespace

// What the device buffers of a CompatBank hold.  The banks serve every batched face in turn, so a slot has one name per role; the slots
// and their sizes are shared.
enum BankSlot {
    kSlotBytes = 0,        // every face: the chunk's bytes as uploaded (packed with break bytes for the item arrays, as they lie otherwise)
    kSlotValues = 1,       // bit path: a packed value per position
    kSlotFlags = 1,        // item arrays, byte path: a flag byte per position
    kSlotMinStrand = 1,    // minimizers: is_rc per record
    kSlotValid = 2,        // items: the valid16 plane
    kSlotMinBytes = 2,     // minimizers: m bytes per record
    kSlotRc = 3,           // items: the rc16 plane
    kSlotMinPos = 3,       // minimizers: window start per record
    kSlotCompaction = 4,   // item arrays: block_items u32[nblocks] | block_off u64[nblocks] | total u64 | counts u64[nrec]
    kSlotTotal = 4,        // planes: the chunk's item total
    kSlotBest = 4,         // minimizers: the wave kernel's word, then the long records' `best`
    kSlotOffsets = 5,      // every face: the chunk's nrec + 1 record offsets
    kSlotDense = 6,        // item arrays: pos | value | flag of the items that leave
    kSlotStartBits = 6,    // planes: the record-start bitmap
    kBankSlots = 7
};

// Everything one in-flight chunk of the batched compat faces owns (run_banked).
struct CompatBank {
    Pinned<uint8_t> h_stage;    // record starts + packed bytes (item arrays)
    Pinned<uint64_t> h_total;   // the chunk's item total
    DeviceArray<uint8_t> d[kBankSlots];
    template <class T> T *at(BankSlot s) const { return (T *)d[s].p; }
    hipEvent_t ev_ready = nullptr;      // the chunk is uploaded (item arrays: and its item total is in h_total)
    hipEvent_t ev_computed = nullptr;   // its kernels have run: the download may start
    hipEvent_t ev_landed = nullptr;     // its download has landed: the bank is free again
    uint64_t r0 = 0, nrec = 0, n = 0;   // the chunk: records [r0, r0 + nrec), n bytes on the device
    uint64_t wbase = 0;                 // planes: its first plane word
    uint64_t n_words = 0, nblocks = 0;  // item arrays: the compaction's geometry ...
    size_t o_off = 0, o_total = 0, o_counts = 0;   // ... and where kSlotCompaction keeps what
    bool busy = false;   // its D2H may still be running
};

struct ntk_ctx {
    int device = 0;
    hipStream_t stream = nullptr;       // compute stream (kernels, compat-face copies)
    hipStream_t copy_stream = nullptr;  // H2D copies of pinned batches
    hipStream_t copy_stream2 = nullptr; // ... every second batch's when NTK_OPT_COPY_STREAMS is 2: the next copy is queued on the other DMA queue
                                        // while one runs, so the link does not idle between batches
    uint32_t copy_streams = 2, copy_rr = 0;
    hipStream_t down_stream = nullptr;  // D2H copies of the bit-plane compat face (its uploads keep the copy stream to themselves)
    bool owns_stream = false;
    int n_cu = 256;
    int launch_blocks = 0, launch_threads = 0;   // 0 = automatic
    uint64_t *d_acc = nullptr;      // accumulators in use (own or caller-bound)
    DeviceArray<uint64_t> d_acc_own;
    DeviceArray<uint32_t> d_part_hist;      // the partials of a reduce launch, a row per block (ensure_partials): kHistBins bins ...
    DeviceArray<uint64_t> d_part_scalars;   // ... and 4 scalars
    DeviceArray<uint32_t> d_work;   // kMaxShards work counters, one per 64-B line
    bool work_dirty = true;         // not known to be zero
    uint32_t *d_lower = nullptr;    // kLowerRing flag words behind the work counters: speculative scans of un-normalised byte-path input (run_scan)
    uint32_t lower_idx = 0;
    // ntk_ctx_set_option (test / A-B support, per ctx: nothing in the dispatch reads the environment)
    uint64_t minimizer_chunk = (uint64_t)256 << 20;  // NTK_OPT_MINIMIZER_CHUNK_BYTES: bytes of input per two-pass minimizer pass
    uint64_t compat_chunk = kCompatChunkBytes;      // NTK_OPT_COMPAT_CHUNK_BYTES: packed bytes per chunk of the batched compat faces
    uint32_t route_off = 0;                          // NTK_OPT_MINIMIZER_ROUTE: NTK_ROUTE_NO_* bits
    uint32_t pack_threads = 8;                       // NTK_OPT_COMPAT_PACK_THREADS
    uint64_t wait_poll_us = 50;                      // NTK_OPT_BATCH_WAIT_POLL_US (0: block in hipEventSynchronize)
    uint64_t gz_limit = 0, gz_window = 0, pipe_stats = 0;   // NTK_OPT_GZ_INMEM_LIMIT_BYTES / _STREAM_WINDOW_BYTES / NTK_OPT_PIPE_STATS: read by the producer (ntk_fastx_api.cpp) through ntk_ctx_get_option; 0 = its default
    DeviceArray<uint16_t> d_lut;  // four byte maps of 256 entries each, in the order of the accessors below
    const uint16_t *lut_normalize() const { return d_lut.p; }
    const uint16_t *lut_normalize_iupac() const { return d_lut.p + 256; }
    const uint16_t *lut_strip() const { return d_lut.p + 512; }
    const uint16_t *lut_complement() const { return d_lut.p + 768; }
    DeviceArray<uint8_t> scratch[6];   // of the per-sequence calls; each names its slots at the top of its body
    template <class T> T *scratch_at(int slot) const { return (T *)scratch[slot].p; }
    CompatBank bank[kCompatBanks];   // the chunks the batched compat faces keep in flight (see run_banked)
    Pinned<uint64_t> h_pinned;  // small pinned staging for scalar read-backs
    bool timing = false;
    std::vector<hipEvent_t> ev_free;
    std::vector<std::pair<hipEvent_t, hipEvent_t>> ev_used;
    std::map<std::pair<const void *, int>, int> occupancy;  // resident blocks per CU of a scan build at a block size
    std::map<const void *, int> auto_threads;               // block size chosen for a reduce build (run_scan)
    // released batches are kept for re-use: pinned + device allocations cost milliseconds each, a parser thread's two
    // batches more than its share of a multi-GB input (tools/pipeline_bench.py).  Guarded: producer threads acquire and
    // release concurrently.
    std::mutex pool_mu;
    std::vector<ntk_batch *> pool;
    uint64_t pool_bytes = 0;
};

struct ntk_batch {
    Pinned<uint8_t> h_seq;
    Pinned<uint64_t> h_off;
    DeviceArray<uint8_t> d_seq;
    Pinned<uint8_t> h_qual;                        // allocated by the first ntk_batch_append_quality ...
    DeviceArray<uint8_t> d_qual;                   // ... and a batch without h_qual has no quality stream
    bool has_qual = false;                         // some record of the current fill carries qualities
    uint32_t qual_cutoff = 0;                      // ... appended for this cutoff (must be the one submitted)
    int device = 0;
    uint64_t cap_bytes = 0, cap_records = 0, n_bytes = 0, n_records = 0;
    hipEvent_t ev_copied = nullptr, ev_done = nullptr;
    bool in_flight = false;
};

namespace {

// no scratch buffer is smaller than 256 bytes
int ensure_scratch(ntk_ctx *c, int slot, size_t bytes) { return c->scratch[slot].ensure(c->stream, bytes < 256 ? 256 : bytes, grow_quarter_again_4k); }

int ensure_partials(ntk_ctx *c, int blocks)
{
    const int rc = c->d_part_hist.ensure(c->stream, (uint64_t)blocks * kHistBins, grow_exact);
    return rc ? rc : c->d_part_scalars.ensure(c->stream, (uint64_t)blocks * 4, grow_exact);
}

struct Mode { int kw; bool canon, tie_rc, accept_u; bool raw_bytes = false; };
inline uint32_t quality_cutoff(const ntk_params *p) { return (p->flags >> 8) & 0xFFu; }

int resolve_mode(const ntk_params *p, bool batch_face, Mode *m)
{
    if (!p) return NTK_ERR_BAD_ARG;
    // CanonicalKmers takes k: u8 (reference src/kmer.rs:48-82); 33 <= k <= 255 exists on the byte path's batch face in reduce mode only
    // (counters + histogram; 2-bit values of more than 64 bits have no sum / xor: ntk_result.n_undigested) - every other face is k <= 32
    if (p->k < 1 || p->k > (batch_face && p->path == NTK_PATH_BYTES_CANONICAL ? 255u : 32u)) return NTK_ERR_BAD_K;
    if ((p->flags & ~(0xFFFFu | NTK_FLAG_RESET)) != 0 || p->pre > NTK_PRE_NORMALIZE_IUPAC) return NTK_ERR_BAD_ARG;
    m->kw = p->k > 16 ? 2 : 1;
    m->accept_u = p->pre >= NTK_PRE_NORMALIZE;
    switch (p->path) {
    case NTK_PATH_BYTES_CANONICAL:
        // The byte path compares RAW bytes (reference src/kmer.rs:124); that equals the 2-bit order only when
        // every base has the same case, which normalize guarantees.  Un-normalised byte-path input is scanned speculatively (the packed-value
        // scan watches for lower case; canonical_bytes_reduce_kernel redoes the launch if there was any: run_scan); items: ntk_canonical_kmers*.
        m->raw_bytes = batch_face && (p->pre < NTK_PRE_NORMALIZE || p->k > 32);
        m->canon = true; m->tie_rc = true; break;
    case NTK_PATH_BITS: m->canon = false; m->tie_rc = false; break;
    case NTK_PATH_BITS_CANONICAL: m->canon = true; m->tie_rc = false; break;
    default: return NTK_ERR_BAD_ARG;
    }
    return NTK_OK;
}

// The scan kernel build for a mode.  Reduce mode: every (path, k, quality stream or not) has its own scan2_kernel instantiation (k is
// a template constant: the window-mask algebra indexes lane masks by k; ntk_scan2.hip).  Materialise mode: the round-1 scan_kernel with
// k at run time, plus a k = 21 build for the canonical paths (-5 %); it runs at the rate of a plain read-1-write-8 expansion kernel
// (2.45 ms per 1.51 GB of input against 2.45-2.50 ms, profiles/r04b/wbw.txt), i.e. it is bound by the 8 bytes it writes per position.
constexpr uint32_t kLowerRing = 64;  // "a lower-case byte was seen" flags of consecutive speculative launches (each launch clears its successor's)

// The round-1 scan_kernel, materialise mode only (QM names a template argument).
// (no TIE_RC && !ACCEPT_U build: that is the byte path on input that was not normalised, which materialise mode rejects - run_scan)
template <bool QM>
const void *pick_materialise(const Mode &m, uint32_t k)
{
#define NTK_PICK_FIX(KF, T, U)                                                                      \
    if (!QM && m.kw == 2 && m.canon && k == KF && m.tie_rc == T && m.accept_u == U)                  \
        return (const void *)&scan_kernel<2, true, T, U, false, KF>;
    NTK_PICK_FIX(21, false, false) NTK_PICK_FIX(21, false, true) NTK_PICK_FIX(21, true, true)
#undef NTK_PICK_FIX
#define NTK_PICK(KW, C, T, U)                                                                       \
    if (m.kw == KW && m.canon == C && m.tie_rc == T && m.accept_u == U)                             \
        return (const void *)&scan_kernel<KW, C, T, U, false, 0, QM>;
    NTK_PICK(1, false, false, false) NTK_PICK(1, false, false, true)
    NTK_PICK(1, true, false, false) NTK_PICK(1, true, false, true)
    NTK_PICK(1, true, true, true)
    NTK_PICK(2, false, false, false) NTK_PICK(2, false, false, true)
    NTK_PICK(2, true, false, false) NTK_PICK(2, true, false, true)
    NTK_PICK(2, true, true, true)
#undef NTK_PICK
    return nullptr;
}

// reduce mode: every (path, k, quality) has an sv2 build; the kernel lives in its own translation unit (ntk_scan2.hip, built
// with the ILP-driven iterative scheduler).
const void *pick_scan(const Mode &m, uint32_t k, bool reduce, bool quality)
{
    if (!reduce) return quality ? pick_materialise<true>(m, k) : pick_materialise<false>(m, k);
    if (quality) return ntk_pick_scan2_q((int)k, m.canon, m.tie_rc, m.accept_u);
    return m.canon ? ntk_pick_scan2((int)k, m.tie_rc, m.accept_u) : ntk_pick_scan2_fwd((int)k, m.accept_u);
}

// Fused windowed-minimizer builds of the sv2 kernel (ntk_tile.hpp lane_tile_sv2_min): k = 15..23 x w = 5, 9..12 (windows of up to 34 bytes),
// and quality-masked builds of (21, 11) and (15, 10) (ntk_scan2.hip); every other (k, w) takes the two-pass path (materialise +
// window-min).
const void *pick_scan_min(const Mode &m, uint32_t k, uint32_t w, bool quality)
{
    if (!m.canon) return nullptr;
    if (const void *fn = ntk_pick_scan2_min_a((int)k, (int)w, m.tie_rc, m.accept_u, quality)) return fn;
    return ntk_pick_scan2_min_b((int)k, (int)w, m.tie_rc, m.accept_u, quality);
}

int get_event(ntk_ctx *c, hipEvent_t *e)
{
    if (!c->ev_free.empty()) { *e = c->ev_free.back(); c->ev_free.pop_back(); return NTK_OK; }
    HIPCHK(hipEventCreate(e));
    return NTK_OK;
}

// What every reduce / materialise launch is made of.  A timed span on c->stream (ntk_ctx_enable_timing; a no-op without it): begin() takes an
// event pair from the pool and records the start, end() records the stop and files the pair in `used`.  A span that does not get that far -
// any error return on the way - hands both events back to the pool when it goes out of scope.
struct TimedSpan {
    ntk_ctx *c = nullptr;
    hipEvent_t e0 = nullptr, e1 = nullptr;
    TimedSpan() = default;
    TimedSpan(const TimedSpan &) = delete;
    TimedSpan &operator=(const TimedSpan &) = delete;
    ~TimedSpan() { for (hipEvent_t e : {e0, e1}) if (e) c->ev_free.push_back(e); }
    int begin(ntk_ctx *ctx)
    {
        if (!ctx->timing) return NTK_OK;
        c = ctx;
        int rc = get_event(c, &e0);
        if (!rc) rc = get_event(c, &e1);
        if (rc) return rc;
        HIPCHK(hipEventRecord(e0, c->stream));
        return NTK_OK;
    }
    int end(std::vector<std::pair<hipEvent_t, hipEvent_t>> &used)
    {
        if (!e0) return NTK_OK;
        HIPCHK(hipEventRecord(e1, c->stream));
        used.emplace_back(e0, e1);
        e0 = e1 = nullptr;
        return NTK_OK;
    }
};

// the blocks a launch may use: what ntk_ctx_set_launch forces, else per_cu on every CU
inline uint64_t block_cap(const ntk_ctx *c, int per_cu) { return c->launch_blocks > 0 ? (uint64_t)c->launch_blocks : (uint64_t)c->n_cu * per_cu; }
inline int blocks_for(const ntk_ctx *c, uint64_t n, uint64_t tile, int per_cu)   // one block per tile of input, up to the cap
{
    const uint64_t n_tiles = (n + tile - 1) / tile, cap = block_cap(c, per_cu);
    return (int)(n_tiles < cap ? n_tiles : cap);
}

// resident blocks per CU of build fn at a block size, clamped to 1..cap; asked once per (fn, threads)
int resident_blocks(ntk_ctx *c, const void *fn, int threads, size_t lds, int cap, int *per_cu)
{
    const auto key = std::make_pair(fn, threads);
    auto it = c->occupancy.find(key);
    if (it != c->occupancy.end()) { *per_cu = it->second; return NTK_OK; }
    HIPCHK(hipOccupancyMaxActiveBlocksPerMultiprocessor(per_cu, fn, threads, lds));
    *per_cu = *per_cu < 1 ? 1 : (*per_cu > cap ? cap : *per_cu);
    c->occupancy[key] = *per_cu;
    return NTK_OK;
}

// the flag word of a speculative launch and its successor's, which the launch clears (the ring of kLowerRing words behind the work counters)
struct FlagPair { uint32_t *flag = nullptr, *next = nullptr; };
inline FlagPair next_flag(ntk_ctx *c)
{
    FlagPair f;
    f.flag = c->d_lower + c->lower_idx;
    c->lower_idx = (c->lower_idx + 1) % kLowerRing;
    f.next = c->d_lower + c->lower_idx;
    return f;
}

// fold_kernel over `rows` rows of the ctx partials into the ctx accumulators (same stream, behind the kernels that wrote them)
struct Fold {
    uint32_t rearm_shards = 0;           // the scan pulled its tiles from this many work counters: the fold zeroes them for the next scan
    const uint32_t *alt_flag = nullptr;  // speculative routes: if this flag is up the companion kernel redid the launch ...
    int alt_rows = 0;                    // ... and left this many rows in place of the first kernel's
    bool undigested = false;             // k > 32 partials: their k-mers are counted in NTK_ACC_UNDIGESTED as well
};
int launch_fold(ntk_ctx *c, int rows, const Fold &f = Fold())
{
    hipLaunchKernelGGL(fold_kernel, dim3(kFoldBlocks), dim3(kFoldThreads), 0, c->stream, (const uint32_t *)c->d_part_hist.p,
                       (const uint64_t *)c->d_part_scalars.p, rows, c->d_acc, f.rearm_shards ? c->d_work.p : (uint32_t *)nullptr, (int)f.rearm_shards,
                       f.alt_flag, f.alt_rows, f.undigested ? 1 : 0);
    HIPCHK(hipGetLastError());
    if (f.rearm_shards) c->work_dirty = false;
    return NTK_OK;
}

inline bool bad_device_input(const uint8_t *d_seq, const uint8_t *d_qual) { return !d_seq || ((uintptr_t)d_seq & 15) || ((uintptr_t)d_qual & 15); }

// The quality switch.  ScanArgs kernels read the stream from their arguments (cutoff 0 masks nothing: the plain build runs) ...
inline void scan_args_set_quality(ScanArgs &a, const uint8_t *d_qual, uint32_t cutoff)
{
    if (!cutoff) return;
    const QualityCut qc = quality_cut(cutoff);
    a.qual = d_qual; a.q_add = qc.add; a.q_sel = qc.sel;
}
// ... the byte-walking and k > 32 kernels have a quality build that takes (qual, q_add, q_sel) as three trailing arguments (ntk_kernels.hpp
// QualIn): kernel_q with d_qual set (masking at `cutoff`, 1..255), the plain kernel without.
template <class KernelQ, class Kernel, class... Args>
void launch_with_quality(ntk_ctx *c, KernelQ kernel_q, Kernel kernel, int blocks, int threads, const uint8_t *d_qual, uint32_t cutoff, Args... args)
{
    if (d_qual) {
        const QualityCut qc = quality_cut(cutoff);
        hipLaunchKernelGGL(kernel_q, dim3(blocks), dim3(threads), 0, c->stream, args..., d_qual, qc.add, qc.sel);
    } else
        hipLaunchKernelGGL(kernel, dim3(blocks), dim3(threads), 0, c->stream, args...);
}

// CanonicalKmers over raw (un-normalised) bytes into the accumulators: canonical_bytes_reduce_kernel + fold (ntk_kernels.hpp).
inline int raw_bytes_blocks(const ntk_ctx *c, uint64_t n) { return blocks_for(c, n, (uint64_t)kPlThreads * 32, 8); }   // (32 starts per thread)

// the quality builds of the byte-walking and k > 32 kernels: (qual, q_add, q_sel) as three trailing arguments (ntk_kernels.hpp QualIn)
template <bool WIDE> constexpr auto bytes_reduce_q = &canonical_bytes_reduce_kernel<WIDE, true, const uint8_t *, uint32_t, uint32_t>;
template <bool ACCEPT_U> constexpr auto wide_reduce_q = &wide_canonical_reduce_kernel<ACCEPT_U, true, const uint8_t *, uint32_t, uint32_t>;

// canonical_bytes_reduce_kernel<wide> over d_seq[0, n), or its quality build when d_qual is set.
void launch_raw_bytes(ntk_ctx *c, bool wide, int blocks, const uint8_t *d_seq, uint64_t n, uint32_t k, const uint32_t *run_if, bool normalized,
                      const uint8_t *d_qual, uint32_t cutoff)
{
    const uint32_t pb = k < 6 ? k : 6;
    launch_with_quality(c, wide ? bytes_reduce_q<true> : bytes_reduce_q<false>, wide ? &canonical_bytes_reduce_kernel<true> : &canonical_bytes_reduce_kernel<false>,
                        blocks, kPlThreads, d_qual, cutoff, d_seq, n, (n + 15) & ~(uint64_t)15, k, 2u * (k - pb), c->lut_complement(),
                        c->d_part_hist.p, c->d_part_scalars.p, run_if, wide && normalized ? 1u : 0u);
}

// The reduce routes of the byte path that no packed-value scan serves alone (d_qual with cutoff 1..255: the quality stream, masked before the
// walk; NULL: none).  k <= 32 on input that was not normalised: canonical_bytes_reduce_kernel<false> walks the raw bytes.
// k = 33..255 (counters + histogram): wide_canonical_reduce_kernel decides the strand on the first 32 bases of the packed 2-bit streams;
// canonical_bytes_reduce_kernel<true> is queued behind it and returns at once unless that launch raised its flag (two k-mers equal over 32
// bases, or - on input that was not normalised - a byte with bit 5 set), and the fold takes whichever partials are valid.  No host round
// trip; 0.9 ms instead of 9.5 per 1.5 GB at k = 64 (profiles/r06r).  Under NTK_ROUTE_NO_SPECULATION the byte walk runs alone.
int run_bytes_reduce(ntk_ctx *c, const uint8_t *d_seq, uint64_t n, const ntk_params *p, bool zero_first, bool normalized,
                     const uint8_t *d_qual, uint32_t cutoff)
{
    const bool wide = p->k > 32, packed_first = wide && !(c->route_off & NTK_ROUTE_NO_SPECULATION);
    if (zero_first) HIPCHK(hipMemsetAsync(c->d_acc, 0, NTK_ACC_WORDS * sizeof(uint64_t), c->stream));
    const int blocks_raw = raw_bytes_blocks(c, n), blocks = packed_first ? blocks_for(c, n, kWkTile, 8) : blocks_raw;
    int rc = ensure_partials(c, blocks > blocks_raw ? blocks : blocks_raw);
    if (rc) return rc;
    Fold fold;
    fold.undigested = wide;
    TimedSpan span;
    if ((rc = span.begin(c))) return rc;
    if (packed_first) {
        const FlagPair f = next_flag(c);
        launch_with_quality(c, normalized ? wide_reduce_q<true> : wide_reduce_q<false>,
                            normalized ? &wide_canonical_reduce_kernel<true> : &wide_canonical_reduce_kernel<false>, blocks, kWkThreads, d_qual, cutoff,
                            d_seq, n, p->k, c->d_part_hist.p, c->d_part_scalars.p, f.flag, f.next);
        HIPCHK(hipGetLastError());
        fold.alt_flag = f.flag; fold.alt_rows = blocks_raw;
    }
    launch_raw_bytes(c, wide, blocks_raw, d_seq, n, p->k, fold.alt_flag, normalized, d_qual, cutoff);
    HIPCHK(hipGetLastError());
    if ((rc = span.end(c->ev_used))) return rc;
    return launch_fold(c, blocks, fold);
}

// One scan of a pull-model kernel that takes a ScanArgs (scan_kernel, scan2_kernel, minimizer_scan_kernel) over a.seq[0, a.n_bytes).
// The caller picks the build and its geometry (TileScan) and fills what is its own in `a`: k, window, quality stream, output planes.
// Everything else is done here, once: the launch ranges of at most kMaxTilesPerLaunch tiles, shards and tiles per pull (plan_launch,
// ntk_plan.hpp), the work counters, zero_acc on the first launch only, the partials, the timed span and - in reduce mode - the fold.
struct TileScan {
    const void *fn = nullptr;
    int threads = 0;
    size_t lds = 0;           // dynamic LDS per block
    uint32_t stride = 0;      // bytes a tile advances by = window ends it emits: the build's own (Sv2Geom<..>::kStride, kTileStride, ...)
    uint64_t max_chunk = 0;   // cap on tiles per pull
    int max_per_cu = 0;       // cap on resident blocks per CU; the auto grid is exactly the resident blocks (work is pulled: more only write empty histograms, +1.5 %)
    bool reduce = true;       // partials + fold; a materialise scan has neither
    bool speculate = false;   // the SPEC build on un-normalised byte-path input: canonical_bytes_reduce_kernel<false> is queued behind the scan,
    uint32_t cutoff = 0;      // ... masking a.qual at this cutoff (0: no quality stream)
};
int launch_tile_scan(ntk_ctx *c, const TileScan &s, ScanArgs &a, bool zero_first)   // zero_first: the first launch zeroes the accumulators in its prologue
{
    int per_cu = 0, rc = resident_blocks(c, s.fn, s.threads, s.lds, s.max_per_cu, &per_cu);
    if (rc) return rc;
    const uint64_t blocks_max = block_cap(c, per_cu), waves_per_block = (uint64_t)s.threads / 64;
    const uint64_t n = a.n_bytes;
    const int blocks_raw = s.speculate ? raw_bytes_blocks(c, n) : 0;
    a.n_tiles = tile_count(n, s.stride);
    a.work_counters = c->d_work.p;
    a.zero_words = NTK_ACC_WORDS;
    for (uint64_t tb = 0; tb < a.n_tiles; tb += kMaxTilesPerLaunch) {
        const LaunchPlan lp = plan_launch(n, s.stride, tb, blocks_max, waves_per_block, s.max_chunk);
        const int blocks = (int)lp.blocks;
        a.tile_begin = lp.tile_begin; a.tile_end = lp.tile_end;
        a.tail_tile_rel = lp.tail_tile_rel;
        a.n_shards = lp.n_shards;
        a.tiles_per_shard = lp.tiles_per_shard;
        a.chunk_tiles = lp.chunk_tiles;
        a.zero_acc = zero_first ? c->d_acc : nullptr;
        zero_first = false;
        // the work counters are zero on entry: the fold of the previous reduce scan re-armed them (launch_fold); anything else
        // (first use, a materialise scan, an error on the way) leaves work_dirty set and costs a memset here
        if (c->work_dirty) HIPCHK(hipMemsetAsync(c->d_work.p, 0, kMaxShards * 64, c->stream));
        c->work_dirty = true;
        if (s.reduce) {
            if ((rc = ensure_partials(c, blocks > blocks_raw ? blocks : blocks_raw))) return rc;
            a.part_hist = c->d_part_hist.p; a.part_scalars = c->d_part_scalars.p;
        }
        Fold fold;
        fold.rearm_shards = a.n_shards;
        if (s.speculate) {
            const FlagPair f = next_flag(c);
            a.lower_flag = f.flag; a.lower_flag_next = f.next;
            fold.alt_flag = f.flag; fold.alt_rows = blocks_raw;
        }
        TimedSpan span;
        if ((rc = span.begin(c))) return rc;
        void *kargs[] = {(void *)&a};
        HIPCHK(hipLaunchKernel(s.fn, dim3(blocks), dim3(s.threads), kargs, s.lds, c->stream));
        if (s.speculate) {   // (inside the timed span: the pair is this route's scan)
            launch_raw_bytes(c, false, blocks_raw, a.seq, n, a.k, fold.alt_flag, false, a.qual, s.cutoff);
            HIPCHK(hipGetLastError());
        }
        if ((rc = span.end(c->ev_used))) return rc;
        if (s.reduce && (rc = launch_fold(c, blocks, fold))) return rc;
    }
    return NTK_OK;
}

// The k-mer scans (reduce and materialise) and the register-fused minimizer builds of scan2_kernel.
int run_scan(ntk_ctx *c, const uint8_t *d_seq, uint64_t n, const ntk_params *p, const Mode &m, bool reduce,
             uint64_t *d_values, uint16_t *d_valid16, uint16_t *d_rc16, const uint8_t *d_qual = nullptr, const void *fused_min_fn = nullptr,
             uint32_t fused_w = 0)   // the window length of a fused-minimizer build: its tile geometry differs (ntk_tile.hpp Sv2Geom)
{
    const bool zero_first = reduce && (p->flags & NTK_FLAG_RESET);
    if (n == 0) {
        if (zero_first) HIPCHK(hipMemsetAsync(c->d_acc, 0, NTK_ACC_WORDS * sizeof(uint64_t), c->stream));
        return NTK_OK;
    }
    if (bad_device_input(d_seq, d_qual)) return NTK_ERR_BAD_ARG;
    const uint32_t cutoff = d_qual ? quality_cutoff(p) : 0u;  // cutoff 0 masks nothing: the plain build runs
    // the stride of the build that runs, from the geometry it was compiled with: a scan2 build in reduce mode (k <= 32: larger k leaves through
    // run_bytes_reduce below), scan_kernel in materialise mode
    const uint32_t stride = !reduce ? (uint32_t)kTileStride : (p->k <= 32 ? (uint32_t)sv2_stride_bytes((int)(fused_w ? p->k + fused_w - 1 : p->k), fused_w == 0) : 0u);
    bool speculate = false;
    if (m.raw_bytes) {
        // byte path on input that was not normalised: reduce mode only; dense values and windowed minimizers on such input are not built
        // (normalize first, as the reference's documented chain does), and k > 32 has counters + histogram only.  A quality stream is masked
        // in by every kernel of the route (`(seq, qual).quality_mask(cutoff)` ahead of canonical_kmers, reference src/sequence.rs:237-239,285-296).
        if (p->k > 32 && (!reduce || fused_min_fn)) return NTK_ERR_BAD_K;
        if (!reduce || fused_min_fn) return NTK_ERR_UNSUPPORTED;
        const uint8_t *qual = cutoff ? d_qual : nullptr;
        // k <= 32: the raw-byte order is the 2-bit order unless a base is lower case - the clean read on which Sequence::normalize returns
        // None (reference src/sequence.rs:57-61).  So the packed-value scan runs (its TIE_RC, !ACCEPT_U build watches every byte it loads for
        // bit 5), the raw-byte kernel is queued behind it and returns at once unless the flag went up, and the fold takes whichever partials
        // are valid: no host round trip, 0.45 ms instead of 5.1 per 1.5 GB of upper-case reads.  One launch only (the raw-byte kernel works on
        // window starts, the scan on window ends: their launch ranges do not line up), the direct route otherwise and under NTK_ROUTE_NO_SPECULATION.
        speculate = p->k <= 32 && tile_count(n, stride) <= kMaxTilesPerLaunch && !(c->route_off & NTK_ROUTE_NO_SPECULATION);
        if (!speculate) return run_bytes_reduce(c, d_seq, n, p, zero_first, m.accept_u, qual, cutoff);   // (accept_u: only k > 32 comes here normalised)
    }
    const void *fn = fused_min_fn ? fused_min_fn : pick_scan(m, p->k, reduce, cutoff != 0);   // (speculate: tie_rc, !accept_u - the SPEC build)
    if (!fn) return NTK_ERR_BAD_ARG;
    // every reduce-mode scan (any path, any k, with or without a quality stream, fused minimizers) is a scan2 build: 768 threads, two
    // blocks per CU = 6 waves per SIMD, which needs <= 80 VGPRs.  A build above that would get ONE 768-thread block per CU; it runs
    // 640-thread blocks instead (two per CU: 5 waves per SIMD).  (No shipped build is above it: the k-mer builds need <= 75, the
    // fused-minimizer builds are compiled under the 6-wave budget, csrc/Makefile MIN_FLAGS.)
    int threads = !reduce ? 256 : (c->launch_threads ? c->launch_threads : 768);
    if (reduce && !c->launch_threads) {
        auto it = c->auto_threads.find(fn);
        if (it != c->auto_threads.end()) threads = it->second;
        else {
            int best_waves = 0;
            for (int t : {768, 640, 512}) {
                int blocks_cu = 0;
                HIPCHK(hipOccupancyMaxActiveBlocksPerMultiprocessor(&blocks_cu, fn, t, 0));
                if (blocks_cu > 2) blocks_cu = 2;
                if (blocks_cu * t > best_waves) { best_waves = blocks_cu * t; threads = t; }
            }
            c->auto_threads[fn] = threads;
        }
    }
    // Reduce builds: two blocks of `threads` (768, or 640 / 512 for a build above 80 VGPRs: chosen above) per CU, each with its 64 KiB LDS
    // histogram, <= 24 tiles per pull; materialise stages 8.7 KiB per wave through LDS: 256-thread blocks, 4 per CU.
    TileScan s;
    s.fn = fn; s.threads = threads; s.stride = stride; s.max_chunk = 24;
    s.lds = reduce ? 0 : (size_t)(threads / 64) * kStageWaveU64 * sizeof(uint64_t);
    s.max_per_cu = reduce ? 2 * (1024 / threads) : 4;
    s.reduce = reduce; s.speculate = speculate; s.cutoff = cutoff;
    ScanArgs a;
    memset(&a, 0, sizeof(a));
    scan_args_set_k(a, p->k);
    a.seq = d_seq; a.n_bytes = n;
    a.values = d_values; a.valid16 = d_valid16; a.rc16 = d_rc16;
    scan_args_set_quality(a, d_qual, cutoff);
    return launch_tile_scan(c, s, a, zero_first);
}

// Generic fused windowed minimizers (ntk_kernels.hpp minimizer_scan_kernel): any k <= 31 and w <= 49 of the canonical paths, with or
// without a quality stream; the tile geometry depends on w (2 + ceil((w - 1) / 16) non-emitting lanes).
const void *pick_min_generic(const Mode &m, bool quality, bool f64, uint32_t k)   // f64: k <= 25 (one v_min_f64 per minimum, ntk_tile.hpp)
{
    const int kw = f64 ? 2 : m.kw;   // (the f64 keys are built from the code streams for any k: one instantiation serves both word counts)
    const int mode = min_gen_mode(k, f64);
#define NTK_PICK_MG(KW, T, U, Q, F, MD) if (kw == KW && m.tie_rc == T && m.accept_u == U && quality == Q && f64 == F && mode == MD) return (const void *)&minimizer_scan_kernel<KW, T, U, Q, F, MD>;
// (no TIE_RC && !ACCEPT_U build: the byte path on input that was not normalised never gets here - minimizers_reduce_impl rejects it)
#define NTK_PICK_MG3(KW, Q, F, MD) NTK_PICK_MG(KW, false, false, Q, F, MD) NTK_PICK_MG(KW, false, true, Q, F, MD) NTK_PICK_MG(KW, true, true, Q, F, MD)
#define NTK_PICK_MG6(KW, F, MD) NTK_PICK_MG3(KW, false, F, MD) NTK_PICK_MG3(KW, true, F, MD)
    NTK_PICK_MG6(2, true, 0) NTK_PICK_MG6(2, true, 1) NTK_PICK_MG6(2, true, 3) NTK_PICK_MG6(2, true, 2)   // f64 keys: k <= 7, 8..18, 19..23, 24..25
    NTK_PICK_MG6(2, false, 2)                                                                             // 26 <= k <= 31
    NTK_PICK_MG6(2, false, 1) NTK_PICK_MG6(1, false, 0) NTK_PICK_MG6(1, false, 1)                         // (only under NTK_ROUTE_NO_F64, the A/B switch)
#undef NTK_PICK_MG6
#undef NTK_PICK_MG3
#undef NTK_PICK_MG
    return nullptr;
}

int run_min_scan(ntk_ctx *c, const uint8_t *d_seq, uint64_t n, const ntk_params *p, const Mode &m, uint32_t w, const uint8_t *d_qual)
{
    if (bad_device_input(d_seq, d_qual)) return NTK_ERR_BAD_ARG;
    const uint32_t cutoff = d_qual ? quality_cutoff(p) : 0u;
    const bool f64 = p->k <= 25 && !(c->route_off & NTK_ROUTE_NO_F64);
    ScanArgs a;
    memset(&a, 0, sizeof(a));
    scan_args_set_k(a, p->k);
    a.seq = d_seq; a.n_bytes = n;
    scan_args_set_quality(a, d_qual, cutoff);
    scan_args_set_window(a, w);   // halo lanes, the validity smear, the overlap of the two power-of-two windows (ntk_tile.hpp)
    TileScan s;
    s.fn = pick_min_generic(m, cutoff != 0, f64, p->k);
    if (!s.fn) return NTK_ERR_BAD_ARG;
    s.threads = min_gen_threads(f64);   // 512: two blocks per CU, 768: one (ntk_kernels.hpp), each with its 64 KiB LDS histogram
    s.stride = (64u - a.min_halo_lanes) * 16u; s.max_chunk = 16; s.max_per_cu = 8;
    return launch_tile_scan(c, s, a, (p->flags & NTK_FLAG_RESET) != 0);
}

void destroy_batch(ntk_batch *b)
{
    b->h_seq.release(); b->h_off.release(); b->d_seq.release();
    b->h_qual.release(); b->d_qual.release();
    if (b->ev_copied) (void)hipEventDestroy(b->ev_copied);
    if (b->ev_done) (void)hipEventDestroy(b->ev_done);
    delete b;
}

int init_ctx(ntk_ctx *c, void *stream, bool borrow);

int create_ctx(int device, void *stream, bool borrow, ntk_ctx **out)
{
    if (!out) return NTK_ERR_BAD_ARG;
    *out = nullptr;
    int count = 0;
    if (hipGetDeviceCount(&count) != hipSuccess || count <= 0) { (void)hipGetLastError(); return NTK_ERR_NO_DEVICE; }
    if (device < 0 || device >= count) return NTK_ERR_NO_DEVICE;
    HIPCHK(hipSetDevice(device));
    hipDeviceProp_t prop;
    HIPCHK(hipGetDeviceProperties(&prop, device));
    if (strncmp(prop.gcnArchName, "gfx950", 6) != 0) return NTK_ERR_NO_DEVICE;  // kernels are built for gfx950 only
    ntk_ctx *c = new (std::nothrow) ntk_ctx();
    if (!c) return NTK_ERR_NOMEM;
    c->device = device;
    c->n_cu = prop.multiProcessorCount > 0 ? prop.multiProcessorCount : 256;
    const int rc = init_ctx(c, stream, borrow);
    if (rc != NTK_OK) { ntk_ctx_destroy(c); return rc; }   // nothing created so far is leaked (destroy skips what is null)
    *out = c;
    return NTK_OK;
}

int init_ctx(ntk_ctx *c, void *stream, bool borrow)
{
    if (borrow) { c->stream = (hipStream_t)stream; c->owns_stream = false; }
    else { HIPCHK(hipStreamCreateWithFlags(&c->stream, hipStreamNonBlocking)); c->owns_stream = true; }
    HIPCHK(hipStreamCreateWithFlags(&c->copy_stream, hipStreamNonBlocking));
    HIPCHK(hipStreamCreateWithFlags(&c->copy_stream2, hipStreamNonBlocking));
    HIPCHK(hipStreamCreateWithFlags(&c->down_stream, hipStreamNonBlocking));
    int rc;
    if ((rc = c->d_acc_own.ensure(c->stream, NTK_ACC_WORDS, grow_exact))) return rc;
    c->d_acc = c->d_acc_own.p;
    HIPCHK(hipMemsetAsync(c->d_acc, 0, NTK_ACC_WORDS * sizeof(uint64_t), c->stream));
    if ((rc = c->d_work.ensure(c->stream, kMaxShards * 16 + kLowerRing, grow_exact))) return rc;
    c->d_lower = c->d_work.p + kMaxShards * 16;
    HIPCHK(hipMemsetAsync(c->d_lower, 0, kLowerRing * sizeof(uint32_t), c->stream));
    if ((rc = c->d_lut.ensure(c->stream, 4 * 256, grow_exact)) || (rc = c->h_pinned.alloc(64 * 1024 / sizeof(uint64_t)))) return rc;
    uint16_t *h = (uint16_t *)c->h_pinned.p;
    build_normalize_lut(h, false);
    build_normalize_lut(h + 256, true);
    build_strip_lut(h + 512);
    build_complement_lut(h + 768);
    HIPCHK(hipMemcpyAsync(c->d_lut.p, h, 4 * 256 * sizeof(uint16_t), hipMemcpyHostToDevice, c->stream));
    HIPCHK(hipStreamSynchronize(c->stream));
    return NTK_OK;
}

}  // namespace

extern "C" {

const char *ntk_strerror(int s)
{
    switch (s) {
    case NTK_OK: return "ok";
    case NTK_ERR_BAD_K: return "k out of range for this entry point";
    case NTK_ERR_BAD_ARG: return "bad argument (null / misaligned pointer or bad enum)";
    case NTK_ERR_HIP: return "HIP runtime error (see ntk_last_hip_error)";
    case NTK_ERR_NO_DEVICE: return "no usable gfx950 device";
    case NTK_ERR_CAPACITY: return "output or batch capacity too small";
    case NTK_ERR_UNSUPPORTED: return "combination not supported on the device path (no CPU fallback exists)";
    case NTK_ERR_NOMEM: return "out of memory";
    case NTK_ERR_PARSE: return "FASTA/FASTQ parse error (see ntk_reader_error)";
    case NTK_ERR_RCCL: return "RCCL error (see ntk_last_rccl_error)";
    case NTK_EOF: return "end of input";
    default: return "unknown status";
    }
}
int ntk_last_hip_error(void) { return g_last_hip; }
int ntk_last_rccl_error(void) { return g_last_rccl; }
int ntk_abi_version(void) { return NTK_ABI_VERSION; }

int ntk_device_count(int *n)
{
    if (!n) return NTK_ERR_BAD_ARG;
    *n = 0;
    int count = 0;
    if (hipGetDeviceCount(&count) != hipSuccess || count <= 0) { (void)hipGetLastError(); return NTK_OK; }
    for (int d = 0; d < count; d++) {   // devices are usable as a prefix 0 .. n-1: stop at the first that is not gfx950
        hipDeviceProp_t prop;
        if (hipGetDeviceProperties(&prop, d) != hipSuccess) { (void)hipGetLastError(); break; }
        if (strncmp(prop.gcnArchName, "gfx950", 6) != 0) break;
        *n = d + 1;
    }
    return NTK_OK;
}

int ntk_ctx_create(int device, ntk_ctx **out) { return create_ctx(device, nullptr, false, out); }
int ntk_ctx_create_on_stream(int device, void *hip_stream, ntk_ctx **out) { return create_ctx(device, hip_stream, true, out); }

void ntk_ctx_destroy(ntk_ctx *c)
{
    if (!c) return;
    (void)hipSetDevice(c->device);
    if (c->stream || !c->owns_stream) (void)hipStreamSynchronize(c->stream);
    if (c->copy_stream) (void)hipStreamSynchronize(c->copy_stream);
    if (c->copy_stream2) (void)hipStreamSynchronize(c->copy_stream2);
    if (c->down_stream) (void)hipStreamSynchronize(c->down_stream);
    for (auto &p : c->ev_used) { (void)hipEventDestroy(p.first); (void)hipEventDestroy(p.second); }
    for (auto e : c->ev_free) (void)hipEventDestroy(e);
    for (auto b : c->pool) destroy_batch(b);
    c->pool.clear();
    for (auto &s : c->scratch) s.release();
    c->d_part_hist.release(); c->d_part_scalars.release();
    c->d_acc_own.release(); c->d_lut.release(); c->d_work.release();
    c->h_pinned.release();
    for (CompatBank &b : c->bank) {
        b.h_stage.release(); b.h_total.release();
        for (auto &s : b.d) s.release();
        for (hipEvent_t e : {b.ev_ready, b.ev_computed, b.ev_landed}) if (e) (void)hipEventDestroy(e);
    }
    if (c->owns_stream && c->stream) (void)hipStreamDestroy(c->stream);
    if (c->copy_stream) (void)hipStreamDestroy(c->copy_stream);
    if (c->copy_stream2) (void)hipStreamDestroy(c->copy_stream2);
    if (c->down_stream) (void)hipStreamDestroy(c->down_stream);
    delete c;
}

int ntk_ctx_synchronize(ntk_ctx *c)
{
    if (!c) return NTK_ERR_BAD_ARG;
    HIPCHK(hipSetDevice(c->device));   // (a process may drive several devices: every entry point selects its ctx's own)
    HIPCHK(hipStreamSynchronize(c->copy_stream));
    HIPCHK(hipStreamSynchronize(c->copy_stream2));
    HIPCHK(hipStreamSynchronize(c->stream));
    return NTK_OK;
}

int ntk_ctx_stream(ntk_ctx *c, int *device, void **hip_stream)
{
    if (!c || !device || !hip_stream) return NTK_ERR_BAD_ARG;
    *device = c->device;
    *hip_stream = (void *)c->stream;
    return NTK_OK;
}

int ntk_ctx_set_launch(ntk_ctx *c, int blocks, int threads)
{
    if (!c || blocks < 0 || threads < 0 || threads > 1024 || (threads & 63)) return NTK_ERR_BAD_ARG;   // threads 0 = automatic
    c->launch_blocks = blocks; c->launch_threads = threads;
    return NTK_OK;
}

int ntk_ctx_get_option(ntk_ctx *c, int option, uint64_t *value)
{
    if (!c || !value) return NTK_ERR_BAD_ARG;
    switch (option) {
    case NTK_OPT_COMPAT_CHUNK_BYTES: *value = c->compat_chunk; return NTK_OK;
    case NTK_OPT_MINIMIZER_CHUNK_BYTES: *value = c->minimizer_chunk; return NTK_OK;
    case NTK_OPT_MINIMIZER_ROUTE: *value = c->route_off; return NTK_OK;
    case NTK_OPT_COMPAT_PACK_THREADS: *value = c->pack_threads; return NTK_OK;
    case NTK_OPT_COPY_STREAMS: *value = c->copy_streams; return NTK_OK;
    case NTK_OPT_BATCH_WAIT_POLL_US: *value = c->wait_poll_us ? c->wait_poll_us : NTK_POLL_BLOCK; return NTK_OK;
    case NTK_OPT_GZ_INMEM_LIMIT_BYTES: *value = c->gz_limit; return NTK_OK;
    case NTK_OPT_GZ_STREAM_WINDOW_BYTES: *value = c->gz_window; return NTK_OK;
    case NTK_OPT_PIPE_STATS: *value = c->pipe_stats; return NTK_OK;
    default: return NTK_ERR_BAD_ARG;
    }
}

int ntk_ctx_set_option(ntk_ctx *c, int option, uint64_t value)
{
    if (!c) return NTK_ERR_BAD_ARG;
    switch (option) {
    case NTK_OPT_COMPAT_CHUNK_BYTES:      // 0 = default; below kCompatChunkMin is taken as that
        c->compat_chunk = value == 0 ? kCompatChunkBytes : (value < kCompatChunkMin ? kCompatChunkMin : value);
        return NTK_OK;
    case NTK_OPT_MINIMIZER_CHUNK_BYTES:   // 0 = default; a multiple of 4096, at least 4096
        if (value && value < 4096) return NTK_ERR_BAD_ARG;
        c->minimizer_chunk = value == 0 ? ((uint64_t)256 << 20) : (value & ~(uint64_t)4095);
        return NTK_OK;
    case NTK_OPT_MINIMIZER_ROUTE:
        if (value & ~(uint64_t)(NTK_ROUTE_NO_REGFUSED | NTK_ROUTE_NO_GENERIC | NTK_ROUTE_NO_F64 | NTK_ROUTE_NO_SPECULATION)) return NTK_ERR_BAD_ARG;
        c->route_off = (uint32_t)value;
        return NTK_OK;
    case NTK_OPT_BATCH_WAIT_POLL_US:      // 0 = default (50); NTK_POLL_BLOCK = block in hipEventSynchronize
        c->wait_poll_us = value == 0 ? 50 : (value == NTK_POLL_BLOCK ? 0 : (value > 10000000 ? 10000000 : value));
        return NTK_OK;
    case NTK_OPT_GZ_INMEM_LIMIT_BYTES: c->gz_limit = value; return NTK_OK;
    case NTK_OPT_GZ_STREAM_WINDOW_BYTES: c->gz_window = value; return NTK_OK;
    case NTK_OPT_PIPE_STATS: c->pipe_stats = value; return NTK_OK;
    case NTK_OPT_COPY_STREAMS:            // 0 = default (2); 1 or 2 HIP streams take the pinned batches' H2D copies in turn
        if (value > 2) return NTK_ERR_BAD_ARG;
        c->copy_streams = value ? (uint32_t)value : 2u;
        return NTK_OK;
    case NTK_OPT_COMPAT_PACK_THREADS: {   // 0 = default (8); capped by the hardware threads and 64
        uint64_t v = value ? value : 8;
        const unsigned hw = std::thread::hardware_concurrency();
        if (hw && v > hw) v = hw;
        c->pack_threads = (uint32_t)(v > 64 ? 64 : v);
        return NTK_OK;
    }
    default: return NTK_ERR_BAD_ARG;
    }
}

int ntk_ctx_enable_timing(ntk_ctx *c, int on)
{
    if (!c) return NTK_ERR_BAD_ARG;
    c->timing = on != 0;
    return NTK_OK;
}

int ntk_ctx_scan_time_ms(ntk_ctx *c, double *total_ms, uint64_t *launches)
{
    if (!c || !total_ms) return NTK_ERR_BAD_ARG;
    HIPCHK(hipSetDevice(c->device));
    HIPCHK(hipStreamSynchronize(c->stream));
    double t = 0;
    for (auto &p : c->ev_used) {
        float ms = 0;
        HIPCHK(hipEventElapsedTime(&ms, p.first, p.second));
        t += ms;
        c->ev_free.push_back(p.first); c->ev_free.push_back(p.second);
    }
    if (launches) *launches = c->ev_used.size();
    c->ev_used.clear();
    *total_ms = t;
    return NTK_OK;
}

int ntk_accum_reset(ntk_ctx *c)
{
    if (!c) return NTK_ERR_BAD_ARG;
    HIPCHK(hipSetDevice(c->device));
    HIPCHK(hipMemsetAsync(c->d_acc, 0, NTK_ACC_WORDS * sizeof(uint64_t), c->stream));
    return NTK_OK;
}

static int minimizers_reduce_impl(ntk_ctx *c, const uint8_t *d_seq, const uint8_t *d_qual, uint64_t n, const ntk_params *p, uint32_t w);

int ntk_reduce_device_quality(ntk_ctx *c, const uint8_t *d_seq, const uint8_t *d_qual, uint64_t n, const ntk_params *p)
{
    if (!c) return NTK_ERR_BAD_ARG;
    Mode m;
    int rc = resolve_mode(p, true, &m);
    if (rc) return rc;
    HIPCHK(hipSetDevice(c->device));
    if (p->flags & 0xFFu) return minimizers_reduce_impl(c, d_seq, d_qual, n, p, p->flags & 0xFFu);
    return run_scan(c, d_seq, n, p, m, true, nullptr, nullptr, nullptr, d_qual);
}

int ntk_reduce_device(ntk_ctx *c, const uint8_t *d_seq, uint64_t n, const ntk_params *p)
{
    return ntk_reduce_device_quality(c, d_seq, nullptr, n, p);
}

int ntk_accum_read(ntk_ctx *c, ntk_result *out)
{
    if (!c || !out) return NTK_ERR_BAD_ARG;
    const uint64_t *h = c->h_pinned.p;
    HIPCHK(hipSetDevice(c->device));
    const int rc = c->h_pinned.read(c->stream, c->d_acc, NTK_ACC_WORDS);
    if (rc) return rc;
    out->n_total = h[NTK_ACC_N_TOTAL]; out->n_fwd = h[NTK_ACC_N_FWD]; out->n_rc = h[NTK_ACC_N_RC];
    out->sum = h[NTK_ACC_SUM]; out->xr = h[NTK_ACC_XOR];
    memcpy(out->hist, h + NTK_ACC_HIST, sizeof(out->hist));
    out->n_undigested = h[NTK_ACC_UNDIGESTED];
    return NTK_OK;
}

int ntk_accum_device_ptr(ntk_ctx *c, uint64_t **d_words)
{
    if (!c || !d_words) return NTK_ERR_BAD_ARG;
    *d_words = c->d_acc;
    return NTK_OK;
}

int ntk_accum_bind_device(ntk_ctx *c, uint64_t *d_words)
{
    if (!c || ((uintptr_t)d_words & 7)) return NTK_ERR_BAD_ARG;
    c->d_acc = d_words ? d_words : c->d_acc_own.p;
    return NTK_OK;
}

int ntk_materialize_device_quality(ntk_ctx *c, const uint8_t *d_seq, const uint8_t *d_qual, uint64_t n, const ntk_params *p,
                                   uint64_t *d_values, uint16_t *d_valid16, uint16_t *d_rc16)
{
    if (!c || !d_valid16 || !d_rc16) return NTK_ERR_BAD_ARG;
    Mode m;
    int rc = resolve_mode(p, true, &m);
    if (rc) return rc;
    HIPCHK(hipSetDevice(c->device));
    return run_scan(c, d_seq, n, p, m, false, d_values, d_valid16, d_rc16, d_qual);
}

int ntk_materialize_device(ntk_ctx *c, const uint8_t *d_seq, uint64_t n, const ntk_params *p,
                           uint64_t *d_values, uint16_t *d_valid16, uint16_t *d_rc16)
{
    return ntk_materialize_device_quality(c, d_seq, nullptr, n, p, d_values, d_valid16, d_rc16);
}

/* ---- pinned batches ------------------------------------------------------------------------ */

int ntk_batch_acquire(ntk_ctx *c, uint64_t max_bytes, uint64_t max_records, ntk_batch **out)
{
    if (!c || !out || max_bytes == 0) return NTK_ERR_BAD_ARG;
    *out = nullptr;
    HIPCHK(hipSetDevice(c->device));
    const uint64_t want_bytes = (max_bytes + 1023) & ~(uint64_t)1023, want_records = max_records ? max_records : 1;
    {   // a pooled batch that is large enough, and not more than twice as large as asked for
        std::lock_guard<std::mutex> g(c->pool_mu);
        for (size_t i = 0; i < c->pool.size(); i++) {
            ntk_batch *p = c->pool[i];
            if (p->cap_bytes >= want_bytes && p->cap_bytes <= 2 * want_bytes && p->cap_records >= want_records) {
                c->pool[i] = c->pool.back(); c->pool.pop_back();
                c->pool_bytes -= p->cap_bytes;
                *out = p;
                return NTK_OK;
            }
        }
    }
    ntk_batch *b = new (std::nothrow) ntk_batch();
    if (!b) return NTK_ERR_NOMEM;
    b->cap_bytes = want_bytes;
    b->cap_records = want_records;
    const auto create = [&]() -> int {   // (a fresh array synchronises no stream)
        int rc;
        if ((rc = b->h_seq.alloc(b->cap_bytes)) || (rc = b->h_off.alloc(b->cap_records + 1)) || (rc = b->d_seq.ensure(c->stream, b->cap_bytes, grow_exact))) return rc;
        HIPCHK(hipEventCreateWithFlags(&b->ev_copied, hipEventDisableTiming));
        HIPCHK(hipEventCreateWithFlags(&b->ev_done, hipEventDisableTiming));
        return NTK_OK;
    };
    const int rc = create();
    if (rc) { destroy_batch(b); return rc; }   // (skips what is null)
    b->h_off.p[0] = 0;
    b->device = c->device;
    *out = b;
    return NTK_OK;
}

static int batch_append_impl(ntk_batch *b, const uint8_t *seq, const uint8_t *qual, uint64_t n, uint32_t pre, uint32_t cutoff)
{
    if (!b || (!seq && n) || pre > NTK_PRE_NORMALIZE_IUPAC || b->in_flight) return NTK_ERR_BAD_ARG;
    if (b->n_records >= b->cap_records || b->n_bytes + n + 1 > b->cap_bytes) return NTK_ERR_CAPACITY;
    if (qual && !b->h_qual.p) {
        // quality stream: same capacity and offsets as the sequence stream; records appended without qualities read
        // as 0xFF (never below a cutoff).  The device array first: whichever allocation fails, h_qual stays empty and the batch usable
        // without qualities (d_qual is empty or of this size: no stream is synchronised)
        HIPCHK(hipSetDevice(b->device));
        int rc = b->d_qual.ensure(nullptr, b->cap_bytes, grow_exact);
        if (rc || (rc = b->h_qual.alloc(b->cap_bytes))) return rc;
        memset(b->h_qual.p, 0xFF, b->n_bytes);
    }
    uint8_t *o = b->h_seq.p + b->n_bytes;
    uint8_t *oq = b->h_qual.p ? b->h_qual.p + b->n_bytes : nullptr;
    uint64_t w = 0;
    // the pre-step's deleted class is dropped here together with its quality byte - unless that quality is below the
    // cutoff: the reference masks (base, quality) pairs BEFORE normalize deletes anything (src/sequence.rs:285-296), so
    // such a byte has become an N by then and stays, as a break.  It is kept here and masked on the device.
    // Line by line (memchr for LF): a line without any other byte of the deleted class - the usual case, checked by a
    // branch-free reduction the compiler vectorises - is one memcpy; wrapped FASTA contigs cost a memchr + memcpy per line.
    const bool ws = pre != NTK_PRE_STRIP_RETURNS;
    bool plain = pre == NTK_PRE_NONE;
    if (!plain && n <= 4096) {
        // a short record (a read): ONE branch-free pass says whether any byte of the deleted class is in it at all - the usual answer is no,
        // and the record is one memcpy (the line-by-line walk below costs a memchr and a second pass per line)
        unsigned any = 0;
        for (uint64_t j = 0; j < n; j++) {
            const uint8_t ch = seq[j];
            any |= (unsigned)(ch == '\n') | (unsigned)(ch == '\r') | ((unsigned)ws & ((unsigned)(ch == ' ') | (unsigned)(ch == '\t')));
        }
        plain = !any;
    }
    if (plain) {
        memcpy(o, seq, n); w = n;
        if (oq) { if (qual) memcpy(oq, qual, n); else memset(oq, 0xFF, n); }
    } else {
        uint64_t i = 0;
        while (i < n) {
            const uint8_t *nl = (const uint8_t *)memchr(seq + i, '\n', n - i);
            const uint64_t end = nl ? (uint64_t)(nl - seq) : n;   // line = [i, end), then the LF (if any)
            unsigned any = 0;
            for (uint64_t j = i; j < end; j++) {
                const uint8_t ch = seq[j];
                any |= (unsigned)(ch == '\r') | ((unsigned)ws & ((unsigned)(ch == ' ') | (unsigned)(ch == '\t')));
            }
            if (!any) {
                memcpy(o + w, seq + i, end - i);
                if (oq) { if (qual) memcpy(oq + w, qual + i, end - i); else memset(oq + w, 0xFF, end - i); }
                w += end - i;
            } else {
                for (uint64_t j = i; j < end; j++) {
                    const uint8_t ch = seq[j];
                    if ((ch == '\r' || (ws && (ch == ' ' || ch == '\t'))) && !(qual && qual[j] < cutoff)) continue;
                    if (oq) oq[w] = qual ? qual[j] : (uint8_t)0xFF;
                    o[w++] = ch;
                }
            }
            if (nl && qual && qual[end] < cutoff) {   // a low-quality LF has become an N: it stays (see above)
                if (oq) oq[w] = qual[end];
                o[w++] = '\n';
            }
            i = end + 1;
        }
    }
    if (oq) oq[w] = 0xFF;
    o[w++] = '\n';
    b->n_bytes += w;
    b->n_records += 1;
    b->h_off.p[b->n_records] = b->n_bytes;
    if (qual) { b->has_qual = true; b->qual_cutoff = cutoff; }
    return NTK_OK;
}

int ntk_batch_append(ntk_batch *b, const uint8_t *seq, uint64_t n, uint32_t pre)
{
    return batch_append_impl(b, seq, nullptr, n, pre, 0);
}

int ntk_batch_append_quality(ntk_batch *b, const uint8_t *seq, const uint8_t *qual, uint64_t n, uint32_t pre, uint32_t cutoff)
{
    if ((!qual && n) || cutoff < 1 || cutoff > 255) return NTK_ERR_BAD_ARG;
    if (b && b->has_qual && b->qual_cutoff != cutoff) return NTK_ERR_BAD_ARG;  // one cutoff per fill
    return batch_append_impl(b, seq, qual ? qual : (const uint8_t *)"", n, pre, cutoff);
}

int ntk_batch_buffers(ntk_batch *b, uint8_t **seq, uint64_t **offsets, uint64_t *n_bytes, uint64_t *n_records)
{
    if (!b) return NTK_ERR_BAD_ARG;
    if (seq) *seq = b->h_seq.p;
    if (offsets) *offsets = b->h_off.p;
    if (n_bytes) *n_bytes = b->n_bytes;
    if (n_records) *n_records = b->n_records;
    return NTK_OK;
}

int ntk_batch_submit(ntk_ctx *c, ntk_batch *b, const ntk_params *p)
{
    if (!c || !b || b->in_flight) return NTK_ERR_BAD_ARG;
    Mode m;
    int rc = resolve_mode(p, true, &m);
    if (rc) return rc;
    HIPCHK(hipSetDevice(c->device));
    if (b->n_bytes) {
        const uint64_t padded = (b->n_bytes + 15) & ~(uint64_t)15;
        for (uint64_t i = b->n_bytes; i < padded; i++) b->h_seq.p[i] = '\n';
        hipStream_t cs = (c->copy_streams > 1 && (c->copy_rr++ & 1u)) ? c->copy_stream2 : c->copy_stream;
        HIPCHK(hipMemcpyAsync(b->d_seq.p, b->h_seq.p, padded, hipMemcpyHostToDevice, cs));
        // the quality stream travels only when a cutoff is set and some record of this fill carries qualities
        const uint8_t *d_qual = nullptr;
        if (b->has_qual && quality_cutoff(p) != b->qual_cutoff) return NTK_ERR_BAD_ARG;
        if (quality_cutoff(p) && b->has_qual) {
            for (uint64_t i = b->n_bytes; i < padded; i++) b->h_qual.p[i] = 0xFF;
            HIPCHK(hipMemcpyAsync(b->d_qual.p, b->h_qual.p, padded, hipMemcpyHostToDevice, cs));
            d_qual = b->d_qual.p;
        }
        HIPCHK(hipEventRecord(b->ev_copied, cs));
        HIPCHK(hipStreamWaitEvent(c->stream, b->ev_copied, 0));
        rc = (p->flags & 0xFFu) ? minimizers_reduce_impl(c, b->d_seq.p, d_qual, b->n_bytes, p, p->flags & 0xFFu)
                               : run_scan(c, b->d_seq.p, b->n_bytes, p, m, true, nullptr, nullptr, nullptr, d_qual);
        if (rc) return rc;
    }
    else if (p->flags & NTK_FLAG_RESET) HIPCHK(hipMemsetAsync(c->d_acc, 0, NTK_ACC_WORDS * sizeof(uint64_t), c->stream));
    HIPCHK(hipEventRecord(b->ev_done, c->stream));
    b->in_flight = true;
    return NTK_OK;
}

int ntk_batch_wait(ntk_ctx *c, ntk_batch *b)
{
    if (!c || !b) return NTK_ERR_BAD_ARG;
    if (b->in_flight) {
        // query + sleep rather than hipEventSynchronize: with dozens of parser threads blocked inside the runtime at once, the
        // submitting thread's enqueue calls slowed down 2 - 3 x (48+ threads: 16 instead of 39 Gbases/s, profiles/r02e/pipeline.txt).
        // NTK_OPT_BATCH_WAIT_POLL_US = NTK_POLL_BLOCK restores the blocking wait (values are clamped to 10 s).
        const long poll_us = (long)c->wait_poll_us;
        if (poll_us > 0) {
            for (;;) {
                const hipError_t q = hipEventQuery(b->ev_done);
                if (q == hipSuccess) break;
                if (q != hipErrorNotReady) { g_last_hip = (int)q; return NTK_ERR_HIP; }
                struct timespec ts = {poll_us / 1000000L, (poll_us % 1000000L) * 1000L};   // tv_nsec stays below 1e9
                nanosleep(&ts, nullptr);
            }
        } else HIPCHK(hipEventSynchronize(b->ev_done));
        b->in_flight = false;
    }
    b->n_bytes = 0; b->n_records = 0; b->h_off.p[0] = 0; b->has_qual = false;
    return NTK_OK;
}

void ntk_batch_release(ntk_ctx *c, ntk_batch *b)
{
    if (!b) return;
    if (c) (void)hipSetDevice(c->device);
    if (b->in_flight && b->ev_done) (void)hipEventSynchronize(b->ev_done);
    b->in_flight = false;
    if (c && b->h_seq.p && b->h_off.p && b->d_seq.p) {  // keep it for the next acquire (bounded: 256 batches / 8 GiB pinned)
        std::lock_guard<std::mutex> g(c->pool_mu);
        if (c->pool.size() < 256 && c->pool_bytes + b->cap_bytes <= ((uint64_t)8 << 30)) {
            b->n_bytes = 0; b->n_records = 0; b->h_off.p[0] = 0; b->has_qual = false; b->qual_cutoff = 0;
            c->pool.push_back(b);
            c->pool_bytes += b->cap_bytes;
            return;
        }
    }
    destroy_batch(b);
}

/* ---- compat face ------------------------------------------------------------------------------ */

static int compact_with_lut(ntk_ctx *c, const uint8_t *seq, uint64_t n, const uint16_t *d_lut,
                            uint8_t *out, uint64_t *out_len, uint32_t *flags_out)
{
    flags_out[0] = flags_out[1] = 0;
    *out_len = 0;
    if (n == 0) return NTK_OK;
    HIPCHK(hipSetDevice(c->device));
    const uint32_t nblocks = (uint32_t)((n + kCompactBlockBytes - 1) / kCompactBlockBytes);
    enum { kIn, kOut, kKept, kOffsets };   // scratch slots: input, output, kept per block, offsets + total + flags
    int rc;
    if ((rc = ensure_scratch(c, kIn, n)) || (rc = ensure_scratch(c, kOut, n))) return rc;
    if ((rc = ensure_scratch(c, kKept, (size_t)nblocks * 4 + 16)) || (rc = ensure_scratch(c, kOffsets, (size_t)nblocks * 8 + 64))) return rc;
    uint8_t *d_in = c->scratch_at<uint8_t>(kIn), *d_out = c->scratch_at<uint8_t>(kOut);
    uint32_t *d_kept = c->scratch_at<uint32_t>(kKept);
    uint64_t *d_off = c->scratch_at<uint64_t>(kOffsets);
    uint64_t *d_total = d_off + nblocks;
    uint32_t *d_flags = (uint32_t *)(d_total + 1);
    HIPCHK(hipMemcpyAsync(d_in, seq, n, hipMemcpyHostToDevice, c->stream));
    HIPCHK(hipMemsetAsync(d_total, 0, 16, c->stream));
    hipLaunchKernelGGL(compact_count_kernel, dim3(nblocks), dim3(kCompactThreads), 0, c->stream, (const uint8_t *)d_in, n, d_lut, d_kept, d_flags);
    hipLaunchKernelGGL(compact_scan_kernel, dim3(1), dim3(1024), 0, c->stream, (const uint32_t *)d_kept, d_off, nblocks, d_total);
    hipLaunchKernelGGL(compact_write_kernel, dim3(nblocks), dim3(kCompactThreads), 0, c->stream, (const uint8_t *)d_in, n, d_lut, (const uint64_t *)d_off, d_out);
    HIPCHK(hipGetLastError());
    const uint64_t *h = c->h_pinned.p;
    if ((rc = c->h_pinned.read(c->stream, d_total, 2))) return rc;   // the total, then the two flag words
    const uint64_t total = h[0];
    memcpy(flags_out, h + 1, 8);
    if (total) {
        HIPCHK(hipMemcpyAsync(out, d_out, total, hipMemcpyDeviceToHost, c->stream));
        HIPCHK(hipStreamSynchronize(c->stream));
    }
    *out_len = total;
    return NTK_OK;
}

int ntk_normalize(ntk_ctx *c, const uint8_t *seq, uint64_t n, int allow_iupac, uint8_t *out, uint64_t *out_len, int *changed)
{
    if (!c || (!seq && n) || (!out && n) || !out_len) return NTK_ERR_BAD_ARG;
    uint32_t flags[2];
    int rc = compact_with_lut(c, seq, n, allow_iupac ? c->lut_normalize_iupac() : c->lut_normalize(), out, out_len, flags);
    if (rc) return rc;
    if (changed) *changed = flags[0] ? 1 : 0;
    return NTK_OK;
}

int ntk_strip_returns(ntk_ctx *c, const uint8_t *seq, uint64_t n, uint8_t *out, uint64_t *out_len, int *borrowed)
{
    if (!c || (!seq && n) || (!out && n) || !out_len) return NTK_ERR_BAD_ARG;
    uint32_t flags[2];
    int rc = compact_with_lut(c, seq, n, c->lut_strip(), out, out_len, flags);
    if (rc) return rc;
    if (borrowed) *borrowed = flags[1] ? 0 : 1;
    return NTK_OK;
}

int ntk_reverse_complement(ntk_ctx *c, const uint8_t *seq, uint64_t n, uint8_t *out)
{
    if (!c || (!seq && n) || (!out && n)) return NTK_ERR_BAD_ARG;
    if (n == 0) return NTK_OK;
    HIPCHK(hipSetDevice(c->device));
    enum { kIn, kOut };   // scratch slots
    int rc;
    if ((rc = ensure_scratch(c, kIn, n)) || (rc = ensure_scratch(c, kOut, n))) return rc;
    uint8_t *d_in = c->scratch_at<uint8_t>(kIn), *d_out = c->scratch_at<uint8_t>(kOut);
    HIPCHK(hipMemcpyAsync(d_in, seq, n, hipMemcpyHostToDevice, c->stream));
    hipLaunchKernelGGL(map_reverse_kernel, dim3(grid_for(n, 256)), dim3(256), 0, c->stream,
                       (const uint8_t *)d_in, d_out, n, c->lut_complement());
    HIPCHK(hipGetLastError());
    HIPCHK(hipMemcpyAsync(out, d_out, n, hipMemcpyDeviceToHost, c->stream));
    HIPCHK(hipStreamSynchronize(c->stream));
    return NTK_OK;
}

int ntk_canonical_kmers(ntk_ctx *c, const uint8_t *seq, uint64_t n, uint32_t k, uint64_t *pos_out, uint8_t *is_rc_out,
                        uint64_t cap, uint64_t *count)
{
    // one record through the batched entry point: the items are compacted on the device, only they come back
    if (!c || (!seq && n) || !count) return NTK_ERR_BAD_ARG;
    const uint64_t offsets[2] = {0, n};
    return ntk_canonical_kmers_batch(c, seq, offsets, 1, k, nullptr, pos_out, is_rc_out, cap, count);
}

int ntk_bit_kmers(ntk_ctx *c, const uint8_t *seq, uint64_t n, uint32_t k, int canonical, uint64_t *pos_out,
                  uint64_t *val_out, uint8_t *was_rc_out, uint64_t cap, uint64_t *count)
{
    if (!c || (!seq && n) || !count) return NTK_ERR_BAD_ARG;
    const uint64_t offsets[2] = {0, n};
    return ntk_bit_kmers_batch(c, seq, offsets, 1, k, canonical, nullptr, pos_out, val_out, was_rc_out, cap, count);
}

/* ---- batched compat face ------------------------------------------------------------------------------------------- */
namespace {
// The banks keep their staging and device buffers between calls (re-allocation costs milliseconds); what a call leaves behind above
// this many bytes per bank is released when it returns (a single 10-kb-record batch used to pin ~1.2 GiB until ctx_destroy).
constexpr size_t kBankKeepBytes = (size_t)512 << 20;   // a 16 MiB chunk of the bit path needs ~420 MiB per bank: kept; more than that: released
void bank_trim(ntk_ctx *c, size_t keep = kBankKeepBytes)
{
    for (CompatBank &b : c->bank) {
        size_t dev = 0;
        for (const auto &s : b.d) dev += s.bytes();
        if (dev > keep) for (auto &s : b.d) s.release();
        if (b.h_stage.bytes() > keep) b.h_stage.release();
    }
}

int bank_scratch(ntk_ctx *c, CompatBank &b, BankSlot slot, size_t bytes)
{
    if (bytes < 256) bytes = 256;
    DeviceArray<uint8_t> &s = b.d[slot];
    // All three streams are idle before a bank's buffer is replaced: ensure() synchronises the compute stream ahead of the free, the copy
    // and down streams go first here, on the growing path only.  (Only this bank's own earlier work can still use the buffer, and that
    // was waited for before the bank was re-used.)
    if (bytes > s.cap && s.p) { HIPCHK(hipStreamSynchronize(c->copy_stream)); HIPCHK(hipStreamSynchronize(c->down_stream)); }
    return s.ensure(c->stream, bytes, grow_quarter_again_4k);
}

int bank_init(CompatBank &b)
{
    if (b.ev_ready) return NTK_OK;
    HIPCHK(hipEventCreateWithFlags(&b.ev_ready, hipEventDisableTiming));
    HIPCHK(hipEventCreateWithFlags(&b.ev_computed, hipEventDisableTiming));
    HIPCHK(hipEventCreateWithFlags(&b.ev_landed, hipEventDisableTiming));
    return b.h_total.alloc(8);   // (a 64-byte line)
}

int stream_sync(hipStream_t s) { HIPCHK(hipStreamSynchronize(s)); return NTK_OK; }

// The pipeline every batched Sequence-trait call runs on.  The batch is cut into chunks of <= ntk_ctx::compat_chunk bytes (compat_cut;
// NTK_OPT_COMPAT_CHUNK_BYTES lets the suites force many chunks out of small batches) and chunk i owns bank i % kCompatBanks while it is
// in flight.  A face supplies two bodies that only enqueue:
//     in(bank, cut):  note the chunk in the bank, size the bank's buffers, upload, and whatever must precede the download
//     out(bank):      what is left of the chunk's device work, the download into the caller's arrays, ev_landed recorded, busy = true
// and the host issues in(i + 1) before out(i): while the copy engine drains chunk i, chunk i + 1 is staged and uploaded.  THREE banks
// rotate: a bank is free again when its chunk's download has landed, and with two the host would wait for download(i - 1) - enqueued a
// moment ago - before it could stage chunk i + 1 (measured on the item arrays: 3.85 ms per chunk = 2.35 ms of copies + 1.5 ms of packing
// in series, profiles/r03b/compat_trace.txt).  retired(bank) runs once for every chunk whose download has landed.
// The call is synchronous: everything of it has landed (or, after an error, nothing of it is still reading the pinned staging buffers or
// writing the caller's arrays) when it returns.  The first failing stage's status wins over a failed synchronise.
extern "C++" template <class In, class Out, class Retired>   // (this part of the file sits inside extern "C")
int run_banked(ntk_ctx *c, const uint64_t *offsets, uint64_t n_records, uint64_t per_record, bool downloads_on_down_stream, In in, Out out,
               Retired retired)
{
    int rc = NTK_OK;
    for (CompatBank &b : c->bank) if ((rc = bank_init(b))) return rc;
    auto retire = [&](CompatBank &b) -> int {
        if (!b.busy) return NTK_OK;
        HIPCHK(hipEventSynchronize(b.ev_landed));
        b.busy = false;
        retired(b);
        return NTK_OK;
    };
    CompatBank *prev = nullptr;
    uint64_t ci = 0;
    for (uint64_t r0 = 0; r0 < n_records; ci++) {
        const CompatCut cut = compat_cut(offsets, n_records, r0, c->compat_chunk, per_record);
        CompatBank &b = c->bank[ci % kCompatBanks];
        if ((rc = retire(b)) || (rc = in(b, cut)) || (prev && (rc = out(*prev)))) break;
        prev = &b; r0 = cut.r1;
    }
    if (rc == NTK_OK && prev) rc = out(*prev);
    const int down = downloads_on_down_stream ? stream_sync(c->down_stream) : NTK_OK, compute = stream_sync(c->stream), copy = stream_sync(c->copy_stream);
    if (rc == NTK_OK) rc = down ? down : compute ? compute : copy;
    // (the streams are idle: what was still in flight has landed, no event needs waiting for)
    for (CompatBank &b : c->bank) { if (rc == NTK_OK && b.busy) retired(b); b.busy = false; }
    bank_trim(c);
    return rc;
}

// ---- item arrays -------------------------------------------------------------------------------------------------------------------
// The items of Sequence::canonical_kmers / bit_kmers (reference src/sequence.rs:237-252) for a whole batch of records in ONE call:
//     in:   pack the chunk into pinned memory (one break byte after each record) -> H2D -> scan -> valid / is_rc planes ->
//           count + scan of the items per 16 384-position block -> the chunk's item total to pinned memory            [ctx stream]
//     out:  (total known) scatter into dense (pos, value, flag) arrays + per-record counts                            [ctx stream]
//           -> D2H straight into the caller's arrays at the chunk's item offset                                       [copy stream]
// While the copy engine drains chunk i's items (the 9 B per item going back over PCIe are the bound of this face), the CPU packs chunk
// i + 1 and the GPU scans it.  Caller arrays may be pageable or pinned (ntk_pinned_alloc).
struct CompatJob {
    const uint8_t *seq; const uint64_t *offsets;
    uint32_t k; int kind;   // 0: byte path (raw-byte CanonicalKmers, any k <= 255), 1: bit path canonical, 2: bit path forward
    uint64_t *counts, *pos_out, *val_out; uint8_t *flag_out;
    uint64_t cap;
};

// in: the records of the cut into bank b, up to the item total
int compat_stage_a(ntk_ctx *c, CompatBank &b, const CompatJob &j, const CompatCut &cut)
{
    int rc;
    const uint64_t r0 = cut.r0, nrec = cut.nrec(), n = cut.bytes;
    const size_t stage_bytes = (size_t)n + (size_t)(nrec + 1) * 8 + 64;
    if ((rc = b.h_stage.ensure(stage_bytes, grow_quarter_again))) return rc;   // (the bank is free: nothing of it is in flight)
    uint64_t *h_start = (uint64_t *)b.h_stage.p;                     // 8-byte aligned head
    uint8_t *h_seq = b.h_stage.p + (size_t)(nrec + 1) * 8;
    // record r of the chunk lands at offsets[r0 + r] - offsets[r0] + r (one break byte after every record before it): the
    // packing splits over threads without a prefix pass (one core packs ~5 GB/s of 150-byte records - less than the PCIe link
    // takes back - so a chunk is packed by up to ntk_ctx::pack_threads threads, default 8)
    const uint64_t o0 = j.offsets[r0];
    auto pack = [&](uint64_t ra, uint64_t rb) {
        for (uint64_t r = ra; r < rb; r++) {
            const uint64_t o = j.offsets[r0 + r], len = j.offsets[r0 + r + 1] - o, w = o - o0 + r;
            h_start[r] = w;
            if (len) memcpy(h_seq + w, j.seq + o, len);
            h_seq[w + len] = '\n';
        }
    };
    const unsigned nth = (unsigned)std::min<uint64_t>(c->pack_threads, n / (256 << 10) + 1);   // a thread per 256 KiB at least
    if (nth <= 1) pack(0, nrec);
    else {
        // a thread that cannot be created (thread / cgroup limit: std::system_error, bad_alloc) must not unwind across the C ABI:
        // the records it would have packed are packed here instead
        std::vector<std::thread> th;
        uint64_t done_to = nrec / nth;            // [0, done_to) is this thread's own share
        uint64_t spawned_from = nrec;             // [spawned_from, nrec) went to threads
        try {
            th.reserve(nth - 1);
            for (unsigned t = nth - 1; t >= 1; t--) {   // from the back, so that what is left over stays one contiguous range
                th.emplace_back(pack, nrec * t / nth, nrec * (t + 1) / nth);
                spawned_from = nrec * t / nth;
            }
        } catch (...) {}
        pack(0, spawned_from < done_to ? spawned_from : done_to);
        if (spawned_from > done_to) pack(done_to, spawned_from);
        for (auto &t : th) t.join();
    }
    h_start[nrec] = n;
    b.r0 = r0; b.nrec = nrec; b.n = n;
    const uint64_t nt = (n + 15) / 16 * 16;
    if ((rc = bank_scratch(c, b, kSlotBytes, nt + 16))) return rc;
    if ((rc = bank_scratch(c, b, kSlotOffsets, (size_t)(nrec + 1) * 8))) return rc;
    if ((rc = bank_scratch(c, b, j.kind == 0 ? kSlotFlags : kSlotValues, j.kind == 0 ? nt : nt * 8))) return rc;
    if ((rc = bank_scratch(c, b, kSlotValid, nt / 8 + 16))) return rc;
    if ((rc = bank_scratch(c, b, kSlotRc, nt / 8 + 16))) return rc;
    b.n_words = (n + 15) >> 4;
    b.nblocks = (b.n_words + kCpBlockWords - 1) / kCpBlockWords;
    b.o_off = ((size_t)b.nblocks * 4 + 7) & ~(size_t)7; b.o_total = b.o_off + (size_t)b.nblocks * 8; b.o_counts = b.o_total + 8;
    if ((rc = bank_scratch(c, b, kSlotCompaction, b.o_counts + (size_t)nrec * 8))) return rc;
    const uint8_t *d_bytes = b.at<uint8_t>(kSlotBytes);
    HIPCHK(hipMemcpyAsync(b.at<uint8_t>(kSlotBytes), h_seq, n, hipMemcpyHostToDevice, c->stream));
    HIPCHK(hipMemcpyAsync(b.at<uint64_t>(kSlotOffsets), h_start, (size_t)(nrec + 1) * 8, hipMemcpyHostToDevice, c->stream));
    uint16_t *d_v16 = b.at<uint16_t>(kSlotValid), *d_r16 = b.at<uint16_t>(kSlotRc);
    if (j.kind == 0) {
        // raw-byte comparison exactly as the reference (src/kmer.rs:84-129): any k <= 255, mixed case compares as bytes
        uint8_t *d_flags = b.at<uint8_t>(kSlotFlags);
        hipLaunchKernelGGL(canonical_bytes_kernel, dim3(grid_for(n, 256)), dim3(256), 0, c->stream,
                           d_bytes, n, j.k, c->lut_complement(), d_flags, (const uint32_t *)nullptr);
        hipLaunchKernelGGL(pack_flags8_kernel, dim3(grid_for((n + 15) / 16, 256)), dim3(256), 0, c->stream, (const uint8_t *)d_flags, n, d_v16, d_r16);
        HIPCHK(hipGetLastError());
    } else {
        const ntk_params p = {j.k, (uint32_t)(j.kind == 1 ? NTK_PATH_BITS_CANONICAL : NTK_PATH_BITS), NTK_PRE_NONE, 0};
        if ((rc = ntk_materialize_device(c, d_bytes, n, &p, b.at<uint64_t>(kSlotValues), d_v16, d_r16))) return rc;
    }
    uint8_t *base = b.at<uint8_t>(kSlotCompaction);
    hipLaunchKernelGGL(cp_count_kernel, dim3((unsigned)b.nblocks), dim3(kCpThreads), 0, c->stream, d_v16, b.n_words, (uint32_t *)base);
    hipLaunchKernelGGL(cp_scan_kernel, dim3(1), dim3(1024), 0, c->stream, (const uint32_t *)base, (uint64_t *)(base + b.o_off), b.nblocks,
                       (uint64_t *)(base + b.o_total));
    HIPCHK(hipGetLastError());
    HIPCHK(hipMemcpyAsync(b.h_total.p, base + b.o_total, 8, hipMemcpyDeviceToHost, c->stream));
    HIPCHK(hipEventRecord(b.ev_ready, c->stream));
    return NTK_OK;
}

// out: the chunk's items leave for the caller's arrays at item offset *base (capacity permitting); *base += the chunk's item total
int compat_stage_b(ntk_ctx *c, CompatBank &b, const CompatJob &j, uint64_t *base_items)
{
    int rc;
    HIPCHK(hipEventSynchronize(b.ev_ready));
    const uint64_t m = *b.h_total.p, at = *base_items;
    const uint64_t take = at >= j.cap ? 0 : (m < j.cap - at ? m : j.cap - at);
    const bool values = j.kind != 0;
    if ((rc = bank_scratch(c, b, kSlotDense, (size_t)take * (8 + (values ? 8 : 0) + 1) + 64))) return rc;
    uint64_t *d_pos = b.at<uint64_t>(kSlotDense), *d_val = values ? d_pos + take : nullptr;
    uint8_t *d_flag = (uint8_t *)(d_pos + take + (values ? take : 0));
    uint8_t *sb = b.at<uint8_t>(kSlotCompaction);
    uint64_t *d_counts = (uint64_t *)(sb + b.o_counts);
    HIPCHK(hipMemsetAsync(d_counts, 0, (size_t)b.nrec * 8, c->stream));
    hipLaunchKernelGGL(cp_scatter_kernel, dim3((unsigned)b.nblocks), dim3(kCpThreads), 0, c->stream, b.at<const uint16_t>(kSlotValid), b.at<const uint16_t>(kSlotRc),
                       values ? b.at<const uint64_t>(kSlotValues) : nullptr, b.n_words, (const uint64_t *)(sb + b.o_off), b.at<const uint64_t>(kSlotOffsets), b.nrec,
                       j.kind == 0 ? 0u : j.k - 1, take, d_pos, d_val, d_flag, (unsigned long long *)d_counts);
    HIPCHK(hipGetLastError());
    HIPCHK(hipEventRecord(b.ev_computed, c->stream));
    HIPCHK(hipStreamWaitEvent(c->copy_stream, b.ev_computed, 0));
    if (j.counts) HIPCHK(hipMemcpyAsync(j.counts + b.r0, d_counts, (size_t)b.nrec * 8, hipMemcpyDeviceToHost, c->copy_stream));
    if (take && j.pos_out) HIPCHK(hipMemcpyAsync(j.pos_out + at, d_pos, (size_t)take * 8, hipMemcpyDeviceToHost, c->copy_stream));
    if (take && j.val_out && d_val) HIPCHK(hipMemcpyAsync(j.val_out + at, d_val, (size_t)take * 8, hipMemcpyDeviceToHost, c->copy_stream));
    if (take && j.flag_out) HIPCHK(hipMemcpyAsync(j.flag_out + at, d_flag, (size_t)take, hipMemcpyDeviceToHost, c->copy_stream));
    HIPCHK(hipEventRecord(b.ev_landed, c->copy_stream));
    b.busy = true;
    *base_items = at + m;
    return NTK_OK;
}

int compat_batch(ntk_ctx *c, const CompatJob &j, uint64_t n_records, uint64_t *total)
{
    for (uint64_t r = 0; r < n_records; r++) if (j.offsets[r] > j.offsets[r + 1]) return NTK_ERR_BAD_ARG;
    uint64_t items = 0;
    const int rc = run_banked(c, j.offsets, n_records, 1, false,
                              [&](CompatBank &b, const CompatCut &cut) { return compat_stage_a(c, b, j, cut); },
                              [&](CompatBank &b) { return compat_stage_b(c, b, j, &items); }, [](CompatBank &) {});
    if (rc != NTK_OK) return rc;
    *total = items;
    return items > j.cap ? NTK_ERR_CAPACITY : NTK_OK;
}

// ---- bit-plane form of the byte-path items -----------------------------------------------------------------------------------
// Sequence::canonical_kmers yields (pos, slice, is_rc) (reference src/kmer.rs:114-129); slice and pos follow from the window's place,
// so all the device has to return is, per window start, "emitted?" and "is_rc?": TWO BITS per sequence byte instead of nine bytes per
// item (the bound of ntk_canonical_kmers_batch: 48 GB/s of items over PCIe = 6.3 Gbases/s).  The caller's bytes are uploaded as they
// lie (no packing pass, no break bytes: record starts travel as a bitmap built on the device from the offsets), the raw-byte kernel
// of the compat face marks the windows, and the two planes come back: 1/4 byte per input byte.  Three stages per chunk on three streams:
// in = upload [copy stream]; out = bitmap + planes kernel [ctx stream] -> download [down stream].  The uploads run back to back (the call
// is bound by them); the kernel and the download of chunk i hide behind the upload of chunk i + 1.  Each chunk starts on a 16-position
// word boundary of the planes; rec_bit[r] is the plane position of record r's first byte.
// kind 0: the byte path (CanonicalKmers, raw-byte compare, any k <= 255); 1 / 2: the bit path, canonical / forward-only (BitNuclKmer, k <= 32),
// with values != nullptr also the items' packed values, one u64 per plane position (0 where nothing is emitted): 8 more bytes per input byte
// come back then, and the download is the call's bound.
int compat_planes(ntk_ctx *c, const uint8_t *seq, const uint64_t *offsets, uint64_t n_records, uint32_t k, uint64_t *rec_bit,
                  uint16_t *valid16, uint16_t *rc16, uint64_t cap_words, uint64_t *n_words, uint64_t *total, int kind = 0, uint64_t *values = nullptr)
{
    for (uint64_t r = 0; r < n_records; r++) if (offsets[r] > offsets[r + 1]) return NTK_ERR_BAD_ARG;
    // pass 1 (host): the words the chunks need
    uint64_t words = 0;
    for (uint64_t r0 = 0; r0 < n_records;) {
        const CompatCut cut = compat_cut(offsets, n_records, r0, c->compat_chunk, 0);
        words += (cut.bytes + 15) >> 4;
        r0 = cut.r1;
    }
    *n_words = words;
    if (words > cap_words) return NTK_ERR_CAPACITY;
    uint64_t items = 0, wbase = 0;
    auto upload = [&](CompatBank &b, const CompatCut &cut) -> int {
        const uint64_t nrec = cut.nrec(), nt = (cut.bytes + 15) / 16 * 16;
        b.r0 = cut.r0; b.nrec = nrec; b.n = cut.bytes; b.wbase = wbase;
        wbase += nt >> 4;
        for (uint64_t q = cut.r0; q < cut.r1; q++) rec_bit[q] = b.wbase * 16 + (offsets[q] - offsets[cut.r0]);
        if (b.n == 0) return NTK_OK;   // only empty records
        int r;
        if ((r = bank_scratch(c, b, kSlotBytes, nt + 16))) return r;
        if ((r = bank_scratch(c, b, kSlotOffsets, (size_t)(nrec + 1) * 8))) return r;
        if ((r = bank_scratch(c, b, kSlotValid, nt / 8 + 16))) return r;
        if ((r = bank_scratch(c, b, kSlotRc, nt / 8 + 16))) return r;
        if ((r = bank_scratch(c, b, kSlotTotal, 64))) return r;
        if ((r = bank_scratch(c, b, kSlotStartBits, (size_t)((nt >> 5) + 2) * 4))) return r;
        if (values && (r = bank_scratch(c, b, kSlotValues, (size_t)nt * 8))) return r;
        HIPCHK(hipMemcpyAsync(b.at<uint8_t>(kSlotBytes), seq + offsets[b.r0], b.n, hipMemcpyHostToDevice, c->copy_stream));
        HIPCHK(hipMemcpyAsync(b.at<uint64_t>(kSlotOffsets), offsets + b.r0, (size_t)(nrec + 1) * 8, hipMemcpyHostToDevice, c->copy_stream));
        HIPCHK(hipEventRecord(b.ev_ready, c->copy_stream));
        return NTK_OK;
    };
    auto compute_and_download = [&](CompatBank &b) -> int {
        if (b.n == 0) return NTK_OK;
        const uint64_t nrec = b.nrec, nb = b.n, nt = (nb + 15) / 16 * 16, nw = nt >> 4, sb_words = (nt >> 5) + 2;
        const uint8_t *d_bytes = b.at<uint8_t>(kSlotBytes);
        uint32_t *d_starts = b.at<uint32_t>(kSlotStartBits);
        uint16_t *d_v16 = b.at<uint16_t>(kSlotValid), *d_r16 = b.at<uint16_t>(kSlotRc);
        uint64_t *d_values = values ? b.at<uint64_t>(kSlotValues) : nullptr;
        unsigned long long *d_total = b.at<unsigned long long>(kSlotTotal);
        HIPCHK(hipStreamWaitEvent(c->stream, b.ev_ready, 0));
        HIPCHK(hipMemsetAsync(d_starts, 0, (size_t)sb_words * 4, c->stream));
        HIPCHK(hipMemsetAsync(d_total, 0, 8, c->stream));
        hipLaunchKernelGGL(mark_record_starts_kernel, dim3(grid_for(nrec, 256)), dim3(256), 0, c->stream, b.at<const uint64_t>(kSlotOffsets), nrec, nb, d_starts);
        const uint64_t tiles = (nb + kPlTile - 1) / kPlTile;
        const dim3 grid((unsigned)(tiles < (uint64_t)c->n_cu * 8 ? tiles : (uint64_t)c->n_cu * 8));
        if (kind == 0)
            hipLaunchKernelGGL(canonical_bytes_planes_kernel, grid, dim3(kPlThreads), 0, c->stream, d_bytes, nb, nt + 16, k, c->lut_complement(),
                               (const uint32_t *)d_starts, sb_words, d_v16, d_r16, d_total);
        else if (kind == 1)
            hipLaunchKernelGGL(bit_kmers_planes_kernel<true>, grid, dim3(kPlThreads), 0, c->stream, d_bytes, nb, nt + 16, k,
                               (const uint32_t *)d_starts, sb_words, d_v16, d_r16, d_values, d_total);
        else
            hipLaunchKernelGGL(bit_kmers_planes_kernel<false>, grid, dim3(kPlThreads), 0, c->stream, d_bytes, nb, nt + 16, k,
                               (const uint32_t *)d_starts, sb_words, d_v16, d_r16, d_values, d_total);
        HIPCHK(hipGetLastError());
        HIPCHK(hipMemcpyAsync(b.h_total.p, d_total, 8, hipMemcpyDeviceToHost, c->stream));
        HIPCHK(hipEventRecord(b.ev_computed, c->stream));
        HIPCHK(hipStreamWaitEvent(c->down_stream, b.ev_computed, 0));
        HIPCHK(hipMemcpyAsync(valid16 + b.wbase, d_v16, (size_t)nw * 2, hipMemcpyDeviceToHost, c->down_stream));
        HIPCHK(hipMemcpyAsync(rc16 + b.wbase, d_r16, (size_t)nw * 2, hipMemcpyDeviceToHost, c->down_stream));
        if (values) HIPCHK(hipMemcpyAsync(values + b.wbase * 16, d_values, (size_t)nw * 16 * 8, hipMemcpyDeviceToHost, c->down_stream));
        HIPCHK(hipEventRecord(b.ev_landed, c->down_stream));
        b.busy = true;
        return NTK_OK;
    };
    // a chunk that has fully landed: its item total joins the sum
    const int rc = run_banked(c, offsets, n_records, 0, true, upload, compute_and_download, [&](CompatBank &b) { items += *b.h_total.p; });
    rec_bit[n_records] = words * 16;
    if (rc != NTK_OK) return rc;
    *total = items;
    return NTK_OK;
}

// sequence::minimizer per record (ntk_minimizer_batch): the same three stages on three streams as compat_planes - upload [copy stream]
// -> wave-per-record kernel [ctx stream] -> download of the chunk's minimizers / window starts / strands [down stream].
int minimizer_batch_impl(ntk_ctx *c, const uint8_t *seq, const uint64_t *offsets, uint64_t n_records, uint32_t m, uint8_t *out, uint64_t *pos_out,
                         uint8_t *is_rc_out)
{
    const uint16_t *comp = c->lut_complement();
    auto upload = [&](CompatBank &b, const CompatCut &cut) -> int {
        const uint64_t nrec = cut.nrec();
        b.r0 = cut.r0; b.nrec = nrec; b.n = cut.bytes;
        int r;
        if ((r = bank_scratch(c, b, kSlotBytes, b.n + 16))) return r;
        if ((r = bank_scratch(c, b, kSlotOffsets, (size_t)(nrec + 1) * 8))) return r;
        if ((r = bank_scratch(c, b, kSlotMinBytes, (size_t)nrec * m))) return r;
        if ((r = bank_scratch(c, b, kSlotMinPos, (size_t)nrec * 8))) return r;
        if ((r = bank_scratch(c, b, kSlotMinStrand, (size_t)nrec))) return r;
        if ((r = bank_scratch(c, b, kSlotBest, 64))) return r;
        HIPCHK(hipMemcpyAsync(b.at<uint8_t>(kSlotBytes), seq + offsets[b.r0], b.n, hipMemcpyHostToDevice, c->copy_stream));
        HIPCHK(hipMemcpyAsync(b.at<uint64_t>(kSlotOffsets), offsets + b.r0, (size_t)(nrec + 1) * 8, hipMemcpyHostToDevice, c->copy_stream));
        HIPCHK(hipEventRecord(b.ev_ready, c->copy_stream));
        return NTK_OK;
    };
    auto compute_and_download = [&](CompatBank &b) -> int {
        const uint64_t nrec = b.nrec;
        const uint8_t *d_bytes = b.at<uint8_t>(kSlotBytes);
        uint8_t *d_min = b.at<uint8_t>(kSlotMinBytes), *d_strand = b.at<uint8_t>(kSlotMinStrand);
        uint64_t *d_pos = b.at<uint64_t>(kSlotMinPos);
        HIPCHK(hipStreamWaitEvent(c->stream, b.ev_ready, 0));
        HIPCHK(hipMemsetAsync(b.at<uint64_t>(kSlotBest), 0xFF, 8, c->stream));
        const uint64_t blocks = (nrec + 3) / 4;
        hipLaunchKernelGGL(minimizer_batch_kernel, dim3((unsigned)(blocks < (uint64_t)c->n_cu * 16 ? blocks : (uint64_t)c->n_cu * 16)), dim3(256), 0, c->stream,
                           d_bytes, b.at<const uint64_t>(kSlotOffsets), nrec, m, kLongRecord, comp, d_min, d_pos, d_strand, b.at<unsigned long long>(kSlotBest));
        for (uint64_t r = b.r0; r < b.r0 + nrec; r++) {   // the rare long record: the one-block kernel of ntk_minimizer, on the uploaded bytes
            const uint64_t n = offsets[r + 1] - offsets[r];
            if (n <= kLongRecord) continue;
            const uint8_t *rec = d_bytes + (offsets[r] - offsets[b.r0]);
            uint64_t *d_best = b.at<uint64_t>(kSlotBest) + 1;
            hipLaunchKernelGGL(minimizer_bytes_kernel, dim3(1), dim3(1024), 0, c->stream, rec, n, m, comp, d_best);
            hipLaunchKernelGGL(minimizer_emit_record_kernel, dim3((m + 255) / 256), dim3(256), 0, c->stream, rec, n, m, comp, (const uint64_t *)d_best, r - b.r0,
                               d_min, d_pos, d_strand);
        }
        HIPCHK(hipGetLastError());
        HIPCHK(hipEventRecord(b.ev_computed, c->stream));
        HIPCHK(hipStreamWaitEvent(c->down_stream, b.ev_computed, 0));
        HIPCHK(hipMemcpyAsync(out + b.r0 * m, d_min, (size_t)nrec * m, hipMemcpyDeviceToHost, c->down_stream));
        if (pos_out) HIPCHK(hipMemcpyAsync(pos_out + b.r0, d_pos, (size_t)nrec * 8, hipMemcpyDeviceToHost, c->down_stream));
        if (is_rc_out) HIPCHK(hipMemcpyAsync(is_rc_out + b.r0, d_strand, (size_t)nrec, hipMemcpyDeviceToHost, c->down_stream));
        HIPCHK(hipEventRecord(b.ev_landed, c->down_stream));
        b.busy = true;
        return NTK_OK;
    };
    return run_banked(c, offsets, n_records, 0, true, upload, compute_and_download, [](CompatBank &) {});
}
}  // namespace

int ntk_canonical_kmers_batch_planes(ntk_ctx *c, const uint8_t *seq, const uint64_t *offsets, uint64_t n_records, uint32_t k,
                                     uint64_t *rec_bit, uint16_t *valid16, uint16_t *rc16, uint64_t cap_words, uint64_t *n_words,
                                     uint64_t *total)
{
    if (!c || !offsets || !rec_bit || !n_words || !total || (!seq && offsets[n_records] > offsets[0])) return NTK_ERR_BAD_ARG;
    if (k < 1 || k > 255) return NTK_ERR_BAD_K;
    *total = 0; *n_words = 0;
    rec_bit[0] = 0;
    if (n_records == 0) return NTK_OK;
    if ((!valid16 || !rc16) && cap_words) return NTK_ERR_BAD_ARG;
    HIPCHK(hipSetDevice(c->device));
    return compat_planes(c, seq, offsets, n_records, k, rec_bit, valid16, rc16, cap_words, n_words, total);
}

int ntk_bit_kmers_batch_planes(ntk_ctx *c, const uint8_t *seq, const uint64_t *offsets, uint64_t n_records, uint32_t k, int canonical,
                               uint64_t *rec_bit, uint16_t *valid16, uint16_t *rc16, uint64_t *values, uint64_t cap_words, uint64_t *n_words,
                               uint64_t *total)
{
    if (!c || !offsets || !rec_bit || !n_words || !total || (!seq && offsets[n_records] > offsets[0])) return NTK_ERR_BAD_ARG;
    if (k < 1 || k > 32) return NTK_ERR_BAD_K;
    *total = 0; *n_words = 0;
    rec_bit[0] = 0;
    if (n_records == 0) return NTK_OK;
    if ((!valid16 || !rc16) && cap_words) return NTK_ERR_BAD_ARG;
    HIPCHK(hipSetDevice(c->device));
    return compat_planes(c, seq, offsets, n_records, k, rec_bit, valid16, rc16, cap_words, n_words, total, canonical ? 1 : 2, values);
}

int ntk_bit_kmers_batch(ntk_ctx *c, const uint8_t *seq, const uint64_t *offsets, uint64_t n_records, uint32_t k, int canonical,
                        uint64_t *counts, uint64_t *pos_out, uint64_t *val_out, uint8_t *was_rc_out, uint64_t cap, uint64_t *total)
{
    if (!c || !offsets || !total || (!seq && offsets[n_records] > offsets[0])) return NTK_ERR_BAD_ARG;
    if (k < 1 || k > 32) return NTK_ERR_BAD_K;
    *total = 0;
    if (counts) memset(counts, 0, (size_t)n_records * 8);
    if (n_records == 0) return NTK_OK;
    HIPCHK(hipSetDevice(c->device));
    const CompatJob j = {seq, offsets, k, canonical ? 1 : 2, counts, pos_out, val_out, was_rc_out, cap};
    return compat_batch(c, j, n_records, total);
}

int ntk_canonical_kmers_batch(ntk_ctx *c, const uint8_t *seq, const uint64_t *offsets, uint64_t n_records, uint32_t k,
                              uint64_t *counts, uint64_t *pos_out, uint8_t *is_rc_out, uint64_t cap, uint64_t *total)
{
    if (!c || !offsets || !total || (!seq && offsets[n_records] > offsets[0])) return NTK_ERR_BAD_ARG;
    if (k < 1 || k > 255) return NTK_ERR_BAD_K;
    *total = 0;
    if (counts) memset(counts, 0, (size_t)n_records * 8);
    if (n_records == 0) return NTK_OK;
    HIPCHK(hipSetDevice(c->device));
    const CompatJob j = {seq, offsets, k, 0, counts, pos_out, nullptr, is_rc_out, cap};
    return compat_batch(c, j, n_records, total);
}

/* Page-locked host memory for the arrays the batched calls read and fill (what a Rust host would back its Vecs with): copies to
 * and from it run at the PCIe rate without a staging pass. */
int ntk_pinned_alloc(uint64_t bytes, void **out)
{
    if (!out || bytes == 0) return NTK_ERR_BAD_ARG;
    *out = nullptr;
    HIPCHK(hipHostMalloc(out, (size_t)bytes, hipHostMallocDefault));
    return NTK_OK;
}
void ntk_pinned_free(void *p) { if (p) (void)hipHostFree(p); }

/* Gives back what the batched compat calls keep between calls (three banks of pinned staging and device buffers: up to ~180 MiB each
 * on the byte path, ~420 MiB on the bit path) and the ctx's scratch buffers.  The next call re-allocates. */
int ntk_ctx_trim(ntk_ctx *c)
{
    if (!c) return NTK_ERR_BAD_ARG;
    HIPCHK(hipSetDevice(c->device));
    HIPCHK(hipStreamSynchronize(c->stream));
    HIPCHK(hipStreamSynchronize(c->copy_stream));
    HIPCHK(hipStreamSynchronize(c->down_stream));
    bank_trim(c, 0);
    for (auto &s : c->scratch) s.release();
    return NTK_OK;
}

/* ---- minimizers, quality mask --------------------------------------------------------------------------------- */

static int minimizers_reduce_impl(ntk_ctx *c, const uint8_t *d_seq, const uint8_t *d_qual, uint64_t n, const ntk_params *p, uint32_t w);

int ntk_minimizers_reduce_device(ntk_ctx *c, const uint8_t *d_seq, uint64_t n, const ntk_params *p, uint32_t w)
{
    return minimizers_reduce_impl(c, d_seq, nullptr, n, p, w);
}

static int minimizers_reduce_impl(ntk_ctx *c, const uint8_t *d_seq, const uint8_t *d_qual, uint64_t n, const ntk_params *p, uint32_t w)
{
    if (!c || w < 1 || w > 256) return NTK_ERR_BAD_ARG;
    enum { kValues = 3, kValid = 4, kRc = 5 };   // scratch slots of the two-pass route: a value per position and the two planes
    Mode m;
    int rc = resolve_mode(p, true, &m);
    if (rc) return rc;
    if (!m.canon) return NTK_ERR_BAD_ARG;
    if (m.raw_bytes) return p->k > 32 ? NTK_ERR_BAD_K : NTK_ERR_UNSUPPORTED;   // windowed minimizers are defined on normalised input (values, not raw bytes)
    HIPCHK(hipSetDevice(c->device));
    // fused build (one pass, nothing written to HBM) where one exists - with a quality stream: the quality-masked builds
    if (n) {
        const bool masked = d_qual && quality_cutoff(p);
        const void *fn = (c->route_off & NTK_ROUTE_NO_REGFUSED) ? nullptr : pick_scan_min(m, p->k, w, masked);   // (route bits: ntk_ctx_set_option)
        if (fn)
            return run_scan(c, d_seq, n, p, m, true, nullptr, nullptr, nullptr, masked ? d_qual : nullptr, fn, w);
        // every other (k <= 31, w <= 49): the generic fused kernel (one pass as well, run-time k and w)
        if (p->k <= 31 && w <= 49 && !(c->route_off & NTK_ROUTE_NO_GENERIC))
            return run_min_scan(c, d_seq, n, p, m, w, masked ? d_qual : nullptr);
    }
    if (p->flags & NTK_FLAG_RESET) HIPCHK(hipMemsetAsync(c->d_acc, 0, NTK_ACC_WORDS * sizeof(uint64_t), c->stream));
    if (n == 0) return NTK_OK;
    // Long inputs are scanned in chunks so that the scratch planes stay bounded (8 B per position: 2 GiB for the default
    // 256 MiB chunk instead of 80 GB for a 10 GB batch).  A chunk is scanned together with the w+k-2 bytes of left context
    // before it (start rounded down to the 16-byte alignment of the scan); only windows ENDING inside the chunk are counted.
    const uint64_t chunk = c->minimizer_chunk;
    const uint64_t back = (uint64_t)w + p->k - 2;
    const int blocks = c->n_cu * 4;  // ~35 KiB of LDS per block
    if ((rc = ensure_partials(c, blocks))) return rc;
    ScanArgs a; memset(&a, 0, sizeof(a)); scan_args_set_k(a, p->k);
    for (uint64_t c0 = 0; c0 < n; c0 += chunk) {
        const uint64_t c1 = c0 + chunk < n ? c0 + chunk : n;
        const uint64_t start = c0 > back ? (c0 - back) & ~(uint64_t)15 : 0;
        const uint64_t n_sub = c1 - start, nt = (n_sub + 15) / 16 * 16;
        if ((rc = ensure_scratch(c, kValues, nt * 8)) || (rc = ensure_scratch(c, kValid, nt / 8 + 16)) || (rc = ensure_scratch(c, kRc, nt / 8 + 16))) return rc;
        uint64_t *d_val = c->scratch_at<uint64_t>(kValues);
        uint16_t *d_v16 = c->scratch_at<uint16_t>(kValid), *d_r16 = c->scratch_at<uint16_t>(kRc);
        if ((rc = run_scan(c, d_seq + start, n_sub, p, m, false, d_val, d_v16, d_r16, d_qual ? d_qual + start : nullptr))) return rc;
#define NTK_WM(WW)                                                                                                    \
    case WW:                                                                                                          \
        hipLaunchKernelGGL(window_min_reduce_kernel<WW>, dim3(blocks), dim3(kWmThreads), 0, c->stream, (const uint64_t *)d_val, \
                           (const uint16_t *)d_v16, (const uint16_t *)d_r16, n_sub, w, a.bin_shift, c->d_part_hist.p,  \
                           c->d_part_scalars.p, c0 - start);                                                          \
        break;
        switch (w <= 16 ? w : 0u) {   // compile-time windows up to 16 (register van Herk), the run-time walk otherwise
            NTK_WM(2) NTK_WM(3) NTK_WM(4) NTK_WM(5) NTK_WM(6) NTK_WM(7) NTK_WM(8) NTK_WM(9) NTK_WM(10) NTK_WM(11) NTK_WM(12)
            NTK_WM(13) NTK_WM(14) NTK_WM(15) NTK_WM(16)
        default:
            hipLaunchKernelGGL(window_min_reduce_kernel<0>, dim3(blocks), dim3(kWmThreads), 0, c->stream, (const uint64_t *)d_val,
                               (const uint16_t *)d_v16, (const uint16_t *)d_r16, n_sub, w, a.bin_shift, c->d_part_hist.p,
                               c->d_part_scalars.p, c0 - start);
        }
#undef NTK_WM
        if ((rc = launch_fold(c, blocks))) return rc;   // (no work counters to re-arm: the materialise scan left them dirty)
    }
    return NTK_OK;
}

int ntk_minimizer(ntk_ctx *c, const uint8_t *seq, uint64_t n, uint32_t m, uint8_t *out)
{
    if (!c || !seq || !out || m < 1 || n < m) return NTK_ERR_BAD_ARG;  // the reference panics on n < m (sequence.rs:141)
    HIPCHK(hipSetDevice(c->device));
    enum { kIn, kOut };   // scratch slots; kOut: the m bytes, then (16-byte aligned) the `best` word
    int rc;
    if ((rc = ensure_scratch(c, kIn, n)) || (rc = ensure_scratch(c, kOut, (size_t)m + 64))) return rc;
    uint8_t *d_in = c->scratch_at<uint8_t>(kIn), *d_out = c->scratch_at<uint8_t>(kOut);
    uint64_t *d_best = (uint64_t *)(d_out + ((m + 15) & ~15u));
    HIPCHK(hipMemcpyAsync(d_in, seq, n, hipMemcpyHostToDevice, c->stream));
    hipLaunchKernelGGL(minimizer_bytes_kernel, dim3(1), dim3(1024), 0, c->stream, (const uint8_t *)d_in, n, m,
                       c->lut_complement(), d_best);
    hipLaunchKernelGGL(minimizer_emit_kernel, dim3((m + 255) / 256), dim3(256), 0, c->stream, (const uint8_t *)d_in, n, m,
                       c->lut_complement(), (const uint64_t *)d_best, d_out);
    HIPCHK(hipGetLastError());
    HIPCHK(hipMemcpyAsync(out, d_out, m, hipMemcpyDeviceToHost, c->stream));
    HIPCHK(hipStreamSynchronize(c->stream));
    return NTK_OK;
}

/* sequence::minimizer for every record of a reader batch in one call: chunks of <= 16 MiB uploaded back to back, one wave per record (one
 * block for a record beyond 64 KiB), the chunk's n x m bytes (+ the optional window starts and strands) downloaded behind the next upload. */
int ntk_minimizer_batch(ntk_ctx *c, const uint8_t *seq, const uint64_t *offsets, uint64_t n_records, uint32_t m, uint8_t *out, uint64_t *pos_out,
                        uint8_t *is_rc_out, uint64_t *bad_record)
{
    if (!c || !offsets || m < 1 || (n_records && !out)) return NTK_ERR_BAD_ARG;
    if (bad_record) *bad_record = ~0ull;
    if (n_records == 0) return NTK_OK;
    for (uint64_t r = 0; r < n_records; r++) {
        if (offsets[r] > offsets[r + 1]) return NTK_ERR_BAD_ARG;
        if (offsets[r + 1] - offsets[r] < m) {   // the reference panics on a sequence shorter than the length asked for (src/sequence.rs:141)
            if (bad_record) *bad_record = r;
            return NTK_ERR_BAD_ARG;
        }
    }
    if (!seq) return NTK_ERR_BAD_ARG;   // (every record holds at least m >= 1 bytes)
    HIPCHK(hipSetDevice(c->device));
    return minimizer_batch_impl(c, seq, offsets, n_records, m, out, pos_out, is_rc_out);
}

int ntk_canonical(ntk_ctx *c, const uint8_t *seq, uint64_t n, uint8_t *out, int *was_rc)
{
    if (!c || (!seq && n) || (!out && n)) return NTK_ERR_BAD_ARG;
    if (was_rc) *was_rc = 0;
    if (n == 0) return NTK_OK;
    if (n > 0xFFFFFFFFull) return NTK_ERR_UNSUPPORTED;
    // the smallest length-n substring over both strands IS the canonical form (one candidate per strand)
    const int rc = ntk_minimizer(c, seq, n, (uint32_t)n, out);
    if (rc == NTK_OK && was_rc) *was_rc = memcmp(out, seq, n) != 0;
    return rc;
}

int ntk_bit_minimizers(ntk_ctx *c, const uint64_t *values, uint64_t n, uint32_t k, uint32_t m, uint64_t *out)
{
    if (!c || (!values && n) || (!out && n)) return NTK_ERR_BAD_ARG;
    if (k < 1 || k > 32 || m < 1 || m > k) return NTK_ERR_BAD_K;
    if (n == 0) return NTK_OK;
    HIPCHK(hipSetDevice(c->device));
    enum { kIn, kOut };   // scratch slots
    int rc;
    if ((rc = ensure_scratch(c, kIn, n * 8)) || (rc = ensure_scratch(c, kOut, n * 8))) return rc;
    uint64_t *d_in = c->scratch_at<uint64_t>(kIn), *d_out = c->scratch_at<uint64_t>(kOut);
    HIPCHK(hipMemcpyAsync(d_in, values, n * 8, hipMemcpyHostToDevice, c->stream));
    hipLaunchKernelGGL(bit_minimizer_kernel, dim3(grid_for(n, 256)), dim3(256), 0, c->stream, (const uint64_t *)d_in, n, k, m, d_out);
    HIPCHK(hipGetLastError());
    HIPCHK(hipMemcpyAsync(out, d_out, n * 8, hipMemcpyDeviceToHost, c->stream));
    HIPCHK(hipStreamSynchronize(c->stream));
    return NTK_OK;
}

int ntk_bit_canonical(ntk_ctx *c, const uint64_t *values, uint64_t n, uint32_t k, int canonical, uint64_t *out, uint8_t *was_rc_out)
{
    if (!c || (n && (!values || !out || (canonical && !was_rc_out)))) return NTK_ERR_BAD_ARG;
    if (k < 1 || k > 32) return NTK_ERR_BAD_K;
    if (n == 0) return NTK_OK;
    HIPCHK(hipSetDevice(c->device));
    enum { kIn, kOut, kWasRc };   // scratch slots
    int rc;
    if ((rc = ensure_scratch(c, kIn, n * 8)) || (rc = ensure_scratch(c, kOut, n * 8)) || (rc = ensure_scratch(c, kWasRc, n))) return rc;
    uint64_t *d_in = c->scratch_at<uint64_t>(kIn), *d_out = c->scratch_at<uint64_t>(kOut);
    uint8_t *d_f = c->scratch_at<uint8_t>(kWasRc);
    HIPCHK(hipMemcpyAsync(d_in, values, n * 8, hipMemcpyHostToDevice, c->stream));
    hipLaunchKernelGGL(bit_canonical_kernel, dim3(grid_for(n, 256)), dim3(256), 0, c->stream, (const uint64_t *)d_in, n, k, canonical, d_out, d_f);
    HIPCHK(hipGetLastError());
    HIPCHK(hipMemcpyAsync(out, d_out, n * 8, hipMemcpyDeviceToHost, c->stream));
    if (canonical) HIPCHK(hipMemcpyAsync(was_rc_out, d_f, n, hipMemcpyDeviceToHost, c->stream));
    HIPCHK(hipStreamSynchronize(c->stream));
    return NTK_OK;
}

int ntk_quality_mask(ntk_ctx *c, const uint8_t *seq, const uint8_t *qual, uint64_t n, uint8_t score, uint8_t *out)
{
    if (!c || (n && (!seq || !qual || !out))) return NTK_ERR_BAD_ARG;
    if (n == 0) return NTK_OK;
    HIPCHK(hipSetDevice(c->device));
    enum { kSeq, kQual, kOut };   // scratch slots
    int rc;
    if ((rc = ensure_scratch(c, kSeq, n)) || (rc = ensure_scratch(c, kQual, n)) || (rc = ensure_scratch(c, kOut, n))) return rc;
    uint8_t *d_s = c->scratch_at<uint8_t>(kSeq), *d_q = c->scratch_at<uint8_t>(kQual), *d_o = c->scratch_at<uint8_t>(kOut);
    HIPCHK(hipMemcpyAsync(d_s, seq, n, hipMemcpyHostToDevice, c->stream));
    HIPCHK(hipMemcpyAsync(d_q, qual, n, hipMemcpyHostToDevice, c->stream));
    hipLaunchKernelGGL(quality_mask_kernel, dim3(grid_for(n, 256)), dim3(256), 0, c->stream, (const uint8_t *)d_s, (const uint8_t *)d_q, n, score, d_o);
    HIPCHK(hipGetLastError());
    HIPCHK(hipMemcpyAsync(out, d_o, n, hipMemcpyDeviceToHost, c->stream));
    HIPCHK(hipStreamSynchronize(c->stream));
    return NTK_OK;
}

/* ---- device utilities ---------------------------------------------------------------------------- */

int ntk_synth_reads_device(ntk_ctx *c, uint64_t seed, uint64_t first_read, uint64_t n_reads, uint32_t read_len,
                           uint32_t n_per_1024, uint8_t *d_out)
{
    if (!c || !d_out || read_len == 0) return NTK_ERR_BAD_ARG;
    if (n_reads == 0) return NTK_OK;
    HIPCHK(hipSetDevice(c->device));
    const uint64_t total = n_reads * ((uint64_t)read_len + 1);
    const uint64_t threads = (total + 15) / 16;
    hipLaunchKernelGGL(synth_reads_kernel, dim3(grid_for(threads, 256)), dim3(256), 0, c->stream,
                       seed, first_read, n_reads, read_len, n_per_1024, d_out);
    HIPCHK(hipGetLastError());
    return NTK_OK;
}

int ntk_reverse_complement_records_device(ntk_ctx *c, const uint8_t *d_in, uint8_t *d_out, uint64_t n_records,
                                          uint32_t record_len, uint32_t stride)
{
    if (!c || !d_in || !d_out || stride == 0 || record_len > stride) return NTK_ERR_BAD_ARG;
    if (n_records == 0) return NTK_OK;
    HIPCHK(hipSetDevice(c->device));
    const uint64_t total = n_records * stride;
    hipLaunchKernelGGL(revcomp_records_kernel, dim3(grid_for(total, 256)), dim3(256), 0, c->stream,
                       d_in, d_out, n_records, record_len, stride, c->lut_complement());
    HIPCHK(hipGetLastError());
    return NTK_OK;
}

}  // extern "C"

// ---------------------------------------------------------------------------------------------
// multi-GPU: one RCCL all-reduce of the accumulators
// ---------------------------------------------------------------------------------------------
namespace {
struct RcclApi {
    decltype(&ncclGetUniqueId) GetUniqueId = nullptr;
    decltype(&ncclCommInitRank) CommInitRank = nullptr;
    decltype(&ncclCommInitAll) CommInitAll = nullptr;
    decltype(&ncclCommDestroy) CommDestroy = nullptr;
    decltype(&ncclAllReduce) AllReduce = nullptr;
    decltype(&ncclGroupStart) GroupStart = nullptr;
    decltype(&ncclGroupEnd) GroupEnd = nullptr;
    bool ok = false;
};
const RcclApi &load_rccl()
{
    static RcclApi api;
    static std::once_flag once;
    std::call_once(once, [] {
        // the copy already mapped into the process first (a torch process brings its own librccl.so), then the ROCm one
        void *h = nullptr;
        for (const char *name : {"librccl.so.1", "librccl.so"}) if ((h = dlopen(name, RTLD_NOW | RTLD_NOLOAD))) break;
        if (!h) for (const char *name : {"librccl.so.1", "librccl.so", "/opt/rocm/lib/librccl.so.1"}) if ((h = dlopen(name, RTLD_NOW | RTLD_LOCAL))) break;
        if (!h) return;
#define NTK_RCCL_SYM(f) api.f = (decltype(api.f))dlsym(h, "nccl" #f); if (!api.f) return;
        NTK_RCCL_SYM(GetUniqueId) NTK_RCCL_SYM(CommInitRank) NTK_RCCL_SYM(CommInitAll) NTK_RCCL_SYM(CommDestroy)
        NTK_RCCL_SYM(AllReduce) NTK_RCCL_SYM(GroupStart) NTK_RCCL_SYM(GroupEnd)
#undef NTK_RCCL_SYM
        api.ok = true;
    });
    return api;
}
#define RCCLCHK(x)                                                  \
    do {                                                            \
        ncclResult_t r__ = (x);                                     \
        if (r__ != ncclSuccess) { g_last_rccl = (int)r__; return NTK_ERR_RCCL; } \
    } while (0)

// after the all-reduce the xor word holds a SUM of xors: rebuild it from the 64 one-bit counters (parity of each sum)
__global__ void xor_from_bit_counters_kernel(uint64_t *acc)
{
    const uint64_t bit = acc[NTK_ACC_XOR_BITS + threadIdx.x] & 1ull;
    const uint64_t word = __builtin_amdgcn_ballot_w64(bit != 0);
    if (threadIdx.x == 0) acc[NTK_ACC_XOR] = word;
}
}  // namespace

extern "C" {

struct ntk_comm {
    std::vector<ntk_ctx *> ctxs;     // local contexts (1 for init_rank, n for init_all)
    std::vector<ncclComm_t> comms;   // one communicator handle per local context
    int size = 0;
    std::vector<std::pair<hipEvent_t, hipEvent_t>> ev_used;   // around each all-reduce on ctxs[0]'s stream while that ctx has timing on
};

int ntk_comm_unique_id(uint8_t id[NTK_COMM_ID_BYTES])
{
    if (!id) return NTK_ERR_BAD_ARG;
    const RcclApi &R = load_rccl();
    if (!R.ok) { g_last_rccl = -1; return NTK_ERR_RCCL; }
    static_assert(sizeof(ncclUniqueId) == NTK_COMM_ID_BYTES, "NTK_COMM_ID_BYTES follows ncclUniqueId");
    ncclUniqueId u;
    RCCLCHK(R.GetUniqueId(&u));
    memcpy(id, &u, sizeof(u));
    return NTK_OK;
}

int ntk_comm_init_rank(ntk_ctx *c, int n_ranks, int rank, const uint8_t id[NTK_COMM_ID_BYTES], ntk_comm **out)
{
    if (!c || !id || !out || n_ranks < 1 || rank < 0 || rank >= n_ranks) return NTK_ERR_BAD_ARG;
    *out = nullptr;
    const RcclApi &R = load_rccl();
    if (!R.ok) { g_last_rccl = -1; return NTK_ERR_RCCL; }
    HIPCHK(hipSetDevice(c->device));
    ncclUniqueId u;
    memcpy(&u, id, sizeof(u));
    ncclComm_t h = nullptr;
    RCCLCHK(R.CommInitRank(&h, n_ranks, u, rank));
    ntk_comm *m = new (std::nothrow) ntk_comm();
    if (!m) { (void)R.CommDestroy(h); return NTK_ERR_NOMEM; }
    m->ctxs.push_back(c); m->comms.push_back(h); m->size = n_ranks;
    *out = m;
    return NTK_OK;
}

int ntk_comm_init_all(ntk_ctx *const *ctxs, int n, ntk_comm **out)
{
    if (!ctxs || !out || n < 1) return NTK_ERR_BAD_ARG;
    *out = nullptr;
    std::vector<int> devs;
    for (int i = 0; i < n; i++) {
        if (!ctxs[i]) return NTK_ERR_BAD_ARG;
        for (int d : devs) if (d == ctxs[i]->device) return NTK_ERR_BAD_ARG;   // one context per device
        devs.push_back(ctxs[i]->device);
    }
    const RcclApi &R = load_rccl();
    if (!R.ok) { g_last_rccl = -1; return NTK_ERR_RCCL; }
    std::vector<ncclComm_t> hs((size_t)n, nullptr);
    RCCLCHK(R.CommInitAll(hs.data(), n, devs.data()));
    ntk_comm *m = new (std::nothrow) ntk_comm();
    if (!m) { for (ncclComm_t h : hs) (void)R.CommDestroy(h); return NTK_ERR_NOMEM; }
    m->ctxs.assign(ctxs, ctxs + n); m->comms = hs; m->size = n;
    *out = m;
    return NTK_OK;
}

int ntk_comm_size(const ntk_comm *m) { return m ? m->size : 0; }

int ntk_allreduce_accumulators(ntk_comm *m)
{
    if (!m) return NTK_ERR_BAD_ARG;
    const RcclApi &R = load_rccl();
    if (!R.ok) { g_last_rccl = -1; return NTK_ERR_RCCL; }
    TimedSpan span;   // the collective's own duration on this rank (ntk_comm_allreduce_time_ms): events on the stream it runs on; a failure
                      // below loses the timing of this call, not the events
    ntk_ctx *c0 = m->ctxs.empty() ? nullptr : m->ctxs[0];
    if (c0 && c0->timing) {
        HIPCHK(hipSetDevice(c0->device));
        int rc = span.begin(c0);
        if (rc) return rc;
    }
    ncclResult_t r = R.GroupStart();
    if (r != ncclSuccess) { g_last_rccl = (int)r; return NTK_ERR_RCCL; }
    for (size_t i = 0; i < m->ctxs.size(); i++) {
        ntk_ctx *c = m->ctxs[i];
        r = R.AllReduce(c->d_acc, c->d_acc, NTK_ACC_WORDS, ncclUint64, ncclSum, m->comms[i], c->stream);
        if (r != ncclSuccess) { (void)R.GroupEnd(); g_last_rccl = (int)r; return NTK_ERR_RCCL; }
    }
    if ((r = R.GroupEnd()) != ncclSuccess) { g_last_rccl = (int)r; return NTK_ERR_RCCL; }
    for (ntk_ctx *c : m->ctxs) {
        HIPCHK(hipSetDevice(c->device));
        hipLaunchKernelGGL(xor_from_bit_counters_kernel, dim3(1), dim3(64), 0, c->stream, c->d_acc);
        HIPCHK(hipGetLastError());
    }
    if (span.e0) HIPCHK(hipSetDevice(c0->device));
    return span.end(m->ev_used);
}

/* Sum of the durations of the all-reduces (collective + xor rebuild, on the first local ctx's stream) issued while that ctx had
 * ntk_ctx_enable_timing on, since the last call; synchronises that stream. */
int ntk_comm_allreduce_time_ms(ntk_comm *m, double *total_ms, uint64_t *calls)
{
    if (!m || !total_ms || m->ctxs.empty()) return NTK_ERR_BAD_ARG;
    ntk_ctx *c = m->ctxs[0];
    HIPCHK(hipSetDevice(c->device));
    HIPCHK(hipStreamSynchronize(c->stream));
    double t = 0;
    for (auto &p : m->ev_used) {
        float ms = 0;
        HIPCHK(hipEventElapsedTime(&ms, p.first, p.second));
        t += ms;
        c->ev_free.push_back(p.first); c->ev_free.push_back(p.second);
    }
    if (calls) *calls = m->ev_used.size();
    m->ev_used.clear();
    *total_ms = t;
    return NTK_OK;
}

void ntk_comm_destroy(ntk_comm *m)
{
    if (!m) return;
    const RcclApi &R = load_rccl();
    if (R.ok) for (ncclComm_t h : m->comms) if (h) (void)R.CommDestroy(h);
    // timing events of all-reduces nobody asked ntk_comm_allreduce_time_ms about: destroyed here (the ctx they were drawn from may be gone)
    for (auto &p : m->ev_used) { (void)hipEventDestroy(p.first); (void)hipEventDestroy(p.second); }
    delete m;
}

}  // extern "C"

