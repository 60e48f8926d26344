// A set of MinHash sketches on the device and its all-pairs comparison (include/needletail_amd_minhash_set.h).  A consumer of the
// core's public ABI like the other libraries (it takes the context's device and stream and nothing else), and of no other library: it
// compares hashes somebody else made and never hashes a k-mer.
//
// Layout: offsets[n_sketches + 1], hashes[n_entries], counts[n_entries] (only with abundance), cut[n_sketches] (a compare's scratch:
// every sketch's length at or below max_hash).  add appends to host staging; flush uploads what is new, one copy per array.
//
// The pair kernel never builds a union (ntk_mhset_rank.hpp has the rule and every per-lane step).  A block of kPairWaves waves shares
// one SEARCHED sketch, staged in LDS when it has at most kStage hashes, and each of its waves walks one WALKED sketch against it in
// coalesced rounds of 64: every lane takes a lower bound in the searched sketch, the round's shared flags become each lane's count of
// shared elements before it through a ballot and a wave-uniform carry, the sums go through wave reductions, and lane 0 stores the
// pair's results; no atomics.  The first pass walks the row sketch (A) against the column sketch (B); norm2_b is the same pass with the
// roles swapped.  DESIGN.md section 17.
#include "../../include/needletail_amd_minhash_set.h"
#include "ntk_consumer.hpp"
#include "ntk_mhset_rank.hpp"

#include <cstring>
#include <new>
#include <vector>

namespace {

constexpr uint32_t kStage = 2048;                  // hashes of a searched sketch that fit the block's LDS stage (16 KiB)
constexpr int kPairThreads = 256;
constexpr uint32_t kPairWaves = kPairThreads / 64; // walked sketches per block
constexpr uint64_t kBlockDefault = (uint64_t)1 << 20;
constexpr uint64_t kResultBytes = 32;              // per pair: two uint32 and three doubles

static_assert(kStage == NTK_MHSET_STAGE, "the header states the stage length");
static_assert(kBlockDefault == NTK_MHSET_BLOCK_DEFAULT, "the header states the default block");

// one side of a launch: a set's arrays and the first sketch of the launch's range in it
struct Side {
    const uint64_t *offsets, *hashes, *counts;   // counts: nullptr = every count is 1
    const uint64_t *cut;                         // indexed by sketch
    uint64_t first;                              // the range's first sketch
    uint64_t n;                                  // sketches in the range
    uint64_t rel;                                // `first` relative to the compare's row0 / col0
    uint64_t stride;                             // what one step on this side adds to the pair index: n_cols for rows, 1 for columns
};

struct PairArgs {
    Side walk, search;
    uint64_t p0, np;        // the sub-block: pair indices [p0, p0 + np) of the compare's row-major block; result slot = index - p0
    uint64_t num;
    uint32_t *n_shared, *n_union;
    double *dot, *norm2;    // norm2: of the walked side
    uint32_t norm_only;     // the swapped pass stores norm2 alone
};

struct CutArgs {
    const uint64_t *offsets[2], *hashes[2];
    uint64_t *cut[2];
    uint64_t first[2], n[2];
    uint64_t max_hash;
};

// one thread per sketch of the two ranges: its length at or below max_hash
__global__ __launch_bounds__(kThreads) void ms_cut_kernel(CutArgs a)
{
    uint64_t t = (uint64_t)blockIdx.x * kThreads + threadIdx.x;
    int side = 0;
    if (t >= a.n[0]) { t -= a.n[0]; side = 1; }
    if (t >= a.n[side]) return;
    const uint64_t s = a.first[side] + t, lo = a.offsets[side][s], hi = a.offsets[side][s + 1];
    a.cut[side][s] = ms_cut_length(a.hashes[side] + lo, hi - lo, a.max_hash);
}

__device__ inline double wave_sum_f64(double v)
{
    for (int off = 32; off > 0; off >>= 1) v += __shfl_xor(v, off, 64);
    return v;
}

// One wave, one pair: A (na hashes at `a`, counts `ca` or nullptr) walked against B (nb hashes at `b`, in LDS or global memory; counts
// `cb` in global memory or nullptr).
__device__ __forceinline__ void pair_wave(const PairArgs &g, uint64_t slot, const uint64_t *a, const uint64_t *ca, uint32_t na,
                                          const uint64_t *b, const uint64_t *cb, uint32_t nb)
{
    const uint32_t lane = threadIdx.x & 63;
    const bool to_num = ms_union_is_num(g.num, na, nb);
    MsLane acc;
    uint64_t carry = 0;   // shared elements of the rounds before (wave-uniform)
    for (uint64_t base = 0; base < na; base += 64) {   // (64-bit: na may be within 64 of 2^32)
        const uint64_t i = base + lane;
        const bool live = i < na;
        MsHit hit;
        hit.p = 0; hit.shared = false;
        double x = 1.0, y = 1.0;
        if (live) {
            hit = ms_probe(b, nb, a[i]);
            if (ca) x = (double)ca[i];
            if (cb && hit.shared) y = (double)cb[hit.p];
        }
        const uint64_t ballot = __ballot(hit.shared);
        const uint64_t position = ms_lane_step(acc, live, i, hit, ballot, lane, carry, g.num, x, y);
        carry += (uint64_t)__popcll(ballot);
        // lane 63's position is the round's largest; if it is at or past num, so is every later element's.  (Lane 63 is dead only in the
        // last round.)
        if (to_num && uniform(__shfl(position, 63, 64)) >= g.num) break;
    }
    const uint64_t counted_shared = wave_sum((uint64_t)acc.n_shared);
    const double dot = wave_sum_f64(acc.dot), norm2 = wave_sum_f64(acc.norm2);
    if (lane == 0) {
        g.norm2[slot] = norm2;
        if (!g.norm_only) {
            g.n_shared[slot] = (uint32_t)counted_shared;
            g.n_union[slot] = (uint32_t)ms_union(g.num, na, nb, carry);   // carry == S only where the walk went to A's end, and only
            g.dot[slot] = dot;                                            // there does ms_union look at it
        }
    }
}

// Block b: searched sketch b / groups of the search range, walked sketches (b % groups) * kPairWaves .. + kPairWaves - 1 of the walk
// range.  A wave whose pair lies outside the sub-block (the launch covers the rows the sub-block touches) has nothing to do.
__global__ __launch_bounds__(kPairThreads) void ms_pair_kernel(PairArgs g)
{
    __shared__ uint64_t stage[kStage];
    const uint64_t groups = (g.walk.n + kPairWaves - 1) / kPairWaves;
    const uint64_t si = blockIdx.x / groups, wi = (blockIdx.x % groups) * kPairWaves + (threadIdx.x >> 6);
    const uint64_t sb = g.search.first + si, b_off = g.search.offsets[sb];
    const uint32_t nb = (uint32_t)g.search.cut[sb];
    const uint64_t *b = g.search.hashes + b_off;
    const bool staged = nb <= kStage;   // block-uniform
    if (staged)
        for (uint32_t t = threadIdx.x; t < nb; t += kPairThreads) stage[t] = b[t];
    __syncthreads();
    if (wi >= g.walk.n) return;
    const uint64_t pair = (g.walk.rel + wi) * g.walk.stride + (g.search.rel + si) * g.search.stride;
    if (pair < g.p0 || pair - g.p0 >= g.np) return;
    const uint64_t sa = g.walk.first + wi, a_off = g.walk.offsets[sa];
    const uint32_t na = (uint32_t)g.walk.cut[sa];
    const uint64_t *a = g.walk.hashes + a_off;
    const uint64_t *ca = g.walk.counts ? g.walk.counts + a_off : nullptr, *cb = g.search.counts ? g.search.counts + b_off : nullptr;
    if (staged) pair_wave(g, pair - g.p0, a, ca, na, stage, cb, nb);
    else pair_wave(g, pair - g.p0, a, ca, na, b, cb, nb);
}

}  // namespace

struct ntk_mhset : Consumer {
    uint32_t abundance = 0;
    uint64_t block_pairs = 0;
    std::vector<uint64_t> offsets{0};          // host: every sketch's start, and the end of the last
    std::vector<uint64_t> new_hashes, new_counts;   // host staging: the entries of the sketches not yet uploaded
    uint64_t up_sketches = 0, up_entries = 0;  // what the device holds
    DeviceArray<uint64_t> d_offsets, d_hashes, d_counts, d_cut;   // grown by doubling, their contents kept
    DeviceArray<uint8_t> d_res;                // the result scratch: kResultBytes per pair of a sub-block
    Pinned<uint8_t> h_res;                     // its mirror
    uint64_t n_launches = 0, n_uploads = 0;

    uint64_t n_sketches() const { return offsets.size() - 1; }
    uint64_t n_entries() const { return offsets.back(); }
};

namespace {

// what was added since the last upload goes to the device: one copy per array (synchronises)
int flush(ntk_mhset *s)
{
    CT_HIPCHK(hipSetDevice(s->device));
    const uint64_t n_sk = s->n_sketches(), n_en = s->n_entries();
    if (s->up_sketches == n_sk && s->d_offsets.p) return NTK_OK;
    int rc = s->d_offsets.ensure(s->stream, n_sk + 1, grow_doubling, s->up_sketches ? s->up_sketches + 1 : 0);
    if (!rc) rc = s->d_cut.ensure(s->stream, n_sk + 1, grow_doubling);
    if (!rc) rc = s->d_hashes.ensure(s->stream, n_en + 1, grow_doubling, s->up_entries);
    if (!rc && s->abundance) rc = s->d_counts.ensure(s->stream, n_en + 1, grow_doubling, s->up_entries);
    if (rc) return rc;
    // offsets[up_sketches] is on the device already, or is the leading 0 of an empty device copy
    const uint64_t from = s->up_sketches ? s->up_sketches + 1 : 0;
    CT_HIPCHK(hipMemcpyAsync(s->d_offsets.p + from, s->offsets.data() + from, (n_sk + 1 - from) * sizeof(uint64_t), hipMemcpyHostToDevice,
                             s->stream));
    const uint64_t fresh = n_en - s->up_entries;
    if (fresh) {
        CT_HIPCHK(hipMemcpyAsync(s->d_hashes.p + s->up_entries, s->new_hashes.data(), fresh * sizeof(uint64_t), hipMemcpyHostToDevice,
                                 s->stream));
        if (s->abundance)
            CT_HIPCHK(hipMemcpyAsync(s->d_counts.p + s->up_entries, s->new_counts.data(), fresh * sizeof(uint64_t), hipMemcpyHostToDevice,
                                     s->stream));
    }
    CT_HIPCHK(hipStreamSynchronize(s->stream));   // the staging is free again
    s->up_sketches = n_sk; s->up_entries = n_en;
    s->new_hashes.clear(); s->new_counts.clear();
    s->n_uploads++;
    return NTK_OK;
}

// room for the results of `pairs` pairs, on the device and in its pinned mirror
int ensure_results(ntk_mhset *s, uint64_t pairs)
{
    if (pairs * kResultBytes <= s->d_res.cap) return NTK_OK;
    int rc = s->d_res.ensure(s->stream, pairs * kResultBytes, grow_exact);
    if (!rc && (rc = s->h_res.alloc(pairs * kResultBytes))) s->d_res.release();   // both or neither
    return rc;
}

Side side_of(const ntk_mhset *s, uint64_t first, uint64_t n, uint64_t rel, uint64_t stride)
{
    Side d;
    d.offsets = s->d_offsets.p; d.hashes = s->d_hashes.p; d.counts = s->abundance ? s->d_counts.p : nullptr; d.cut = s->d_cut.p;
    d.first = first; d.n = n; d.rel = rel; d.stride = stride;
    return d;
}

}  // namespace

extern "C" {

int ntk_mhset_create(ntk_ctx *ctx, uint32_t abundance, uint64_t block_pairs, ntk_mhset **out)
{
    if (!ctx || !out) return NTK_ERR_BAD_ARG;
    *out = nullptr;
    if (abundance > 1) return NTK_ERR_BAD_ARG;
    if (block_pairs == 0) block_pairs = NTK_MHSET_BLOCK_DEFAULT;
    if (block_pairs < NTK_MHSET_BLOCK_MIN || block_pairs > NTK_MHSET_BLOCK_MAX) return NTK_ERR_BAD_ARG;
    ntk_mhset *s = new (std::nothrow) ntk_mhset();
    if (!s) return NTK_ERR_NOMEM;
    const int rc = s->bind(ctx, 0, 0);
    if (rc) { delete s; return rc; }
    s->abundance = abundance; s->block_pairs = block_pairs;
    *out = s;
    return NTK_OK;
}

void ntk_mhset_destroy(ntk_mhset *s)
{
    if (!s) return;
    (void)hipSetDevice(s->device);
    (void)hipStreamSynchronize(s->stream);
    for (DeviceArray<uint64_t> *g : {&s->d_offsets, &s->d_hashes, &s->d_counts, &s->d_cut}) g->release();
    s->d_res.release();
    s->h_res.release();
    (void)hipGetLastError();
    delete s;
}

int ntk_mhset_reset(ntk_mhset *s)
{
    if (!s) return NTK_ERR_BAD_ARG;
    s->offsets.assign(1, 0);
    s->new_hashes.clear(); s->new_counts.clear();
    s->up_sketches = 0; s->up_entries = 0;
    return NTK_OK;
}

int ntk_mhset_add(ntk_mhset *s, const uint64_t *hashes, const uint64_t *counts, uint64_t n, uint64_t *index)
{
    if (!s || n >= ((uint64_t)1 << 32) || (n && !hashes) || (counts && !s->abundance)) return NTK_ERR_BAD_ARG;
    for (uint64_t i = 1; i < n; i++)
        if (hashes[i] <= hashes[i - 1]) return NTK_ERR_BAD_ARG;
    const size_t staged = s->new_hashes.size();
    try {
        s->offsets.reserve(s->offsets.size() + 1);
        s->new_hashes.insert(s->new_hashes.end(), hashes, hashes + n);
        if (s->abundance) {
            if (counts) s->new_counts.insert(s->new_counts.end(), counts, counts + n);
            else s->new_counts.insert(s->new_counts.end(), n, (uint64_t)1);
        }
    } catch (const std::bad_alloc &) {
        s->new_hashes.resize(staged);
        s->new_counts.resize(s->abundance ? staged : 0);
        return NTK_ERR_NOMEM;
    }
    if (index) *index = s->n_sketches();
    s->offsets.push_back(s->offsets.back() + n);   // reserved above
    return NTK_OK;
}

int ntk_mhset_read(ntk_mhset *s, uint64_t index, uint64_t *hashes, uint64_t *counts, uint64_t cap, uint64_t *n)
{
    if (!s || !n || index >= s->n_sketches() || (cap && !hashes)) return NTK_ERR_BAD_ARG;
    const uint64_t lo = s->offsets[index], len = s->offsets[index + 1] - lo;
    *n = len;
    if (len > cap) return NTK_ERR_CAPACITY;
    const int rc = flush(s);
    if (rc || len == 0) return rc;
    CT_HIPCHK(hipMemcpyAsync(hashes, s->d_hashes.p + lo, len * sizeof(uint64_t), hipMemcpyDeviceToHost, s->stream));
    if (counts && s->abundance)
        CT_HIPCHK(hipMemcpyAsync(counts, s->d_counts.p + lo, len * sizeof(uint64_t), hipMemcpyDeviceToHost, s->stream));
    CT_HIPCHK(hipStreamSynchronize(s->stream));
    if (counts && !s->abundance)
        for (uint64_t i = 0; i < len; i++) counts[i] = 1;
    return NTK_OK;
}

int ntk_mhset_stats(ntk_mhset *s, struct ntk_mhset_stats *out)
{
    if (!s || !out) return NTK_ERR_BAD_ARG;
    out->n_sketches = s->n_sketches();
    out->n_entries = s->n_entries();
    out->abundance = s->abundance;
    out->block_pairs = s->block_pairs;
    out->device_bytes = s->d_offsets.bytes() + s->d_hashes.bytes() + s->d_counts.bytes() + s->d_cut.bytes() + s->d_res.bytes();
    out->n_launches = s->n_launches;
    out->n_uploads = s->n_uploads;
    return NTK_OK;
}

int ntk_mhset_compare(ntk_mhset *rows, uint64_t row0, uint64_t n_rows, ntk_mhset *cols, uint64_t col0, uint64_t n_cols, uint64_t num,
                      uint64_t max_hash, uint32_t *n_shared, uint32_t *n_union, double *dot, double *norm2_a, double *norm2_b, uint64_t *n_a,
                      uint64_t *n_b)
{
    if (!rows || !cols || rows->ctx != cols->ctx) return NTK_ERR_BAD_ARG;
    if (row0 > rows->n_sketches() || n_rows > rows->n_sketches() - row0 || col0 > cols->n_sketches() || n_cols > cols->n_sketches() - col0)
        return NTK_ERR_BAD_ARG;
    if (n_rows == 0 || n_cols == 0) return NTK_OK;
    if (n_rows > ~(uint64_t)0 / n_cols) return NTK_ERR_BAD_ARG;   // the pair index is 64-bit
    const uint64_t n_pairs = n_rows * n_cols;
    ntk_mhset *s = rows;
    int rc = flush(rows);
    if (!rc && cols != rows) rc = flush(cols);
    if (rc) return rc;
    hipStream_t stream = s->stream;

    CutArgs c;
    const ntk_mhset *both[2] = {rows, cols};
    for (int i = 0; i < 2; i++) {
        c.offsets[i] = both[i]->d_offsets.p; c.hashes[i] = both[i]->d_hashes.p; c.cut[i] = both[i]->d_cut.p;
    }
    c.first[0] = row0; c.n[0] = n_rows; c.first[1] = col0; c.n[1] = n_cols;
    c.max_hash = max_hash;
    hipLaunchKernelGGL(ms_cut_kernel, dim3(grid_for(n_rows + n_cols, kThreads, 0x7FFFFFFFu)), dim3(kThreads), 0, stream, c);
    CT_HIPCHK(hipGetLastError());
    if (n_a) CT_HIPCHK(hipMemcpyAsync(n_a, rows->d_cut.p + row0, n_rows * sizeof(uint64_t), hipMemcpyDeviceToHost, stream));
    if (n_b) CT_HIPCHK(hipMemcpyAsync(n_b, cols->d_cut.p + col0, n_cols * sizeof(uint64_t), hipMemcpyDeviceToHost, stream));

    // what is copied back of a sub-block's results: the arrays lie in this order, and the copy ends with the last one asked for
    const uint64_t fields = norm2_b ? 32 : norm2_a ? 24 : dot ? 16 : (n_shared || n_union) ? 8 : 0;
    if (fields == 0) {
        CT_HIPCHK(hipStreamSynchronize(stream));
        return NTK_OK;
    }
    if ((rc = ensure_results(s, n_pairs < s->block_pairs ? n_pairs : s->block_pairs))) return rc;
    for (uint64_t p0 = 0; p0 < n_pairs; p0 += s->block_pairs) {
        const uint64_t np = n_pairs - p0 < s->block_pairs ? n_pairs - p0 : s->block_pairs;
        // the rectangle the launch covers: the rows the sub-block touches; of a single row, only its columns
        const uint64_t r_lo = p0 / n_cols, r_hi = (p0 + np - 1) / n_cols;
        const uint64_t c_lo = r_lo == r_hi ? p0 % n_cols : 0, c_n = r_lo == r_hi ? np : n_cols;
        const Side row_side = side_of(rows, row0 + r_lo, r_hi - r_lo + 1, r_lo, n_cols);
        const Side col_side = side_of(cols, col0 + c_lo, c_n, c_lo, 1);
        PairArgs g;
        g.p0 = p0; g.np = np; g.num = num;
        g.n_shared = (uint32_t *)s->d_res.p; g.n_union = g.n_shared + np;
        g.dot = (double *)(s->d_res.p + 8 * np);
        double *d_norm_a = g.dot + np, *d_norm_b = d_norm_a + np;
        for (int pass = 0; pass < (norm2_b ? 2 : 1); pass++) {
            g.walk = pass ? col_side : row_side; g.search = pass ? row_side : col_side;
            g.norm2 = pass ? d_norm_b : d_norm_a; g.norm_only = (uint32_t)pass;
            const uint64_t blocks = g.search.n * ((g.walk.n + kPairWaves - 1) / kPairWaves);
            if (blocks > 0x7FFFFFFFull) return NTK_ERR_UNSUPPORTED;   // cannot happen below NTK_MHSET_BLOCK_MAX
            hipLaunchKernelGGL(ms_pair_kernel, dim3((unsigned)blocks), dim3(kPairThreads), 0, stream, g);
            CT_HIPCHK(hipGetLastError());
            s->n_launches++;
        }
        if ((rc = s->h_res.read(stream, s->d_res.p, fields * np))) return rc;
        if (n_shared) memcpy(n_shared + p0, s->h_res.p, np * sizeof(uint32_t));
        if (n_union) memcpy(n_union + p0, s->h_res.p + 4 * np, np * sizeof(uint32_t));
        if (dot) memcpy(dot + p0, s->h_res.p + 8 * np, np * sizeof(double));
        if (norm2_a) memcpy(norm2_a + p0, s->h_res.p + 16 * np, np * sizeof(double));
        if (norm2_b) memcpy(norm2_b + p0, s->h_res.p + 24 * np, np * sizeof(double));
    }
    return NTK_OK;
}

}  // extern "C"
