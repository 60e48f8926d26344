// Base-level alignment of reported chains (include_pending/needletail_amd/align.h): the gaps between a chain's anchors filled by banded
// affine dynamic programming, over the chain and anchor arrays and the two sequence batches where they lie on the device.  A consumer of
// the core's public ABI on the shared scaffold (ntk_consumer.hpp); it reads bases only through the two batches it is given, names no
// other library and links nothing but the core.
//
// run_device: verify the arrays (aln_verify_kernel), number the segments of the selected chains by a scan (rocPRIM), size every between
// part (aln_plan_kernel), scan the direction bytes and the run bounds (rocPRIM), fill the direction bytes group by group, one wave per DP
// segment (aln_dp_kernel), walk them back into per-segment run lists (aln_trace_kernel), then count and, behind one more scan, write every
// chain's canonical CIGAR (aln_emit_kernel).  rocPRIM's temporary storage is held inside a call only.  The rule is ntk_align_rule.hpp's.
// DESIGN.md section 26.
#include "../../include_pending/needletail_amd/align.h"
#include "ntk_consumer.hpp"
#include "ntk_align_rule.hpp"

#include <rocprim/device/device_scan.hpp>
#include <rocprim/iterator/counting_iterator.hpp>
#include <rocprim/iterator/transform_iterator.hpp>

#include <new>

namespace {

// the counter words: what the verification raised and what the plan, the DP and the emit kernels counted
constexpr int kCtrFlags = 0, kCtrAligned = 1, kCtrTooLong = 2, kCtrSegments = 3, kCtrDpSegments = 4, kCtrCells = 5, kCtrMostCols = 6, kCtrWords = 7;
constexpr uint32_t kWaves = ALN_THREADS / 64;

static_assert(ALN_THREADS == kThreads && ALN_DP_THREADS == 64, "the blocks of the scaffold; one wave per DP block");
static_assert(sizeof(struct ntk_align_params) == 32 && sizeof(struct ntk_align_stats) == 72, "the header's struct sizes");
static_assert((uint64_t)ALN_SEG_MAX * ALN_SEG_MAX <= (uint64_t)ALN_WORK_MIB_MIN << 20, "one segment fits the smallest workspace");

__device__ inline void or_agent(uint64_t *p, uint64_t v) { (void)__hip_atomic_fetch_or(p, v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT); }
__device__ inline void max_agent(uint64_t *p, uint64_t v) { (void)__hip_atomic_fetch_max(p, v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT); }

// what one lane of a wave stored in LDS is seen by the loads of the other lanes behind this
__device__ inline void wave_fence()
{
    __builtin_amdgcn_fence(__ATOMIC_SEQ_CST, "workgroup");
    __builtin_amdgcn_wave_barrier();
}

__device__ inline uint64_t first_item() { return (uint64_t)blockIdx.x * ALN_THREADS + threadIdx.x; }
__device__ inline uint64_t item_step() { return (uint64_t)gridDim.x * ALN_THREADS; }

struct AlnArgs {
    const uint8_t *ref, *seq;                 // the two batches ...
    const uint64_t *ref_offsets, *seq_offsets;   // ... and their n_refs + 1 and n_reads + 1 record starts
    uint64_t ref_bytes, seq_bytes, n_refs, n_reads;
    const uint64_t *c_offsets;                // the chains: n_reads + 1 offsets ...
    const uint32_t *chain_rows;               // ... n_chains rows of eight words ...
    const uint64_t *m_offsets;                // ... their n_chains + 1 member ranges ...
    const uint32_t *members;                  // ... and n_members members,
    const uint32_t *rpos, *qpos;              // indices into the n_anchors anchors
    const uint32_t *sel;                      // the n_sel chains to align
    uint64_t n_chains, n_members, n_anchors, n_sel, n_seg;
    aln_rule_params r;
    uint32_t *rows;                           // the result per entry of sel ...
    int64_t *scores;
    uint64_t *g_offsets;
    uint32_t *cigar;
    uint64_t *seg_offsets;                    // the work per entry: its first segment
    uint32_t *seg_entry;                      // per segment: its entry of sel,
    uint64_t *seg_cells, *dir_offsets;        // its direction bytes and their scan,
    uint32_t *seg_runs;                       // the bound of its run list, then its length,
    uint64_t *run_offsets;                    // and the scan of the bounds
    uint8_t *dir;                             // the direction bytes of one group
    uint32_t *runs;
    uint64_t *ctr;
};

// a selected chain as the kernels walk it
struct Chain {
    uint64_t first, cnt;                      // its members
    uint32_t rev;
    const uint8_t *ref, *read;                // its two records
    uint64_t read_len;
};

// entry s of sel of verified arrays
__device__ inline Chain chain_of(const AlnArgs &a, uint64_t s)
{
    const uint64_t c = a.sel[s];
    const uint32_t ref_rev = a.chain_rows[8 * c + 2];
    const uint64_t q = aln_at_or_before(a.c_offsets, a.n_reads + 1, c) - 1;
    Chain ch;
    ch.first = a.m_offsets[c]; ch.cnt = a.m_offsets[c + 1] - ch.first;
    ch.rev = ref_rev & 1;
    ch.ref = a.ref + a.ref_offsets[ref_rev >> 1];
    ch.read = a.seq + a.seq_offsets[q];
    ch.read_len = aln_record_len(a.seq_offsets[q], a.seq_offsets[q + 1]);
    return ch;
}

// where member t of a chain starts on the reference and on the query, in the coordinates of the rule
__device__ inline void anchor_of(const AlnArgs &a, const Chain &ch, uint64_t t, uint64_t &r, uint64_t &q)
{
    const uint32_t m = a.members[ch.first + t];
    r = a.rpos[m];
    q = ch.rev ? ch.read_len - a.qpos[m] - a.r.k : a.qpos[m];
}

// the between part behind member t of a chain: n reference bases from r on against m query bases from q on
struct Between {
    uint64_t r, q, n, m, m0;
};
__device__ inline Between between_of(const AlnArgs &a, const Chain &ch, uint64_t t)
{
    uint64_t r0, q0, r1, q1;
    anchor_of(a, ch, t, r0, q0);
    anchor_of(a, ch, t + 1, r1, q1);
    Between b;
    b.m0 = (uint64_t)aln_m0((int64_t)(r1 - r0), (int64_t)(q1 - q0), a.r.k);
    b.r = r0 + b.m0; b.q = q0 + b.m0; b.n = r1 - r0 - b.m0; b.m = q1 - q0 - b.m0;
    return b;
}

// the number of segments of entry s of sel, for the scan that numbers them; 0 behind the last
struct SegmentCount {
    const uint32_t *sel;
    const uint64_t *m_offsets;
    uint64_t n_sel;
    __host__ __device__ uint64_t operator()(uint64_t s) const
    {
        if (s >= n_sel) return 0;
        const uint64_t c = sel[s];
        return m_offsets[c + 1] - m_offsets[c] - 1;
    }
};

// the CIGAR length of entry s of sel, for the scan that places them; 0 behind the last
struct CigarCount {
    const uint32_t *rows;
    uint64_t n_sel;
    __host__ __device__ uint64_t operator()(uint64_t s) const { return s < n_sel ? rows[ALN_ROW_WORDS * s + ALN_N_CIGAR] : 0; }
};

// The arrays as the rule reads them: one record start of either batch and one read's chain range per thread, then one wave per entry
// of sel; ctr is zeroed before.  A chain's members are read only where its range lies inside the members, an anchor only where the
// member is below n_anchors, a record start only where the record exists; no base is read.
__global__ __launch_bounds__(ALN_THREADS) void aln_verify_kernel(AlnArgs a)
{
    uint32_t bad = 0;
    uint64_t items = a.n_refs > a.n_reads ? a.n_refs : a.n_reads;
    for (uint64_t i = first_item(); i <= items; i += item_step()) {
        if (i < a.n_refs && a.ref_offsets[i] > a.ref_offsets[i + 1]) bad |= ALN_BAD_OFFSETS;
        if (i == a.n_refs && a.ref_offsets[i] > a.ref_bytes) bad |= ALN_BAD_OFFSETS;
        if (i < a.n_reads && (a.seq_offsets[i] > a.seq_offsets[i + 1] || a.c_offsets[i] > a.c_offsets[i + 1])) bad |= ALN_BAD_OFFSETS;
        if (i == a.n_reads && (a.seq_offsets[i] > a.seq_bytes || a.c_offsets[i] > a.n_chains)) bad |= ALN_BAD_OFFSETS;
    }
    const uint32_t wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
    const uint64_t waves = (uint64_t)gridDim.x * kWaves, lo = a.c_offsets[0], hi = a.c_offsets[a.n_reads];
    for (uint64_t s = (uint64_t)blockIdx.x * kWaves + wave; s < a.n_sel; s += waves) {
        const uint64_t c = a.sel[s];
        if (c >= a.n_chains || c < lo || c >= hi) { bad |= ALN_BAD_SEL; continue; }
        const uint64_t b = a.m_offsets[c], e = a.m_offsets[c + 1];
        const uint32_t score = a.chain_rows[8 * c], ref_rev = a.chain_rows[8 * c + 2];
        if (score < 1 || score > ALN_SCORE_MAX) bad |= ALN_BAD_SCORE;
        if (b > e || e > a.n_members) { bad |= ALN_BAD_OFFSETS; continue; }
        if (b == e) { bad |= ALN_NO_MEMBER; continue; }
        for (uint64_t t = b + lane; t < e; t += 64) {
            const uint32_t m = a.members[t];
            if (m >= a.n_anchors) { bad |= ALN_BAD_MEMBER; continue; }
            if (t == b) continue;
            const uint32_t prev = a.members[t - 1];
            if (prev >= a.n_anchors) continue;   // (raised by the lane of t - 1)
            int64_t dr, dq;
            aln_step(ref_rev & 1, a.rpos[prev], a.qpos[prev], a.rpos[m], a.qpos[m], dr, dq);
            if (dr < 1 || dq < 1) bad |= ALN_BAD_ORDER;
        }
        if (lane != 0) continue;
        const uint64_t ref = ref_rev >> 1, at = aln_at_or_before(a.c_offsets, a.n_reads + 1, c);
        if (ref >= a.n_refs) { bad |= ALN_BAD_END; continue; }
        const uint32_t first = a.members[b], last = a.members[e - 1];
        if (first >= a.n_anchors || last >= a.n_anchors || at < 1 || at > a.n_reads) continue;
        const uint64_t r_b = a.ref_offsets[ref], r_e = a.ref_offsets[ref + 1], q_b = a.seq_offsets[at - 1], q_e = a.seq_offsets[at];
        if (r_b > r_e || q_b > q_e) continue;   // (raised above)
        const uint64_t rs = a.rpos[first], re = (uint64_t)a.rpos[last] + a.r.k;
        const uint64_t q0 = a.qpos[first], q1 = a.qpos[last], qs = q0 < q1 ? q0 : q1, qe = (q0 < q1 ? q1 : q0) + a.r.k;
        if (re > aln_record_len(r_b, r_e) || qe > aln_record_len(q_b, q_e)) bad |= ALN_BAD_END;
        else if ((re >= rs && re - rs >= ALN_SPAN_MAX) || qe - qs >= ALN_SPAN_MAX) bad |= ALN_LONG_SPAN;
    }
    if (bad) or_agent(a.ctr + kCtrFlags, bad);
}

// The between parts of verified arrays, one wave per entry of sel: lanes stride over the entry's segments twice.  First for the chain's
// flag - one part longer than max_seg makes the whole chain TOO_LONG - then for every segment's entry, its direction bytes and the bound
// of its run list, both 0 where the part needs no DP or the chain is too long.  Lane 0 writes the entry's row as its flag and zeros.
__global__ __launch_bounds__(ALN_THREADS) void aln_plan_kernel(AlnArgs a)
{
    const uint32_t wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
    const uint64_t waves = (uint64_t)gridDim.x * kWaves;
    uint64_t n_dp = 0, most = 0, n_long = 0, n_segments = 0;
    if (first_item() == 0) { a.seg_cells[a.n_seg] = 0; a.seg_runs[a.n_seg] = 0; }
    for (uint64_t s = (uint64_t)blockIdx.x * kWaves + wave; s < a.n_sel; s += waves) {
        const Chain ch = chain_of(a, s);
        bool too_long = false;
        for (uint64_t t = lane; t + 1 < ch.cnt; t += 64) {
            const Between b = between_of(a, ch, t);
            too_long |= (b.n > b.m ? b.n : b.m) > a.r.max_seg;
        }
        too_long = __ballot(too_long) != 0;
        const uint64_t seg0 = a.seg_offsets[s];
        for (uint64_t t = lane; t + 1 < ch.cnt; t += 64) {
            const Between b = between_of(a, ch, t);
            const bool dp = !too_long && b.n && b.m;
            int32_t lo = 0, hi = 0;
            if (dp) aln_band((uint32_t)b.n, (uint32_t)b.m, a.r.band_pad, lo, hi);
            a.seg_entry[seg0 + t] = (uint32_t)s;
            a.seg_cells[seg0 + t] = dp ? b.n * aln_row_width((uint32_t)b.m, lo, hi) : 0;
            a.seg_runs[seg0 + t] = dp ? (uint32_t)(b.n + b.m) : 0;
            if (dp) { n_dp++; most = b.m > most ? b.m : most; }
        }
        if (lane < ALN_ROW_WORDS) a.rows[ALN_ROW_WORDS * s + lane] = lane == ALN_FLAGS ? (too_long ? ALN_TOO_LONG : ALN_ALIGNED) : 0;
        if (lane == 0) { n_long += too_long; n_segments += too_long ? 0 : ch.cnt - 1; }
    }
    n_dp = wave_sum(n_dp);
    if (most) max_agent(a.ctr + kCtrMostCols, most);
    if (lane == 0) {
        if (n_dp) add_agent(a.ctr + kCtrDpSegments, n_dp);
        if (n_long) add_agent(a.ctr + kCtrTooLong, n_long);
        if (n_segments) add_agent(a.ctr + kCtrSegments, n_segments);
    }
}

// The direction bytes of the DP segments [seg_lo, seg_hi), one wave per segment, the waves of a capped grid striding over them.  The
// matrix is swept in strips of 64 rows, lane l on row i0 + l, and a strip anti-diagonal by anti-diagonal: at step t lane l is at column
// j_lo + t - l, so that the cell above it is what lane l - 1 computed one step earlier and the cell above and left of it what lane l - 1
// computed two steps earlier.  H and F of a lane's own row stay in registers; H and E of the row above and the query's code come down one
// lane per step by a wave shift.  Lane 0 takes them from the last row of the strip above, which lane 63 left in LDS (row 0: the border),
// and the query's codes from a register block that the wave loads 64 columns at a time, reverse-complemented on load.  One direction
// byte per cell in band goes out; cells out of band are ALN_NEG and write nothing.  dir_base is the group's first direction byte.
__global__ __launch_bounds__(ALN_DP_THREADS) void aln_dp_kernel(AlnArgs a, uint64_t seg_lo, uint64_t seg_hi, uint64_t dir_base, uint32_t row_words)
{
    extern __shared__ int32_t s_above[];      // H then E of the row above the strip, by column
    int32_t *s_h = s_above, *s_e = s_above + row_words;
    const int32_t lane = (int32_t)threadIdx.x;
    const uint32_t q = a.r.q, e = a.r.e;
    uint64_t cells = 0;
    for (uint64_t seg = seg_lo + blockIdx.x; seg < seg_hi; seg += gridDim.x) {
        if (a.seg_cells[seg] == 0) continue;
        const uint64_t s = a.seg_entry[seg];
        const Chain ch = chain_of(a, s);
        const Between b = between_of(a, ch, seg - a.seg_offsets[s]);
        const int32_t n = (int32_t)b.n, m = (int32_t)b.m;
        int32_t lo, hi;
        aln_band((uint32_t)n, (uint32_t)m, a.r.band_pad, lo, hi);
        const uint32_t width = aln_row_width((uint32_t)m, lo, hi);
        uint8_t *dir = a.dir + (a.dir_offsets[seg] - dir_base);
        for (int32_t i0 = 1; i0 <= n; i0 += 64) {
            const int32_t i = i0 + lane, last_row = i0 + 63 < n ? i0 + 63 : n;
            const bool row = i <= n;
            const uint32_t r_code = row ? aln_code(ch.ref[b.r + (uint64_t)(i - 1)]) : 4;
            const int32_t j_lo = i0 + lo > 1 ? i0 + lo : 1, j_hi = last_row + hi < m ? last_row + hi : m;
            const int32_t my_first = i + lo > 1 ? i + lo : 1, my_last = i + hi < m ? i + hi : m;
            const int32_t row_start = aln_row_start(i, (uint32_t)m, lo, width);
            const int32_t steps = j_hi - j_lo + 64;
            int32_t h_left = ALN_NEG, f_left = ALN_NEG, h_diag = ALN_NEG, h_out = ALN_NEG, e_out = ALN_NEG;
            uint32_t q_out = 4, q_block = 4;
            for (int32_t t = 0; t < steps; t++) {
                if ((t & 63) == 0) {   // the codes of the next 64 columns, one per lane
                    const int32_t col = j_lo + t + lane;
                    q_block = col <= m ? aln_query_code(ch.read, ch.read_len, ch.rev, b.q + (uint64_t)(col - 1)) : 4;
                }
                const int32_t j = j_lo + t - lane;
                int32_t h_up = __shfl_up(h_out, 1, 64), e_up = __shfl_up(e_out, 1, 64);
                uint32_t q_code = __shfl_up(q_out, 1, 64);
                const uint32_t q_first = __shfl(q_block, t & 63, 64);
                if (lane == 0) {
                    q_code = q_first;
                    const bool above = j <= m && aln_in_band(i0 - 1, j, lo, hi), above_left = j - 1 <= m && aln_in_band(i0 - 1, j - 1, lo, hi);
                    if (i0 == 1) {
                        h_up = j <= m ? aln_border_h(0, j, lo, hi, q, e) : ALN_NEG;
                        e_up = ALN_NEG;
                        h_diag = aln_border_h(0, j - 1, lo, hi, q, e);
                    } else {
                        h_up = above ? s_h[j] : ALN_NEG;
                        e_up = above ? s_e[j] : ALN_NEG;
                        h_diag = j == 1 ? aln_border_h(i0 - 1, 0, lo, hi, q, e) : above_left ? s_h[j - 1] : ALN_NEG;
                    }
                }
                const bool active = row && j >= my_first && j <= my_last;
                h_out = ALN_NEG; e_out = ALN_NEG;
                if (active) {
                    if (j == 1) {   // column 0 is the border
                        h_left = aln_border_h(i, 0, lo, hi, q, e);
                        f_left = ALN_NEG;
                        if (lane != 0) h_diag = aln_border_h(i - 1, 0, lo, hi, q, e);
                    }
                    int32_t h, ee, f;
                    const uint32_t d = aln_cell(h_diag, h_up, e_up, h_left, f_left, aln_match(r_code, q_code), a.r.a, a.r.b, q, e, h, ee, f);
                    dir[(uint64_t)(i - 1) * width + (uint32_t)(j - row_start)] = (uint8_t)d;
                    cells++;
                    h_left = h; f_left = f; h_out = h; e_out = ee;
                    if (lane == 63) { s_h[j] = h; s_e[j] = ee; }
                } else {
                    h_left = ALN_NEG; f_left = ALN_NEG;
                }
                h_diag = h_up;
                q_out = q_code;
            }
            wave_fence();   // the next strip reads what lane 63 left
        }
    }
    cells = wave_sum(cells);
    if (lane == 0 && cells) add_agent(a.ctr + kCtrCells, cells);
}

// the run list of every DP segment of [seg_lo, seg_hi) from its direction bytes, one segment per thread: seg_runs becomes its length
__global__ __launch_bounds__(ALN_THREADS) void aln_trace_kernel(AlnArgs a, uint64_t seg_lo, uint64_t seg_hi, uint64_t dir_base)
{
    for (uint64_t seg = seg_lo + first_item(); seg < seg_hi; seg += item_step()) {
        if (a.seg_cells[seg] == 0) continue;
        const uint64_t s = a.seg_entry[seg];
        const Chain ch = chain_of(a, s);
        const Between b = between_of(a, ch, seg - a.seg_offsets[s]);
        int32_t lo, hi;
        aln_band((uint32_t)b.n, (uint32_t)b.m, a.r.band_pad, lo, hi);
        a.seg_runs[seg] = aln_trace(a.dir + (a.dir_offsets[seg] - dir_base), (uint32_t)b.n, (uint32_t)b.m, lo, hi,
                                    aln_row_width((uint32_t)b.m, lo, hi), a.runs + a.run_offsets[seg]);
    }
}

// the runs of a chain as they come, merged into its canonical CIGAR
struct Cigar {
    uint32_t *out;                            // where the words go, or nullptr to count alone
    uint32_t op = 0;
    uint64_t len = 0, n = 0, n_eq = 0, n_x = 0, n_ins = 0, n_del = 0, n_gaps = 0;

    __device__ void flush()
    {
        if (!len) return;
        if (out) out[n] = (uint32_t)len << 4 | op;
        n++;
        if (op == ALN_OP_EQ) n_eq += len;
        else if (op == ALN_OP_X) n_x += len;
        else { n_gaps++; if (op == ALN_OP_I) n_ins += len; else n_del += len; }
        len = 0;
    }
    __device__ void push(uint32_t o, uint64_t l)
    {
        if (!l) return;
        if (o != op) { flush(); op = o; }
        len += l;
    }
};

// Every aligned chain's CIGAR, one entry of sel per thread: the diagonal columns of every member compared base by base, a between part
// without DP as one gap run and one with DP as its run list, read from the last run to the first.  write == 0: the row and the score;
// write != 0: the words, behind g_offsets.  A chain that is TOO_LONG keeps its row of zeros.
__global__ __launch_bounds__(ALN_THREADS) void aln_emit_kernel(AlnArgs a, uint32_t write)
{
    uint64_t n_aligned = 0;
    for (uint64_t s = first_item(); s < a.n_sel; s += item_step()) {
        uint32_t *row = a.rows + ALN_ROW_WORDS * s;
        if (row[ALN_FLAGS] != ALN_ALIGNED) {
            if (!write) a.scores[s] = 0;
            continue;
        }
        const Chain ch = chain_of(a, s);
        Cigar cg;
        cg.out = write ? a.cigar + a.g_offsets[s] : nullptr;
        for (uint64_t t = 0; t < ch.cnt; t++) {
            uint64_t r, q, cols = a.r.k;
            anchor_of(a, ch, t, r, q);
            Between b = {};
            if (t + 1 < ch.cnt) { b = between_of(a, ch, t); cols = b.m0; }
            for (uint64_t x = 0; x < cols; x++)
                cg.push(aln_match(aln_code(ch.ref[r + x]), aln_query_code(ch.read, ch.read_len, ch.rev, q + x)) ? ALN_OP_EQ : ALN_OP_X, 1);
            if (b.n && b.m) {
                const uint64_t seg = a.seg_offsets[s] + t;
                const uint32_t *runs = a.runs + a.run_offsets[seg];
                for (uint32_t x = a.seg_runs[seg]; x > 0; x--) cg.push(runs[x - 1] & 15, runs[x - 1] >> 4);
            } else {
                cg.push(ALN_OP_D, b.n);
                cg.push(ALN_OP_I, b.m);
            }
        }
        cg.flush();
        if (write) continue;
        row[ALN_N_CIGAR] = (uint32_t)cg.n; row[ALN_N_EQ] = (uint32_t)cg.n_eq; row[ALN_N_X] = (uint32_t)cg.n_x; row[ALN_N_INS] = (uint32_t)cg.n_ins;
        row[ALN_N_DEL] = (uint32_t)cg.n_del; row[ALN_N_GAPS] = (uint32_t)cg.n_gaps;
        a.scores[s] = aln_score(a.r, cg.n_eq, cg.n_x, cg.n_ins, cg.n_del, cg.n_gaps);
        n_aligned++;
    }
    n_aligned = wave_sum(n_aligned);
    if (!write && (threadIdx.x & 63) == 0 && n_aligned) add_agent(a.ctr + kCtrAligned, n_aligned);
}

}  // namespace

struct ntk_align : Consumer {
    Pinned<uint64_t> h_stage;                              // kCtrWords words and four totals
    Pinned<uint64_t> h_offsets;                            // the direction offsets, where a run takes more than one group
    DeviceArray<uint32_t> d_rows;                          // the result: per entry of sel its row,
    DeviceArray<int64_t> d_scores;                         // its score,
    DeviceArray<uint64_t> d_g_offsets;                     // the n_sel + 1 ranges of the CIGARs ...
    DeviceArray<uint32_t> d_cigar;                         // ... and their words
    DeviceArray<uint64_t> d_seg_offsets;                   // the work: per entry its first segment;
    DeviceArray<uint32_t> d_seg_entry;                     // per segment its entry,
    DeviceArray<uint64_t> d_seg_cells, d_dir_offsets;      // its direction bytes and their scan,
    DeviceArray<uint32_t> d_seg_runs;                      // its runs,
    DeviceArray<uint64_t> d_run_offsets;                   // and the scan of their bounds;
    DeviceArray<uint8_t> d_dir;                            // the direction bytes of the largest group
    DeviceArray<uint32_t> d_runs;                          // the run lists
    DeviceArray<uint64_t> d_ctr;                           // kCtrWords words
    DeviceArray<char> d_tmp;                               // rocPRIM's temporary storage: held inside a run only
    bool held = false;                                     // a result is held (n_sel may be 0)
    uint64_t n_sel = 0, n_aligned = 0, n_too_long = 0, n_segments = 0, n_dp_segments = 0, dp_cells = 0, n_cigar = 0, n_groups = 0;
    int failed = 0;                                        // the status of a run that failed halfway

    uint64_t device_bytes() const
    {
        return d_rows.bytes() + d_scores.bytes() + d_g_offsets.bytes() + d_cigar.bytes() + d_seg_offsets.bytes() + d_seg_entry.bytes() +
               d_seg_cells.bytes() + d_dir_offsets.bytes() + d_seg_runs.bytes() + d_run_offsets.bytes() + d_dir.bytes() + d_runs.bytes() +
               d_ctr.bytes() + d_tmp.bytes();
    }

    // the result and every work array
    void release_all()
    {
        d_rows.release(); d_scores.release(); d_g_offsets.release(); d_cigar.release(); d_seg_offsets.release(); d_seg_entry.release();
        d_seg_cells.release(); d_dir_offsets.release(); d_seg_runs.release(); d_run_offsets.release(); d_dir.release(); d_runs.release();
        d_ctr.release(); d_tmp.release();
    }
};

namespace {

using Handle = ntk_align;
constexpr int kStageTotals = kCtrWords, kStageWords = kCtrWords + 4;

// what run_device refuses before any device call: the parameters ...
int check_params(const ntk_align_params *p)
{
    if (!p) return NTK_ERR_BAD_ARG;
    if (p->k < 1 || p->k > ALN_BYTE_MAX || p->a < 1 || p->a > ALN_BYTE_MAX || p->b < 1 || p->b > ALN_BYTE_MAX) return NTK_ERR_BAD_ARG;
    if (p->q > ALN_BYTE_MAX || p->e < 1 || p->e > ALN_BYTE_MAX) return NTK_ERR_BAD_ARG;
    if (p->band_pad > ALN_SEG_MAX || p->max_seg < 1 || p->max_seg > ALN_SEG_MAX) return NTK_ERR_BAD_ARG;
    if (p->work_mib && (p->work_mib < ALN_WORK_MIB_MIN || p->work_mib > ALN_WORK_MIB_MAX)) return NTK_ERR_BAD_ARG;
    return NTK_OK;
}

// ... and the arrays
int check_arrays(const Handle *m, const uint8_t *d_ref, const uint64_t *d_ref_offsets, const uint8_t *d_seq, const uint64_t *d_seq_offsets,
                 const uint64_t *d_c_offsets, const uint32_t *d_chain_rows, const uint64_t *d_m_offsets, const uint32_t *d_members,
                 const uint32_t *d_rpos, const uint32_t *d_qpos, const uint32_t *d_sel, uint64_t ref_bytes, uint64_t seq_bytes, uint64_t n_refs,
                 uint64_t n_reads, uint64_t n_chains, uint64_t n_members, uint64_t n_anchors, uint64_t n_sel)
{
    if (!m) return NTK_ERR_BAD_ARG;
    if ((n_chains >> 32) || (n_reads >> 32) || (n_refs >> 31) || (n_sel >> 32)) return NTK_ERR_BAD_ARG;
    if (!d_ref_offsets || ((uintptr_t)d_ref_offsets & 7) || !d_seq_offsets || ((uintptr_t)d_seq_offsets & 7)) return NTK_ERR_BAD_ARG;
    if (!d_c_offsets || ((uintptr_t)d_c_offsets & 7) || !d_m_offsets || ((uintptr_t)d_m_offsets & 7)) return NTK_ERR_BAD_ARG;
    if ((ref_bytes && !d_ref) || (seq_bytes && !d_seq)) return NTK_ERR_BAD_ARG;
    if (n_chains && (!d_chain_rows || ((uintptr_t)d_chain_rows & 3))) return NTK_ERR_BAD_ARG;
    if (n_members && (!d_members || ((uintptr_t)d_members & 3))) return NTK_ERR_BAD_ARG;
    if (n_anchors && (!d_rpos || !d_qpos || ((uintptr_t)d_rpos & 3) || ((uintptr_t)d_qpos & 3))) return NTK_ERR_BAD_ARG;
    if (n_sel && (!d_sel || ((uintptr_t)d_sel & 3))) return NTK_ERR_BAD_ARG;
    return NTK_OK;
}

inline unsigned grid_of(const Handle *m, uint64_t items, unsigned per_block = ALN_THREADS)
{
    return grid_for(items, per_block, (unsigned)m->n_cu * ALN_BLOCKS_PER_CU);
}

// the verification on the device: NTK_OK or the refusal; nothing held is touched
int verify(Handle *m, AlnArgs &a)
{
    int rc;
    hipStream_t st = m->stream;
    CT_HIPCHK(hipSetDevice(m->device));
    if ((rc = m->d_ctr.ensure(st, kCtrWords, grow_exact))) return rc;
    a.ctr = m->d_ctr.p;
    CT_HIPCHK(hipMemsetAsync(m->d_ctr.p, 0, kCtrWords * sizeof(uint64_t), st));
    uint64_t items = (a.n_refs > a.n_reads ? a.n_refs : a.n_reads) + 1;
    if (a.n_sel * 64 > items) items = a.n_sel * 64;
    hipLaunchKernelGGL(aln_verify_kernel, dim3(grid_of(m, items)), dim3(ALN_THREADS), 0, st, a);
    CT_HIPCHK(hipGetLastError());
    if ((rc = m->h_stage.read(st, m->d_ctr.p, 1))) return rc;
    if (m->h_stage.p[kCtrFlags] & ALN_BAD_ARG_FLAGS) return NTK_ERR_BAD_ARG;
    if (m->h_stage.p[kCtrFlags] & ALN_UNSUPPORTED_FLAGS) return NTK_ERR_UNSUPPORTED;
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

// A refused call changes nothing held: where the handle held nothing before the verification - no run yet, or a trim since - the
// counter words it allocated go again, so that stats reports 0 bytes as before the call
void drop_counters(Handle *m)
{
    if (m->held || !m->d_ctr.p) return;
    (void)hipStreamSynchronize(m->stream);
    m->d_ctr.release();
    (void)hipGetLastError();
}

// the DP and the traceback of the segments [seg_lo, seg_hi), whose direction bytes start at dir_base
int run_group(Handle *m, const AlnArgs &a, uint64_t seg_lo, uint64_t seg_hi, uint64_t dir_base, uint32_t row_words)
{
    hipStream_t st = m->stream;
    const unsigned dp_grid = grid_for(seg_hi - seg_lo, 1, (unsigned)m->n_cu * ALN_BLOCKS_PER_CU * kWaves);
    hipLaunchKernelGGL(aln_dp_kernel, dim3(dp_grid), dim3(ALN_DP_THREADS), 2 * row_words * sizeof(int32_t), st, a, seg_lo, seg_hi, dir_base, row_words);
    CT_HIPCHK(hipGetLastError());
    hipLaunchKernelGGL(aln_trace_kernel, dim3(grid_of(m, seg_hi - seg_lo)), dim3(ALN_THREADS), 0, st, a, seg_lo, seg_hi, dir_base);
    CT_HIPCHK(hipGetLastError());
    m->n_groups++;
    return NTK_OK;
}

// the whole run behind the verification; a failure in here marks the handle
int align(Handle *m, AlnArgs &a, uint64_t n_sel, uint64_t work_bytes)
{
    int rc;
    hipStream_t st = m->stream;
    uint64_t *stage = m->h_stage.p;
    if ((rc = m->d_rows.ensure(st, 8 * n_sel, grow_exact)) || (rc = m->d_scores.ensure(st, n_sel, grow_exact)) ||
        (rc = m->d_g_offsets.ensure(st, n_sel + 1, grow_exact)) || (rc = m->d_seg_offsets.ensure(st, n_sel + 1, grow_exact)))
        return rc;
    a.rows = m->d_rows.p; a.scores = m->d_scores.p; a.g_offsets = m->d_g_offsets.p; a.seg_offsets = m->d_seg_offsets.p;
    const auto items = rocprim::counting_iterator<uint64_t>(0);
    rc = with_tmp(m->d_tmp, st, grow_exact, [&](void *tmp, size_t &bytes) {
        return rocprim::exclusive_scan(tmp, bytes, rocprim::make_transform_iterator(items, SegmentCount{a.sel, a.m_offsets, n_sel}), a.seg_offsets,
                                       (uint64_t)0, (size_t)(n_sel + 1), rocprim::plus<uint64_t>(), st);
    });
    if (rc || (rc = m->h_stage.read(st, a.seg_offsets + n_sel, 1, kStageTotals))) return rc;
    const uint64_t n_seg = a.n_seg = stage[kStageTotals];
    if ((rc = m->d_seg_entry.ensure(st, n_seg, grow_exact)) || (rc = m->d_seg_cells.ensure(st, n_seg + 1, grow_exact)) ||
        (rc = m->d_dir_offsets.ensure(st, n_seg + 1, grow_exact)) || (rc = m->d_seg_runs.ensure(st, n_seg + 1, grow_exact)) ||
        (rc = m->d_run_offsets.ensure(st, n_seg + 1, grow_exact)))
        return rc;
    a.seg_entry = m->d_seg_entry.p; a.seg_cells = m->d_seg_cells.p; a.dir_offsets = m->d_dir_offsets.p; a.seg_runs = m->d_seg_runs.p;
    a.run_offsets = m->d_run_offsets.p;
    hipLaunchKernelGGL(aln_plan_kernel, dim3(grid_of(m, n_sel, kWaves)), dim3(ALN_THREADS), 0, st, a);
    CT_HIPCHK(hipGetLastError());
    rc = with_tmp(m->d_tmp, st, grow_exact, [&](void *tmp, size_t &bytes) {
        return rocprim::exclusive_scan(tmp, bytes, a.seg_cells, a.dir_offsets, (uint64_t)0, (size_t)(n_seg + 1), rocprim::plus<uint64_t>(), st);
    });
    if (rc) return rc;
    rc = with_tmp(m->d_tmp, st, grow_exact, [&](void *tmp, size_t &bytes) {
        return rocprim::exclusive_scan(tmp, bytes, a.seg_runs, a.run_offsets, (uint64_t)0, (size_t)(n_seg + 1), rocprim::plus<uint64_t>(), st);
    });
    if (rc) return rc;
    CT_HIPCHK(hipMemcpyAsync(stage + kStageTotals + 1, a.dir_offsets + n_seg, sizeof(uint64_t), hipMemcpyDeviceToHost, st));
    CT_HIPCHK(hipMemcpyAsync(stage + kStageTotals + 2, a.run_offsets + n_seg, sizeof(uint64_t), hipMemcpyDeviceToHost, st));
    if ((rc = m->h_stage.read(st, m->d_ctr.p, kCtrWords))) return rc;
    const uint64_t dir_bytes = stage[kStageTotals + 1], n_runs = stage[kStageTotals + 2];
    const uint32_t row_words = (uint32_t)stage[kCtrMostCols] + 1;
    m->n_too_long = stage[kCtrTooLong]; m->n_segments = stage[kCtrSegments]; m->n_dp_segments = stage[kCtrDpSegments];
    if ((rc = m->d_runs.ensure(st, n_runs, grow_exact))) return rc;
    a.runs = m->d_runs.p;
    if (m->n_dp_segments && dir_bytes <= work_bytes) {   // one group
        if ((rc = m->d_dir.ensure(st, dir_bytes, grow_exact))) return rc;
        a.dir = m->d_dir.p;
        if ((rc = run_group(m, a, 0, n_seg, 0, row_words))) return rc;
    } else if (m->n_dp_segments) {   // consecutive groups that fit: the offsets on the host give their borders
        if ((rc = m->h_offsets.ensure(n_seg + 1, grow_exact)) || (rc = m->h_offsets.read(st, a.dir_offsets, n_seg + 1))) return rc;
        const uint64_t *off = m->h_offsets.p;
        uint64_t most = 0;
        for (uint64_t lo = 0, hi; lo < n_seg; lo = hi) {
            for (hi = lo; hi < n_seg && off[hi + 1] - off[lo] <= work_bytes; hi++) {}
            most = off[hi] - off[lo] > most ? off[hi] - off[lo] : most;
        }
        if ((rc = m->d_dir.ensure(st, most, grow_exact))) return rc;
        a.dir = m->d_dir.p;
        for (uint64_t lo = 0, hi; lo < n_seg; lo = hi) {
            for (hi = lo; hi < n_seg && off[hi + 1] - off[lo] <= work_bytes; hi++) {}
            if ((rc = run_group(m, a, lo, hi, off[lo], row_words))) return rc;
        }
    }
    if (n_sel) {
        hipLaunchKernelGGL(aln_emit_kernel, dim3(grid_of(m, n_sel)), dim3(ALN_THREADS), 0, st, a, 0u);
        CT_HIPCHK(hipGetLastError());
    }
    rc = with_tmp(m->d_tmp, st, grow_exact, [&](void *tmp, size_t &bytes) {
        return rocprim::exclusive_scan(tmp, bytes, rocprim::make_transform_iterator(items, CigarCount{a.rows, n_sel}), a.g_offsets, (uint64_t)0,
                                       (size_t)(n_sel + 1), rocprim::plus<uint64_t>(), st);
    });
    if (rc || (rc = m->h_stage.read(st, a.g_offsets + n_sel, 1, kStageTotals + 3))) return rc;
    const uint64_t n_cigar = stage[kStageTotals + 3];
    if ((rc = m->d_cigar.ensure(st, n_cigar, grow_exact))) return rc;
    a.cigar = m->d_cigar.p;
    if (n_cigar) {
        hipLaunchKernelGGL(aln_emit_kernel, dim3(grid_of(m, n_sel)), dim3(ALN_THREADS), 0, st, a, 1u);
        CT_HIPCHK(hipGetLastError());
    }
    if ((rc = m->h_stage.read(st, m->d_ctr.p, kCtrWords))) return rc;
    m->n_aligned = stage[kCtrAligned]; m->dp_cells = stage[kCtrCells];
    m->n_cigar = n_cigar;
    return NTK_OK;
}

}  // namespace

extern "C" {

int ntk_align_create(ntk_ctx *ctx, ntk_align **out)
{
    if (!ctx || !out) return NTK_ERR_BAD_ARG;
    *out = nullptr;
    ntk_align *m = new (std::nothrow) ntk_align();
    if (!m) return NTK_ERR_NOMEM;
    int rc = m->bind(ctx, 0, 0);
    if (rc) { delete m; return rc; }
    if ((rc = m->h_stage.alloc(kStageWords))) { delete m; return rc; }
    *out = m;
    return NTK_OK;
}

int ntk_align_trim(ntk_align *m)
{
    if (!m) return NTK_ERR_BAD_ARG;
    CT_HIPCHK(hipSetDevice(m->device));
    CT_HIPCHK(hipStreamSynchronize(m->stream));
    m->release_all();
    m->h_offsets.release();
    (void)hipGetLastError();
    m->held = false;
    m->n_sel = m->n_aligned = m->n_too_long = m->n_segments = m->n_dp_segments = m->dp_cells = m->n_cigar = m->n_groups = 0;
    m->failed = 0;
    return NTK_OK;
}

void ntk_align_destroy(ntk_align *m)
{
    if (!m) return;
    (void)ntk_align_trim(m);
    m->h_stage.release();
    (void)hipGetLastError();
    delete m;
}

int ntk_align_run_device(ntk_align *m, const uint8_t *d_ref, uint64_t ref_bytes, const uint64_t *d_ref_offsets, uint64_t n_refs,
                         const uint8_t *d_seq, uint64_t seq_bytes, const uint64_t *d_seq_offsets, uint64_t n_reads, const uint64_t *d_c_offsets,
                         const uint32_t *d_chain_rows, const uint64_t *d_m_offsets, const uint32_t *d_members, const uint32_t *d_rpos,
                         const uint32_t *d_qpos, uint64_t n_chains, uint64_t n_members, uint64_t n_anchors, const uint32_t *d_sel, uint64_t n_sel,
                         const struct ntk_align_params *params)
{
    int rc = check_arrays(m, d_ref, d_ref_offsets, d_seq, d_seq_offsets, d_c_offsets, d_chain_rows, d_m_offsets, d_members, d_rpos, d_qpos, d_sel,
                          ref_bytes, seq_bytes, n_refs, n_reads, n_chains, n_members, n_anchors, n_sel);
    if (rc || (rc = check_params(params))) return rc;
    AlnArgs a = {};
    a.ref = d_ref; a.seq = d_seq; a.ref_offsets = d_ref_offsets; a.seq_offsets = d_seq_offsets;
    a.ref_bytes = ref_bytes; a.seq_bytes = seq_bytes; a.n_refs = n_refs; a.n_reads = n_reads;
    a.c_offsets = d_c_offsets; a.chain_rows = d_chain_rows; a.m_offsets = d_m_offsets; a.members = d_members; a.rpos = d_rpos; a.qpos = d_qpos;
    a.sel = d_sel; a.n_chains = n_chains; a.n_members = n_members; a.n_anchors = n_anchors; a.n_sel = n_sel;
    a.r.k = params->k; a.r.a = params->a; a.r.b = params->b; a.r.q = params->q; a.r.e = params->e; a.r.band_pad = params->band_pad;
    a.r.max_seg = params->max_seg;
    if ((rc = verify(m, a))) {
        drop_counters(m);
        return rc;
    }
    // the run starts over: nothing of the result held so far is part of the new one
    m->held = true; m->failed = 0;
    m->n_sel = n_sel;
    m->n_aligned = m->n_too_long = m->n_segments = m->n_dp_segments = m->dp_cells = m->n_cigar = m->n_groups = 0;
    rc = align(m, a, n_sel, (uint64_t)(params->work_mib ? params->work_mib : ALN_WORK_MIB_DEFAULT) << 20);
    drop_tmp(m);
    if (rc) m->failed = rc;
    return rc;
}

int ntk_align_read(ntk_align *m, uint32_t *rows, int64_t *scores, uint64_t *g_offsets, uint32_t *cigar, uint64_t cap_sel, uint64_t cap_cigar,
                   uint64_t *n_sel, uint64_t *n_cigar)
{
    if (!m || !n_sel || !n_cigar || (cap_sel && (!rows || !scores)) || (cap_cigar && !cigar)) return NTK_ERR_BAD_ARG;
    if (m->failed) return m->failed;
    *n_sel = m->held ? m->n_sel : 0;
    *n_cigar = m->held ? m->n_cigar : 0;
    if (!m->held) return NTK_OK;
    if (m->n_sel > cap_sel || m->n_cigar > cap_cigar) return NTK_ERR_CAPACITY;
    if (!g_offsets) return NTK_OK;   // the sizes alone
    hipStream_t st = m->stream;
    CT_HIPCHK(hipSetDevice(m->device));
    CT_HIPCHK(hipMemcpyAsync(g_offsets, m->d_g_offsets.p, (m->n_sel + 1) * sizeof(uint64_t), hipMemcpyDeviceToHost, st));
    if (m->n_sel) {
        CT_HIPCHK(hipMemcpyAsync(rows, m->d_rows.p, 8 * m->n_sel * sizeof(uint32_t), hipMemcpyDeviceToHost, st));
        CT_HIPCHK(hipMemcpyAsync(scores, m->d_scores.p, m->n_sel * sizeof(int64_t), hipMemcpyDeviceToHost, st));
    }
    if (m->n_cigar) CT_HIPCHK(hipMemcpyAsync(cigar, m->d_cigar.p, m->n_cigar * sizeof(uint32_t), hipMemcpyDeviceToHost, st));
    CT_HIPCHK(hipStreamSynchronize(st));
    return NTK_OK;
}

int ntk_align_result_device(ntk_align *m, const uint32_t **d_rows, const int64_t **d_scores, const uint64_t **d_g_offsets, const uint32_t **d_cigar,
                            uint64_t *n_sel, uint64_t *n_cigar)
{
    if (!m || !d_rows || !d_scores || !d_g_offsets || !d_cigar || !n_sel || !n_cigar) return NTK_ERR_BAD_ARG;
    if (m->failed) return m->failed;
    const bool held = m->held;
    *d_rows = held && m->n_sel ? m->d_rows.p : nullptr;
    *d_scores = held && m->n_sel ? m->d_scores.p : nullptr;
    *d_g_offsets = held ? m->d_g_offsets.p : nullptr;
    *d_cigar = held && m->n_cigar ? m->d_cigar.p : nullptr;
    *n_sel = held ? m->n_sel : 0;
    *n_cigar = held ? m->n_cigar : 0;
    return NTK_OK;
}

int ntk_align_stats(ntk_align *m, struct ntk_align_stats *out)
{
    if (!m || !out) return NTK_ERR_BAD_ARG;
    if (m->failed) return m->failed;
    CT_HIPCHK(hipSetDevice(m->device));
    CT_HIPCHK(hipStreamSynchronize(m->stream));
    out->n_sel = m->n_sel; out->n_aligned = m->n_aligned; out->n_too_long = m->n_too_long; out->n_segments = m->n_segments;
    out->n_dp_segments = m->n_dp_segments; out->dp_cells = m->dp_cells; out->n_cigar = m->n_cigar; out->n_groups = m->n_groups;
    out->device_bytes = m->device_bytes();
    return NTK_OK;
}

}  // extern "C"
