// The rule of the alignment library (ntk_align.hip, include_pending/needletail_amd/align.h).  Plain C++ without any device call, so that
// it also compiles with g++: the CPU suite sweeps aln_segment_host - the same cell, band, storage and traceback functions the kernels
// call, driven by a row-major loop instead of the kernel's anti-diagonal sweep - against the host model (tests/test_align_rule.py), also
// under the sanitizers.  Integer arithmetic only.
//
// Bases.  aln_code: 0..3 for Aa Cc Gg TtUu, 4 for every other byte; two bases match iff their codes are equal and below 4.  Band.  Cell
// (i, j) of an n x m between part is in band iff lo <= j - i <= hi, lo = min(0, m - n) - band_pad, hi = max(0, m - n) + band_pad.  Cells.
// E = max(E_up, H_up - q) - e; F = max(F_left, H_left - q) - e; H = max(H_diag + s, E, F); cells out of band are ALN_NEG.  Traceback.  From
// (n, m) in state H: diagonal first, then E (deletion), then F (insertion); inside a gap, opening is preferred over extending.
#pragma once

#include <stdint.h>

#if defined(__HIPCC__) || defined(__CUDACC__)
#define ALN_FN __host__ __device__ inline
#else
#define ALN_FN inline
#include <vector>
#endif

// The geometry of the kernels.  aln_dp_kernel runs blocks of one wave, one DP segment per wave at a time; the other kernels run blocks
// of ALN_THREADS.  Every kernel that loops does so with a grid of at most ALN_BLOCKS_PER_CU blocks per compute unit (the DP kernel, whose
// blocks are a quarter as large, four times as many).  First choices, none measured.
constexpr uint32_t ALN_THREADS = 256;
constexpr uint32_t ALN_DP_THREADS = 64;
constexpr uint32_t ALN_BLOCKS_PER_CU = 8;

constexpr int32_t ALN_NEG = -(1 << 29);                    // minus infinity: real values stay above -2^23, what derives from this below -2^28
constexpr uint32_t ALN_BYTE_MAX = 255;                     // of k, a, b, q and e
constexpr uint32_t ALN_SEG_MAX = 4095;                     // of band_pad and max_seg
constexpr uint32_t ALN_WORK_MIB_MIN = 16, ALN_WORK_MIB_MAX = 4096, ALN_WORK_MIB_DEFAULT = 256;
constexpr uint64_t ALN_SPAN_MAX = (uint64_t)1 << 28;       // re - rs and qe - qs stay below this: a CIGAR length has 28 bits
constexpr uint32_t ALN_SCORE_MAX = 0x7FFFFFFFu;
constexpr uint32_t ALN_ROW_WORDS = 8;
// the words of a row
constexpr uint32_t ALN_FLAGS = 0, ALN_N_CIGAR = 1, ALN_N_EQ = 2, ALN_N_X = 3, ALN_N_INS = 4, ALN_N_DEL = 5, ALN_N_GAPS = 6;
constexpr uint32_t ALN_ALIGNED = 1, ALN_TOO_LONG = 2;      // the flags of a row
constexpr uint32_t ALN_OP_I = 1, ALN_OP_D = 2, ALN_OP_EQ = 7, ALN_OP_X = 8;   // BAM's codes
// a direction byte: where H came from in bits 0-1, "E opened here" and "F opened here"
constexpr uint32_t ALN_SRC_EQ = 0, ALN_SRC_E = 1, ALN_SRC_F = 2, ALN_SRC_X = 3, ALN_E_OPEN = 4, ALN_F_OPEN = 8;
// what the verification raises: the first six are NTK_ERR_BAD_ARG, the last NTK_ERR_UNSUPPORTED
constexpr uint32_t ALN_BAD_OFFSETS = 1, ALN_NO_MEMBER = 2, ALN_BAD_MEMBER = 4, ALN_BAD_ORDER = 8, ALN_BAD_SCORE = 16, ALN_BAD_SEL = 32,
                   ALN_BAD_END = 64, ALN_LONG_SPAN = 128;
constexpr uint32_t ALN_BAD_ARG_FLAGS = ALN_BAD_OFFSETS | ALN_NO_MEMBER | ALN_BAD_MEMBER | ALN_BAD_ORDER | ALN_BAD_SCORE | ALN_BAD_SEL | ALN_BAD_END;
constexpr uint32_t ALN_UNSUPPORTED_FLAGS = ALN_LONG_SPAN;

struct aln_rule_params {
    uint32_t k, a, b, q, e, band_pad, max_seg;
};

// 0..3 for Aa Cc Gg TtUu, 4 for every other byte
ALN_FN uint32_t aln_code(uint8_t c)
{
    switch (c | 0x20) {
    case 'a': return 0;
    case 'c': return 1;
    case 'g': return 2;
    case 't': case 'u': return 3;
    default: return 4;
    }
}
// the complement of a code; 4 stays 4
ALN_FN uint32_t aln_comp(uint32_t code) { return code < 4 ? 3 - code : 4; }
ALN_FN bool aln_match(uint32_t x, uint32_t y) { return x == y && x < 4; }

// the length of the record between two record starts: the last byte is the break byte
ALN_FN uint64_t aln_record_len(uint64_t begin, uint64_t end) { return (end - begin > 1 ? end - begin : 1) - 1; }

// the code of query position p of a read of `len` bases at `read`: on the reverse strand the reverse complement
ALN_FN uint32_t aln_query_code(const uint8_t *read, uint64_t len, uint32_t rev, uint64_t p)
{
    return rev ? aln_comp(aln_code(read[len - 1 - p])) : aln_code(read[p]);
}

// the steps of two consecutive members of a chain on strand rev, and the diagonal columns in front of their between part
ALN_FN void aln_step(uint32_t rev, uint32_t rpos_j, uint32_t qpos_j, uint32_t rpos_i, uint32_t qpos_i, int64_t &dr, int64_t &dq)
{
    dr = (int64_t)rpos_i - (int64_t)rpos_j;
    dq = rev ? (int64_t)qpos_j - (int64_t)qpos_i : (int64_t)qpos_i - (int64_t)qpos_j;
}
ALN_FN int64_t aln_m0(int64_t dr, int64_t dq, uint32_t k)
{
    const int64_t least = dr < dq ? dr : dq;
    return least < (int64_t)k ? least : (int64_t)k;
}

// the band of an n x m between part
ALN_FN void aln_band(uint32_t n, uint32_t m, uint32_t band_pad, int32_t &lo, int32_t &hi)
{
    const int32_t d = (int32_t)m - (int32_t)n;
    lo = (d < 0 ? d : 0) - (int32_t)band_pad;
    hi = (d > 0 ? d : 0) + (int32_t)band_pad;
}
ALN_FN bool aln_in_band(int32_t i, int32_t j, int32_t lo, int32_t hi) { return j - i >= lo && j - i <= hi; }

// H of a cell of row 0 or column 0: a gap run from the corner where the cell is in band
ALN_FN int32_t aln_border_h(int32_t i, int32_t j, int32_t lo, int32_t hi, uint32_t q, uint32_t e)
{
    if (i == 0 && j == 0) return 0;
    if (!aln_in_band(i, j, lo, hi)) return ALN_NEG;
    return -(int32_t)(q + (uint32_t)(i + j) * e);
}

// The direction bytes of a between part lie row by row: row i (1..n) holds `width` bytes, from column aln_row_start on.  The width is the
// band's, but never more than m, so that a segment takes at most n * m bytes.
ALN_FN uint32_t aln_row_width(uint32_t m, int32_t lo, int32_t hi)
{
    const uint32_t band = (uint32_t)(hi - lo) + 1;
    return band < m ? band : m;
}
ALN_FN int32_t aln_row_start(int32_t i, uint32_t m, int32_t lo, uint32_t width)
{
    const int32_t first = i + lo > 1 ? i + lo : 1, last = (int32_t)m - (int32_t)width + 1;
    return first < last ? first : last;
}
ALN_FN uint64_t aln_dir_at(int32_t i, int32_t j, uint32_t m, int32_t lo, uint32_t width)
{
    return (uint64_t)(i - 1) * width + (uint32_t)(j - aln_row_start(i, m, lo, width));
}

// One cell: H, E and F and its direction byte from the three neighbours; s is a on a match and -b otherwise.
ALN_FN uint32_t aln_cell(int32_t h_diag, int32_t h_up, int32_t e_up, int32_t h_left, int32_t f_left, bool match, uint32_t a, uint32_t b,
                         uint32_t q, uint32_t e, int32_t &h, int32_t &ee, int32_t &f)
{
    const int32_t open_e = h_up - (int32_t)q, open_f = h_left - (int32_t)q;
    const int32_t diag = h_diag + (match ? (int32_t)a : -(int32_t)b);
    uint32_t dir = 0;
    if (open_e >= e_up) { ee = open_e - (int32_t)e; dir |= ALN_E_OPEN; } else ee = e_up - (int32_t)e;
    if (open_f >= f_left) { f = open_f - (int32_t)e; dir |= ALN_F_OPEN; } else f = f_left - (int32_t)e;
    h = diag;
    if (ee > h) h = ee;
    if (f > h) h = f;
    return dir | (h == diag ? (match ? ALN_SRC_EQ : ALN_SRC_X) : h == ee ? ALN_SRC_E : ALN_SRC_F);
}

// The traceback of an n x m between part over its direction bytes: the runs (len << 4 | op) from the LAST to the first, at most n + m of
// them; returns their number.  A walk that left the band would end there: it never does on bytes the cells above wrote.
ALN_FN uint32_t aln_trace(const uint8_t *dir, uint32_t n, uint32_t m, int32_t lo, int32_t hi, uint32_t width, uint32_t *runs)
{
    int32_t i = (int32_t)n, j = (int32_t)m;
    uint32_t state = 0, n_runs = 0, op = 0, len = 0;
    while (i > 0 || j > 0) {
        uint32_t now;
        if (i > 0 && j > 0) {
            if (!aln_in_band(i, j, lo, hi)) break;
            const uint32_t d = dir[aln_dir_at(i, j, m, lo, width)], src = d & 3;
            if (state == 0 && (src == ALN_SRC_E || src == ALN_SRC_F)) { state = src; continue; }
            if (state == 0) { now = src == ALN_SRC_EQ ? ALN_OP_EQ : ALN_OP_X; i--; j--; }
            else if (state == ALN_SRC_E) { now = ALN_OP_D; if (d & ALN_E_OPEN) state = 0; i--; }
            else { now = ALN_OP_I; if (d & ALN_F_OPEN) state = 0; j--; }
        } else if (i > 0) { now = ALN_OP_D; i--; }   // column 0: a deletion run to the corner
        else { now = ALN_OP_I; j--; }                // row 0: an insertion run
        if (now == op) { len++; continue; }
        if (len) runs[n_runs++] = len << 4 | op;
        op = now; len = 1;
    }
    if (len) runs[n_runs++] = len << 4 | op;
    return n_runs;
}

// the score of a row's counts
ALN_FN int64_t aln_score(const aln_rule_params &p, uint64_t n_eq, uint64_t n_x, uint64_t n_ins, uint64_t n_del, uint64_t n_gaps)
{
    return (int64_t)(p.a * n_eq) - (int64_t)(p.b * n_x) - (int64_t)(p.q * n_gaps) - (int64_t)(p.e * (n_ins + n_del));
}

// the number of j in [0, n) with a[j] <= x: the read of chain x is one less where the offsets a are non-decreasing.  Terminates and
// stays inside [0, n] on any array.
ALN_FN uint64_t aln_at_or_before(const uint64_t *a, uint64_t n, uint64_t x)
{
    uint64_t lo = 0, hi = n;
    while (lo < hi) {
        const uint64_t mid = lo + (hi - lo) / 2;
        if (a[mid] <= x) lo = mid + 1; else hi = mid;
    }
    return lo;
}

#if !defined(__HIPCC__) && !defined(__CUDACC__)
// A between part on the host, n, m >= 1: the cells row by row, then the traceback.  ref and qry hold codes.  Returns the runs from the
// first to the last; *score is H[n][m] and *cells the number of cells in band.
inline std::vector<uint32_t> aln_segment_host(const uint8_t *ref, uint32_t n, const uint8_t *qry, uint32_t m, const aln_rule_params &p,
                                              int32_t *score, uint64_t *cells)
{
    int32_t lo, hi;
    aln_band(n, m, p.band_pad, lo, hi);
    const uint32_t width = aln_row_width(m, lo, hi);
    std::vector<uint8_t> dir((uint64_t)n * width, 0xFF);
    std::vector<int32_t> h_prev(m + 1), e_prev(m + 1, ALN_NEG), h_now(m + 1), e_now(m + 1);
    for (uint32_t j = 0; j <= m; j++) h_prev[j] = aln_border_h(0, (int32_t)j, lo, hi, p.q, p.e);
    *cells = 0;
    for (uint32_t i = 1; i <= n; i++) {
        h_now[0] = aln_border_h((int32_t)i, 0, lo, hi, p.q, p.e);
        e_now[0] = ALN_NEG;
        int32_t f = ALN_NEG;
        for (uint32_t j = 1; j <= m; j++) {
            if (!aln_in_band((int32_t)i, (int32_t)j, lo, hi)) { h_now[j] = e_now[j] = f = ALN_NEG; continue; }
            int32_t h, ee, ff;
            dir[aln_dir_at((int32_t)i, (int32_t)j, m, lo, width)] =
                (uint8_t)aln_cell(h_prev[j - 1], h_prev[j], e_prev[j], h_now[j - 1], f, aln_match(ref[i - 1], qry[j - 1]), p.a, p.b, p.q, p.e, h, ee, ff);
            h_now[j] = h; e_now[j] = ee; f = ff;
            ++*cells;
        }
        h_prev.swap(h_now); e_prev.swap(e_now);
    }
    *score = h_prev[m];
    std::vector<uint32_t> runs(n + m);
    runs.resize(aln_trace(dir.data(), n, m, lo, hi, width, runs.data()));
    return std::vector<uint32_t>(runs.rbegin(), runs.rend());
}
#endif
