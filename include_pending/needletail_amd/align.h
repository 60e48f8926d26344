/*
 * needletail_amd/align.h — base-level alignment of reported chains (libneedletail_amd_align.so): the gaps between a chain's anchors are
 * filled by banded affine dynamic programming on the device, over the chains where needletail_amd/chain.h left them, a selection such as
 * needletail_amd/mapping.h's reported chains and the two sequence batches where they lie.  The result is, per selected chain, an exact,
 * canonical CIGAR with its counts and score, held on the device.  It is exact and deterministic: integer arithmetic only.  The library
 * reads bases only through the two batches it is given, takes pointers, not handles, and links nothing but the core.
 *
 * THE RULE.  (csrc/ntk_align_rule.hpp states it as code.)
 *   Input.     The reference batch d_ref of ref_bytes with d_ref_offsets[n_refs + 1] and the read batch d_seq of seq_bytes with
 *              d_seq_offsets[n_reads + 1] (u64): the device batch layout of needletail_amd.h, the offsets the packer's record starts.  The
 *              arrays of ntk_chain_result_device: d_c_offsets[n_reads + 1] (u64), d_chain_rows[8 * n_chains] (u32), d_m_offsets[n_chains +
 *              1] (u64) and d_members[n_members] (u32); the anchor arrays d_rpos and d_qpos (u32, n_anchors each); d_sel[n_sel] (u32), the
 *              chains to align - ntk_mapping_result_device's d_out is such a list.  From a chain row only score (word 0) and ref_rev
 *              (word 2) are used.  Duplicates in d_sel are allowed, in any order; each entry is aligned independently.
 *   Bases.     code(byte) is 0..3 for Aa Cc Gg TtUu and 4 for every other byte; two bases MATCH iff their codes are equal and below 4.
 *              The length of record r is max(off[r + 1] - off[r], 1) - 1: the last byte is the break byte.  On the reverse strand
 *              (ref_rev odd) the query is the reverse complement of the read: query position p is read position len - 1 - p,
 *              complemented (code 4 stays 4), and an anchor's query start is len - qpos - k.  Everything below is in reference-forward
 *              coordinates, as in PAF and SAM.
 *   Parameters. struct ntk_align_params, eight u32: k, the seed length of the lists, 1..255; a, the match score, 1..255 (2); b, the
 *              mismatch penalty, 1..255 (4); q, gap open, 0..255 (4), and e, gap extend, 1..255 (2): a gap of length L costs q + L * e;
 *              band_pad 0..4095 (64); max_seg 1..4095 (2048); work_mib 0 or 16..4096, 0 for 256.  Anything else is NTK_ERR_BAD_ARG
 *              before any device call.
 *   Verified.  On the device, before anything held is touched: the two record offset arrays and c_offsets are non-decreasing and their
 *              last entries at most ref_bytes, seq_bytes and n_chains; every selected index is < n_chains and inside [c_offsets[0],
 *              c_offsets[n_reads]); for every selected chain m_offsets[c] <= m_offsets[c + 1] <= n_members, it has at least one member,
 *              every member is < n_anchors, along its members dr = rpos_i - rpos_prev >= 1 and dq >= 1 (dq = qpos_i - qpos_prev where
 *              ref_rev is even and qpos_prev - qpos_i where it is odd), 1 <= score < 2^31, ref = ref_rev >> 1 < n_refs, and re = rpos(last
 *              member) + k is at most the reference's length and qe = max(qpos first, qpos last) + k at most the read's.  A failure of
 *              any of these is NTK_ERR_BAD_ARG.  re - rs >= 2^28 or qe - qs >= 2^28 is NTK_ERR_UNSUPPORTED.  NTK_ERR_BAD_ARG goes first.
 *              A refused call changes nothing that is held.  No input can make a kernel read outside the arrays it was given.  Sequence
 *              bytes are never verified: any byte is a valid byte.
 *   Segments.  For consecutive members i, i + 1 of a chain: m0 = min(dr, dq, k) diagonal columns, then the BETWEEN part, n = dr - m0
 *              reference bases against m = dq - m0 query bases, aligned globally.  The last member contributes k diagonal columns.
 *              Diagonal columns are compared base by base, = or X: the anchors are not trusted to match.  With n == 0 or m == 0 the
 *              between part is one gap run, or nothing; otherwise it is the DP below.  max(n, m) > max_seg for any segment makes the
 *              whole chain TOO_LONG: flag bit 1, everything else zero, an empty CIGAR; its segments count in no statistic.
 *   DP.        Cell (i, j) is IN BAND iff lo <= j - i <= hi, lo = min(0, m - n) - band_pad, hi = max(0, m - n) + band_pad; cells out of
 *              band are minus infinity (-2^29 on the device: real values stay above -2^23, what derives from it below -2^28).
 *              H[0][0] = 0, E[0][*] = F[*][0] = -inf;
 *                E[i][j] = max(E[i-1][j], H[i-1][j] - q) - e      F[i][j] = max(F[i][j-1], H[i][j-1] - q) - e
 *                H[i][j] = max(H[i-1][j-1] + s, E[i][j], F[i][j]),  s = a on a MATCH and -b otherwise;
 *              the diagonal term is absent where i == 0 or j == 0.
 *   Traceback. From (n, m) in state H.  In H: if i, j > 0 and H == H[i-1][j-1] + s, emit = or X and move diagonally; else if i > 0 and
 *              H == E, go to state E; else to state F.  In E: emit D; if E == H[i-1][j] - q - e go to H (opening is preferred over
 *              extending), else stay; i -= 1 in both cases.  F is symmetric with I.  So: diagonal first, then deletion, then insertion,
 *              and ties place gaps leftmost: AAAA against AAA is 1D3=.
 *   Result.    Indexed by position in d_sel.  rows, eight u32 per entry: flags (bit 0 aligned, bit 1 too long), n_cigar, n_eq, n_x,
 *              n_ins (bases), n_del (bases), n_gaps (runs of I or D), 0.  scores (i64) = a * n_eq - b * n_x - q * n_gaps - e * (n_ins +
 *              n_del).  g_offsets[n_sel + 1] (u64) and cigar[] (u32, len << 4 | op, BAM's codes I = 1, D = 2, = is 7, X = 8).  The CIGAR
 *              is CANONICAL: no zero lengths and no two adjacent runs of one op, across segment borders too.
 *   Groups.    A DP segment's direction bytes are n * min(hi - lo + 1, m), at most 4095 * 4095 < 16 MiB.  Where the sum over all
 *              segments exceeds work_mib MiB, the segments run in consecutive GROUPS, each the longest run of segments from where the
 *              last ended whose bytes fit; n_groups counts them, 0 without a DP segment.
 *   Not here.  Extension beyond a chain's ends and soft clips, z-drop, a two-piece gap cost, re-ranking chains by alignment score, and
 *              a place in tools/lib_fuzz.py.
 *
 * How.  aln_verify_kernel takes one record start and one read's chain range per thread and one wave per selected chain, lanes striding
 * over its members, and raises a flag word that the host reads back.  A scan (rocPRIM) of the members less one numbers the segments.
 * aln_plan_kernel, one wave per selected chain: lanes stride over the chain's segments twice, for the TOO_LONG flag, then for every
 * segment's direction bytes and run bound; two scans place them.  aln_dp_kernel, the hot path, one wave per DP segment, the waves of a
 * capped grid striding over them: the matrix is swept in strips of 64 rows, lane l on row i0 + l, anti-diagonal by anti-diagonal, so
 * that a lane's upper neighbours are what lane l - 1 computed one and two steps earlier.  H and F of a lane's own row stay in registers,
 * H and E of the row above and the query's code come down one lane per step by a wave shift, lane 0 takes them from the last row of the
 * strip above, which lane 63 left in LDS (8 B per column of the widest segment, per wave), and the query's codes from a register block
 * loaded 64 columns at a time, reverse-complemented on load; the reference's code is loaded once per strip.  One direction byte goes
 * out per cell in band: H's source in two bits (=, E, F, X), "E opened", "F opened".  aln_trace_kernel, one DP segment per thread, walks
 * the bytes back into the segment's run list, at most n + m runs.  aln_emit_kernel, one selected chain per thread, runs twice: it
 * compares the diagonal columns, adds gap runs and run lists and merges them, first for the row, the score and the CIGAR's length, then,
 * behind one more scan, for the words.  Sequences are read from global memory, not staged in LDS; small segments take the same route as
 * large ones.  Every kernel that loops has a capped grid.  Nothing here has been tuned.
 *
 * Every call returns a status code of needletail_amd.h.  run_device, read, stats and trim are SYNCHRONOUS: they return when the work
 * they queued on the context's stream is done.  result_device is host-side only.  A handle is used by one thread at a time, like its
 * context, and must be destroyed before its context.
 *
 * A run_device that fails halfway through its work on the device (NTK_ERR_NOMEM, NTK_ERR_HIP) leaves the handle marked: read,
 * result_device and stats return that status again until the next run_device.  Every refusal comes before any device call, except the
 * verification of the arrays on the device, which comes before anything held is touched.  The verification needs the counter words: a
 * call it refuses on a handle that held nothing - before any run, or behind a trim - frees them again, so that the handle holds nothing
 * afterwards either.
 *
 * Memory on the device (ntk_align_stats reports the sum), all of it freed by trim.  The result: 32 + 8 + 8 B per selected chain and 8
 * more (the rows, scores and g_offsets) and 4 B per CIGAR word.  Work arrays: 8 B per selected chain and 8 more (its first segment); 32 B
 * per segment of a selected chain and 28 more (its entry, its direction bytes and run bound and the scans of both); 4 B per run bound,
 * n + m per DP segment (the run lists); the direction bytes of the largest group; 7 counter words.  Every array grows to exactly the
 * largest size needed so far.  The scans' scratch, rocPRIM's temporary storage, which rocPRIM sizes, is held INSIDE a run_device only and
 * freed before the call returns: it is part of the call's peak and of nothing stats reports.
 */
#ifndef NEEDLETAIL_AMD_ALIGN_H
#define NEEDLETAIL_AMD_ALIGN_H

#include "needletail_amd.h"

#ifdef __cplusplus
extern "C" {
#endif

typedef struct ntk_align ntk_align;

struct ntk_align_params {
    uint32_t k;                 /* the seed length of the lists the anchors came from, 1..255                                  */
    uint32_t a;                 /* the score of a match, 1..255                                                                */
    uint32_t b;                 /* the penalty of a mismatch, 1..255                                                           */
    uint32_t q;                 /* gap open, 0..255                                                                            */
    uint32_t e;                 /* gap extend, 1..255                                                                          */
    uint32_t band_pad;          /* the padding of the band around the two diagonals, 0..4095                                   */
    uint32_t max_seg;           /* the largest between part that is aligned, 1..4095                                           */
    uint32_t work_mib;          /* the direction workspace of one group in MiB, 16..4096, or 0 for 256                         */
};

/* (a struct tag, not a typedef: ntk_align_stats is also the function that fills it) */
struct ntk_align_stats {
    uint64_t n_sel;             /* of the held result                                                                          */
    uint64_t n_aligned;         /* entries with flag bit 0                                                                     */
    uint64_t n_too_long;        /* entries with flag bit 1                                                                     */
    uint64_t n_segments;        /* between parts of the aligned entries                                                        */
    uint64_t n_dp_segments;     /* those with n > 0 and m > 0                                                                  */
    uint64_t dp_cells;          /* their cells in band with i, j >= 1                                                          */
    uint64_t n_cigar;           /* the length of cigar                                                                         */
    uint64_t n_groups;          /* the groups the DP segments ran in                                                           */
    uint64_t device_bytes;      /* device memory the handle holds now                                                          */
};

/* The handle holds no result and works on ctx's device and stream. */
int ntk_align_create(ntk_ctx *ctx, ntk_align **out);
void ntk_align_destroy(ntk_align *m);
/* Aligns the selected chains (synchronous); the result replaces the one held.  The arrays are verified and the parameters checked as
 * the head comment says.  An offset array NULL or not 8-byte aligned; with its size != 0, d_ref, d_seq NULL, or d_chain_rows, d_members,
 * d_rpos, d_qpos or d_sel NULL or not 4-byte aligned; n_chains, n_reads or n_sel >= 2^32 or n_refs >= 2^31; params NULL:
 * NTK_ERR_BAD_ARG.  n_sel == 0 is NTK_OK with an empty result. */
int ntk_align_run_device(ntk_align *m, const uint8_t *d_ref, uint64_t ref_bytes, const uint64_t *d_ref_offsets, uint64_t n_refs,
                         const uint8_t *d_seq, uint64_t seq_bytes, const uint64_t *d_seq_offsets, uint64_t n_reads, const uint64_t *d_c_offsets,
                         const uint32_t *d_chain_rows, const uint64_t *d_m_offsets, const uint32_t *d_members, const uint32_t *d_rpos,
                         const uint32_t *d_qpos, uint64_t n_chains, uint64_t n_members, uint64_t n_anchors, const uint32_t *d_sel, uint64_t n_sel,
                         const struct ntk_align_params *params);
/* The held result in host arrays (synchronous): rows has 8 * *n_sel entries, scores *n_sel, g_offsets *n_sel + 1, cigar *n_cigar.  rows
 * and scores hold `cap_sel` entries and cigar `cap_cigar`: a capacity too small is NTK_ERR_CAPACITY with *n_sel and *n_cigar the sizes
 * needed and NOTHING written; NULL arrays with capacities 0 ask for the sizes that way.  g_offsets == NULL: only the sizes are set.
 * Before any run: *n_sel = *n_cigar = 0 and nothing is written. */
int ntk_align_read(ntk_align *m, uint32_t *rows, int64_t *scores, uint64_t *g_offsets, uint32_t *cigar, uint64_t cap_sel, uint64_t cap_cigar,
                   uint64_t *n_sel, uint64_t *n_cigar);
/* The held result where it lies on the device; host-side only: queues nothing and waits for nothing.  The arrays are those of read;
 * the pointers stay valid until the next run_device, trim or destroy.  Before any run: NULL pointers and sizes 0. */
int ntk_align_result_device(ntk_align *m, const uint32_t **d_rows, const int64_t **d_scores, const uint64_t **d_g_offsets, const uint32_t **d_cigar,
                            uint64_t *n_sel, uint64_t *n_cigar);
/* What the handle holds and what the last run did (synchronous). */
int ntk_align_stats(ntk_align *m, struct ntk_align_stats *out);
/* Frees the result and every work array (synchronous).  read answers sizes 0 afterwards, as before any run. */
int ntk_align_trim(ntk_align *m);

#ifdef __cplusplus
}
#endif

#endif /* NEEDLETAIL_AMD_ALIGN_H */
