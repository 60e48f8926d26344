/*
 * needletail_amd/mapping.h — mark the primary and secondary chains of every read and give each a mapping quality
 * (libneedletail_amd_mapping.so): minimap2's mm_set_parent with a hard mask level, mm_select_sub and the chain-only mapping quality of
 * minimap2 2.17, run on the device over the chains of a read batch where needletail_amd/chain.h left them.  The result is a row of sixteen
 * words per chain - the columns of a PAF line - and per read the chains to report, held on the device.  It is exact and deterministic:
 * integer arithmetic only.  The library never reads a base: it works on the chain and anchor arrays alone and links nothing but the core.
 *
 * THE RULE.  (csrc/ntk_map_rule.hpp states it as code.)
 *   Input.     The arrays of ntk_chain_result_device: d_c_offsets[n_reads + 1] (u64), d_chain_rows[8 * n_chains] (u32),
 *              d_m_offsets[n_chains + 1] (u64) and d_members[n_members] (u32); the anchor arrays d_rpos and d_qpos (u32, n_anchors each);
 *              the four sizes.  The library takes pointers, not handles; any arrays of that shape are valid input.  From a chain row
 *              only score (word 0) and ref_rev (word 2) are used: everything else is recomputed from the members, so a row's end
 *              coordinates need not be trusted.  Chains in front of c_offsets[0] or behind c_offsets[n_reads] belong to no read: they
 *              are not looked at and their rows are zero.  n_chains >= 2^32 or n_reads >= 2^32 is NTK_ERR_BAD_ARG.
 *   Verified.  On the device, before anything held is touched: both offset arrays are non-decreasing, c_offsets[n_reads] <= n_chains
 *              and m_offsets[n_chains] <= n_members; every chain of a read has at least one member; every member of such a chain is
 *              < n_anchors; along a chain's members dr = rpos_i - rpos_prev >= 1 and dq >= 1, dq = qpos_i - qpos_prev where the chain's
 *              ref_rev is even and qpos_prev - qpos_i where it is odd; 1 <= score < 2^31.  A failure of any of these is
 *              NTK_ERR_BAD_ARG.  A read with 2^16 chains or more (the parent rule is quadratic per read), a chain whose re or qe does
 *              not fit a u32 and a chain whose blen does not fit a u32 are NTK_ERR_UNSUPPORTED.  NTK_ERR_BAD_ARG goes first.  A refused
 *              call changes nothing that is held.  No input can make a kernel read outside the arrays it was given.
 *   Parameters. struct ntk_mapping_params, eight u32: k, the seed length of the lists, 1..255; mask_level_pm 0..1000 (500);
 *              pri_ratio_pm 0..1000 (800); best_n 0..65535 (5); min_chain_score >= 1 (40); three reserved words that must be 0.
 *              Anything else is NTK_ERR_BAD_ARG before any device call.
 *   Per chain. rs = rpos(first member), re = rpos(last member) + k; qs = min(qpos first, qpos last), qe = max(qpos first, qpos last) + k
 *              (on the reverse strand the first member has the largest qpos); cnt the number of members; mlen = k + sum of
 *              min(dr, dq, k) and blen = k + sum of max(dr, dq) over consecutive members: the matching and the block length of a PAF
 *              line.
 *   Rank.      A read's chains by (score descending, chain index ascending).
 *   Parent.    Chains i and j of one read OVERLAP iff ol = min(qe_i, qe_j) - max(qs_i, qs_j) > 0 and
 *              ol * 1000 > mask_level_pm * min(qe_i - qs_i, qe_j - qs_j): on the query only, whatever the reference and strand.
 *              link[i] is the LOWEST-ranked chain of rank below i's that overlaps i.  Without one, i is PRIMARY and parent[i] = i;
 *              otherwise parent[i] = parent[link[i]]: the root of the link tree.  For a primary p, n_sub is the number of other chains
 *              whose parent is p and subsc the largest score among them, 0 without any.
 *   Secondaries. A non-primary chain is ELIGIBLE iff score * 1000 >= pri_ratio_pm * score(parent), and KEPT iff it is eligible and
 *              fewer than best_n eligible chains of its read have a lower rank.
 *   Quality.   Non-primaries get 0.  For a primary, in u64:
 *                lg8(v), v >= 1: e = ilog2(v); m = v << (31 - e); frac = 0;
 *                                8 times: m = (m * m) >> 31; frac <<= 1; if (m >> 32) { frac |= 1; m >>= 1; }   lg8 = e << 8 | frac
 *                pen  = min(min(score, 100), 10 * min(cnt, 10))
 *                sub  = max(subsc, min_chain_score);  d = score > sub ? score - sub : 0
 *                t    = (40 * pen * d * lg8(score)) / score
 *                raw  = ((t * 45426) >> 16) / 25600
 *                mapq = clamp(raw - ((lg8(n_sub + 1) * 771 + 32768) >> 16), 0, 60)
 *              lg8(v) is floor(256 * log2 v); the whole is minimap2 2.17's 40 * pen * (1 - sub / score) * ln score -
 *              4.343 * ln(n_sub + 1) with uniq_ratio 1, to within 1.
 *   Result.    rows[n_chains] of sixteen u32: qs, qe, rs, re, ref_rev, score, cnt, mlen, blen, parent (a batch chain index), subsc,
 *              n_sub, mapq, flags (bit 0 primary, bit 1 kept secondary), rank (within the read), 0.  order[n_chains] (u32): under
 *              c_offsets, each read's chain indices by rank; 0 for a chain of no read.  out_offsets[n_reads + 1] (u64) and out[] (u32):
 *              per read the chains to report, primaries and kept secondaries, by rank.  Per read a row of four u32: chains, primaries,
 *              kept secondaries, the mapq of the rank-0 chain (0 without a chain).
 *   Not here.  Base-level alignment, minimap2's rep_len / uniq_ratio terms and its soft mask level (mask_len).
 *
 * How.  mp_verify_kernel takes one chain, one offset and one member per thread (a member's chain by a binary search of m_offsets) and
 * raises a flag word that the host reads back.  mp_span_kernel, one wave per chain: lanes stride over the chain's consecutive member
 * pairs and a wave reduction gives the two sums; where the verification could not bound a blen it runs once without writing, for the
 * exact sums.  mp_keys_kernel writes (0x7FFFFFFF - score) << 32 | chain per chain and one segmented radix sort (rocPRIM) over the reads
 * ranks them.  mp_parent_kernel, one wave per read, the waves of a capped grid striding over the reads: the read's intervals are staged
 * in rank order, in LDS where the read has at most 512 chains and in a work array otherwise; for the chain of rank i, lane l tests the
 * chain of rank 64 s + l of every strip s below i, one ballot and a find-first-set give link, and the loop ends at the first strip with
 * a hit; parent[i] = parent[link] is known by then, since link < i.  A second pass over the ranks, 64 at a time, counts the eligible
 * chains in front of each with a ballot, writes parent, flags and rank and adds every child to its primary's n_sub and subsc; a third
 * gives every primary its mapq.  A scan (rocPRIM) of the reported counts gives out_offsets and mp_emit_kernel writes out, one chain
 * per thread.  Every kernel that loops has a grid of at most 8 blocks per compute unit.  Nothing here has been tuned.
 *
 * Every call returns a status code of needletail_amd.h.  run_device, read, stats and trim are SYNCHRONOUS: they return when the work
 * they queued on the context's stream is done.  result_device is host-side only.  A handle is used by one thread at a time, like its
 * context, and must be destroyed before its context.
 *
 * A run_device that fails halfway through its work on the device (NTK_ERR_NOMEM, NTK_ERR_HIP) leaves the handle marked: read,
 * result_device and stats return that status again until the next run_device.  Every refusal comes before any device call, except the
 * verification of the arrays on the device, which comes before anything held is touched.
 *
 * Memory on the device (ntk_mapping_stats reports the sum), all of it freed by trim.  The result: 64 + 4 B per chain (the rows and
 * order), 8 + 16 B per read and 8 more (out_offsets and the read rows) and 4 B per reported chain (out).  Work arrays: 24 B per chain
 * (the rank keys twice - the first copy holds the intervals in rank order once the sort is done - the parents and the places among the
 * reported), 4 B per read and 4 more (the reported counts), 6 counter words.  Every array grows to exactly the largest size needed so
 * far.  The scan's and the sort's scratch, rocPRIM's temporary storage, which rocPRIM sizes, is held INSIDE a run_device only and freed
 * before the call returns: it is part of the call's peak and of nothing stats reports.
 */
#ifndef NEEDLETAIL_AMD_MAPPING_H
#define NEEDLETAIL_AMD_MAPPING_H

#include "needletail_amd.h"

#ifdef __cplusplus
extern "C" {
#endif

typedef struct ntk_mapping ntk_mapping;

struct ntk_mapping_params {
    uint32_t k;                 /* the seed length of the lists the anchors came from, 1..255                                 */
    uint32_t mask_level_pm;     /* the mask level in per mille, 0..1000                                                        */
    uint32_t pri_ratio_pm;      /* the least score of a secondary in per mille of its parent's, 0..1000                        */
    uint32_t best_n;            /* the most secondaries kept per read, 0..65535                                                */
    uint32_t min_chain_score;   /* the floor of sub in the mapping quality, >= 1                                               */
    uint32_t reserved[3];       /* must be 0                                                                                   */
};

/* (a struct tag, not a typedef: ntk_mapping_stats is also the function that fills it) */
struct ntk_mapping_stats {
    uint64_t n_reads;           /* of the held result                                                                          */
    uint64_t n_chains;          /* the length of its chain arrays                                                              */
    uint64_t n_primary;         /* primary chains                                                                              */
    uint64_t n_secondary;       /* kept secondaries                                                                            */
    uint64_t n_reported;        /* the length of out: the two together                                                         */
    uint64_t most_chains;       /* chains of the read that has most                                                            */
    uint64_t reserved;          /* 0                                                                                           */
    uint64_t device_bytes;      /* device memory the handle holds now                                                          */
};

/* The handle holds no result and works on ctx's device and stream. */
int ntk_mapping_create(ntk_ctx *ctx, ntk_mapping **out);
void ntk_mapping_destroy(ntk_mapping *m);
/* Marks the chains of a read batch (synchronous); the result replaces the one held.  The arrays are verified and the parameters
 * checked as the head comment says.  d_c_offsets or d_m_offsets NULL or not 8-byte aligned; with n_chains != 0, d_chain_rows NULL or
 * not 4-byte aligned; with n_members != 0, d_members NULL or not 4-byte aligned; with n_anchors != 0, d_rpos or d_qpos NULL or not
 * 4-byte aligned; params NULL: NTK_ERR_BAD_ARG.  n_reads == 0, n_chains == 0 and reads without chains are NTK_OK with empty ranges. */
int ntk_mapping_run_device(ntk_mapping *m, const uint64_t *d_c_offsets, const uint32_t *d_chain_rows, const uint64_t *d_m_offsets,
                           const uint32_t *d_members, const uint32_t *d_rpos, const uint32_t *d_qpos, uint64_t n_reads, uint64_t n_chains,
                           uint64_t n_members, uint64_t n_anchors, const struct ntk_mapping_params *params);
/* The held result in host arrays (synchronous): rows has 16 * *n_chains entries, order *n_chains, out_offsets n_reads + 1, out *n_out,
 * read_rows 4 * n_reads.  rows and order hold `cap_chains` chains and out `cap_out`: a capacity too small is NTK_ERR_CAPACITY with
 * *n_chains and *n_out the sizes needed and NOTHING written; NULL arrays with capacities 0 ask for the sizes that way.
 * out_offsets == NULL: only the sizes are set; read_rows may be NULL.  Before any run: *n_chains = *n_out = 0 and nothing is written. */
int ntk_mapping_read(ntk_mapping *m, uint32_t *rows, uint32_t *order, uint64_t *out_offsets, uint32_t *out, uint32_t *read_rows,
                     uint64_t cap_chains, uint64_t cap_out, uint64_t *n_chains, uint64_t *n_out);
/* The held result where it lies on the device; host-side only: queues nothing and waits for nothing.  The arrays are those of read;
 * the pointers stay valid until the next run_device, trim or destroy.  Before any run: NULL pointers and sizes 0. */
int ntk_mapping_result_device(ntk_mapping *m, const uint32_t **d_rows, const uint32_t **d_order, const uint64_t **d_out_offsets,
                              const uint32_t **d_out, const uint32_t **d_read_rows, uint64_t *n_chains, uint64_t *n_out);
/* What the handle holds and what the last run did (synchronous). */
int ntk_mapping_stats(ntk_mapping *m, struct ntk_mapping_stats *out);
/* Frees the result and every work array (synchronous).  read answers sizes 0 afterwards, as before any run. */
int ntk_mapping_trim(ntk_mapping *m);

#ifdef __cplusplus
}
#endif

#endif /* NEEDLETAIL_AMD_MAPPING_H */
