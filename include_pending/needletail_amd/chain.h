/*
 * needletail_amd/chain.h — chain seed anchors into colinear chains (libneedletail_amd_chain.so): minimap2's chaining recurrence over a
 * fixed predecessor window and its backtrack, run on the device over a per-read CSR of anchors.  The result is a per-read CSR of chains
 * with their member anchors, held on the device: where each read lies - a reference, a strand, an interval on both sequences and a
 * score.  It is exact and deterministic: integer arithmetic only.  The library never reads a base: it works on the anchor arrays alone
 * (needletail_amd/seed_index.h makes them) and links nothing but the core.
 *
 * THE RULE.  (csrc/ntk_chain_rule.hpp states it as code.)
 *   Input.     The arrays of ntk_seed_index_result_device: d_a_offsets[n_reads + 1] (u64), d_ref_rev, d_rpos, d_qpos (u32, n each;
 *              ref_rev = ref << 1 | rev).  The library takes the four pointers and the two sizes, not a handle; any arrays of that
 *              shape are valid input.  n >= 2^32 or n_reads >= 2^31 is NTK_ERR_BAD_ARG.  The arrays are VERIFIED on the device before
 *              anything held is touched: offsets not non-decreasing or offsets[n_reads] > n, or an anchor of a read whose triple
 *              (ref_rev, rpos, qpos) is not strictly greater than its predecessor's in that read, is NTK_ERR_BAD_ARG; a read with 2^23
 *              anchors or more is NTK_ERR_UNSUPPORTED (with k <= 255 a score then stays below 2^31).  Anchors in front of offsets[0] or
 *              behind offsets[n_reads] belong to no read: they are not looked at, their f is 0 and their p none.  A refused call
 *              changes nothing that is held.  No input can make a kernel read outside the arrays it was given.
 *   Parameters. struct ntk_chain_params, eight u32: k, the seed length of the lists, 1..255; max_dist 1..2^31 - 1 (minimap2's default
 *              is 5000); bw 0..max_dist (500); h 1..512 (64); min_score >= 1 (40); min_cnt >= 1 (3); two reserved words that must be
 *              0.  Anything else is NTK_ERR_BAD_ARG before any device call.
 *   Pair.      Anchors j < i of one read with equal ref_rev.  dr = rpos_i - rpos_j; dq = qpos_i - qpos_j where rev is 0 and
 *              qpos_j - qpos_i where rev is 1.  j may precede i iff 1 <= dr <= max_dist, 1 <= dq <= max_dist and
 *              dd = |dr - dq| <= bw.  Then gain = min(dr, dq, k) and gap = dd == 0 ? 0 : ((dd * k * 41) >> 12) + (ilog2(dd) >> 1):
 *              minimap2 2.17's 0.01 * span * dd + log2(dd) / 2 in integers.
 *   Recurrence. f[i] = max(k, max over j of f[j] + gain - gap), as i32.  j runs over the at most h anchors directly in front of i in
 *              the read's order that have i's ref_rev.  p[i] is the j that attains the maximum; ties go to the LARGEST j; p[i] is
 *              none (0xFFFFFFFF) where no candidate exceeds k.  The window is by index: distance only decides whether a pair counts.
 *   Runs.      A run is a maximal range of a read's anchors that has one ref_rev and whose consecutive rpos differ by at most
 *              max_dist.  No pair crosses a run, because the order is by rpos: a gap of exactly max_dist stays in one run, max_dist + 1
 *              splits it.  Runs are the unit of parallel work and a consequence of the rule, not a part of it.
 *   Chains.    Per read, anchors are visited in order of (f descending, index ascending).  An anchor that is already used, or whose
 *              f < min_score, starts nothing.  Otherwise p is walked from the anchor until none or a used anchor t, and every walked
 *              anchor is marked used.  The score is f[i], or f[i] - f[t] where the walk stopped at a used anchor t.  The chain is kept
 *              iff score >= min_score and it has at least min_cnt members.  Walked anchors stay used even when the chain is dropped:
 *              this is minimap2's rule.
 *   Result.    c_offsets[n_reads + 1] (u64): read q's chains [c_offsets[q], c_offsets[q + 1]), in the order found.  Per chain a row of
 *              eight u32: score, n_members, ref_rev, rpos and qpos of the first member, rpos and qpos of the last member, one zero
 *              word.  m_offsets[n_chains + 1] (u64) and members[] (u32): chain c's members [m_offsets[c], m_offsets[c + 1]), indices
 *              into the batch's anchor arrays, ascending within a chain.  Per anchor f (i32) and p (u32: an index into the batch's
 *              arrays, or none).  Per read a row of four u32: n_anchors, n_chains, the anchors in kept chains, the best score (0
 *              without a chain).
 *   Not here.  Primary and secondary marking, mapping quality, alignment, chain merging and minimap2's max_skip heuristic.
 *
 * How.  ch_verify_kernel takes one anchor and one offset per thread (an anchor's read by a binary search of the offsets) and raises a
 * flag word that the host reads back.  ch_heads_kernel marks run starts, a scan (rocPRIM) numbers the runs and ch_runs_kernel writes
 * where each starts.  ch_dp_kernel, the recurrence: one wave per run, the waves of a capped grid striding over the runs; the wave walks
 * i in order, lane l scores predecessor i - 1 - l in strips of 64 up to h, from a per-wave ring in LDS of the last 512 anchors' rpos,
 * qpos and f (6 KiB per wave); the 64 candidates are reduced with one cross-lane maximum of (score << 32 | j), which is the rule's
 * tie-break; lane 0 writes f and p.  ch_keys_kernel writes (0x7FFFFFFF - f) << 32 | index per anchor and one segmented radix sort
 * (rocPRIM) over the reads orders them.  ch_walk_kernel, one thread per read, backtracks twice: a first pass counts chains and members,
 * two scans give the bases, the totals are read back and the result arrays grown, and a second pass writes rows and members, each
 * chain's members back to front.  Every kernel that loops has a grid of at most 8 blocks per compute unit.  Nothing here has been
 * tuned: the window strips, the one thread per read of the backtrack and the grid caps are first choices.
 *
 * Every call returns a status code of needletail_amd.h.  run_device, read, stats and trim are SYNCHRONOUS: they return when the work
 * they queued on the context's stream is done.  result_device is host-side only.  A handle is used by one thread at a time, like its
 * context, and must be destroyed before its context.
 *
 * A run_device that fails halfway through its work on the device (NTK_ERR_NOMEM, NTK_ERR_HIP) leaves the handle marked: read,
 * result_device and stats return that status again until the next run_device.  Every refusal comes before any device call, except the
 * verification of the arrays on the device, which comes before anything held is touched.
 *
 * Memory on the device (ntk_chain_stats reports the sum), all of it freed by trim.  The result: 8 B per anchor (f and p), 8 + 16 B per
 * read and 8 more (c_offsets and the read rows), 32 + 8 B per chain and 8 more (the chain rows and m_offsets) and 4 B per member.  Work
 * arrays: 25 B per anchor (run heads and their scan, the visit keys twice, the used marks), 4 B per run and 4 more (where each run
 * starts), 16 B per read and 16 more (the chain and member counts and the member bases), 4 counter words.  Every array grows to
 * exactly the largest size needed so far.  The scans' and the sort's scratch, rocPRIM's temporary storage, which rocPRIM sizes, is held
 * INSIDE a run_device only and freed before the call returns: it is part of the call's peak and of nothing stats reports.
 */
#ifndef NEEDLETAIL_AMD_CHAIN_H
#define NEEDLETAIL_AMD_CHAIN_H

#include "needletail_amd.h"

#ifdef __cplusplus
extern "C" {
#endif

typedef struct ntk_chain ntk_chain;

struct ntk_chain_params {
    uint32_t k;                 /* the seed length of the lists the anchors came from, 1..255                                 */
    uint32_t max_dist;          /* the largest dr and dq of a pair, 1..2^31 - 1                                                */
    uint32_t bw;                /* the largest |dr - dq| of a pair, 0..max_dist                                                */
    uint32_t h;                 /* the predecessor window, 1..512                                                              */
    uint32_t min_score;         /* of a kept chain, >= 1                                                                       */
    uint32_t min_cnt;           /* members of a kept chain, >= 1                                                               */
    uint32_t reserved[2];       /* must be 0                                                                                   */
};

/* (a struct tag, not a typedef: ntk_chain_stats is also the function that fills it) */
struct ntk_chain_stats {
    uint64_t n_reads;           /* of the held result                                                                          */
    uint64_t n_anchors;         /* the length of its anchor arrays                                                             */
    uint64_t n_runs;            /* runs of its reads                                                                           */
    uint64_t longest_run;       /* anchors of the longest run                                                                  */
    uint64_t n_chains;          /* kept chains                                                                                 */
    uint64_t n_members;         /* their members                                                                               */
    uint64_t reserved;          /* 0                                                                                           */
    uint64_t device_bytes;      /* device memory the handle holds now                                                          */
};

/* The handle holds no result and works on ctx's device and stream. */
int ntk_chain_create(ntk_ctx *ctx, ntk_chain **out);
void ntk_chain_destroy(ntk_chain *c);
/* Chains the anchors of a read batch (synchronous); the result replaces the one held.  The arrays are verified and the parameters
 * checked as the head comment says.  d_a_offsets NULL or not 8-byte aligned; with n_anchors != 0, d_ref_rev, d_rpos or d_qpos NULL or
 * not 4-byte aligned; params NULL: NTK_ERR_BAD_ARG.  n_reads == 0, n_anchors == 0 and reads without anchors are NTK_OK with empty
 * ranges. */
int ntk_chain_run_device(ntk_chain *c, const uint64_t *d_a_offsets, const uint32_t *d_ref_rev, const uint32_t *d_rpos, const uint32_t *d_qpos,
                         uint64_t n_reads, uint64_t n_anchors, const struct ntk_chain_params *params);
/* The held result in host arrays (synchronous): c_offsets has n_reads + 1 entries, chain_rows 8 * *n_chains, m_offsets *n_chains + 1,
 * members *n_members, f and p n_anchors each, read_rows 4 * n_reads.  chain_rows and m_offsets hold `cap_chains` chains and members
 * `cap_members`: a capacity too small is NTK_ERR_CAPACITY with *n_chains and *n_members the sizes needed and NOTHING written; NULL
 * arrays with capacities 0 ask for the sizes that way.  c_offsets == NULL: only the sizes are set; f, p and read_rows may be NULL.
 * Before any run: *n_chains = *n_members = 0 and nothing is written. */
int ntk_chain_read(ntk_chain *c, uint64_t *c_offsets, uint32_t *chain_rows, uint64_t *m_offsets, uint32_t *members, int32_t *f, uint32_t *p,
                   uint32_t *read_rows, uint64_t cap_chains, uint64_t cap_members, uint64_t *n_chains, uint64_t *n_members);
/* The held result where it lies on the device; host-side only: queues nothing and waits for nothing.  The arrays are those of read;
 * the pointers stay valid until the next run_device, trim or destroy.  Before any run: NULL pointers and sizes 0. */
int ntk_chain_result_device(ntk_chain *c, const uint64_t **d_c_offsets, const uint32_t **d_chain_rows, const uint64_t **d_m_offsets,
                            const uint32_t **d_members, const int32_t **d_f, const uint32_t **d_p, const uint32_t **d_read_rows,
                            uint64_t *n_chains, uint64_t *n_members);
/* What the handle holds and what the last run did (synchronous). */
int ntk_chain_stats(ntk_chain *c, struct ntk_chain_stats *out);
/* Frees the result and every work array (synchronous).  read answers sizes 0 afterwards, as before any run. */
int ntk_chain_trim(ntk_chain *c);

#ifdef __cplusplus
}
#endif

#endif /* NEEDLETAIL_AMD_CHAIN_H */
