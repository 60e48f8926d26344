/*
 * needletail_amd/seed_index.h — seed reads against references (libneedletail_amd_seed_index.so): a minimizer index of a reference batch
 * held on the device, and the minimizer lists of a read batch matched against it.  The result is a per-read CSR of seed hits - what
 * minimap2 calls anchors - that is exact, deterministic and ordered for chaining.  The library never reads a base: it works on
 * minimizer-list CSRs alone (needletail_amd/minimizer_list.h makes them) and links nothing but the core.
 *
 * THE RULE.
 *   Input lists.  A list is what ntk_minimizer_list_result_device hands out: d_offsets[n_records + 1] (u64), d_pos[n] (u64),
 *              d_values[n] (u64), d_info[n] (u32: bit 0 = strand flag, bits 31:1 = span, which is ignored here).  The library takes the
 *              four pointers and the two sizes, not a handle; any arrays of that shape are valid input.  Unlike the minimizer list, this
 *              library VERIFIES its lists on the device before it uses them: offsets not non-decreasing, offsets[n_records] > n,
 *              n >= 2^32 or n_records >= 2^31 is NTK_ERR_BAD_ARG; a pos >= 2^32 is NTK_ERR_UNSUPPORTED.  Entries in front of offsets[0] or
 *              behind offsets[n_records] belong to no record and are ignored (their pos too).  A refused call changes nothing that is
 *              held.  No input can make a kernel read outside the arrays it was given.
 *   Index.     (build_device, from the list of a reference batch.)  Every entry i of reference record r is one occurrence
 *              (value_i, r, pos_i, strand_i).  Occurrences are held sorted by (value, r, pos) - entry order within equal values.  The
 *              index holds the distinct values (keys, ascending), each key's range of occurrences, and per occurrence
 *              ref = r << 1 | strand (u32) and rpos (u32).  occ(key) is the length of its range.  A build replaces the index held and
 *              drops a held match result.
 *   Match.     (match_device, from the list of a read batch, with max_occ and max_anchors.)  Every entry of read q is a seed
 *              (value, qpos, qstrand).  A seed is ABSENT: its value is not a key; REPETITIVE: max_occ != 0 and occ(value) > max_occ
 *              (minimap2's mid_occ / -f rule; occ == max_occ is kept); a HIT otherwise.  A hit makes one anchor per occurrence of its
 *              key: (ref_rev = r << 1 | (strand ^ qstrand), rpos, qpos).  rev = 1 means the read matches the reference's reverse strand:
 *              forward anchors of one alignment share rpos - qpos, reverse ones share rpos + qpos.
 *   Order.     The anchors of read q are held in ascending order of (ref_rev, rpos, qpos).  That triple is unique within a read of a
 *              real list, so the order is total and does not depend on how it was produced; a_offsets[q] .. a_offsets[q + 1] is read
 *              q's range (u64).
 *   Rows.      Per read one row of four u32: n_seeds, n_hit, n_repetitive, n_absent; n_seeds = n_hit + n_repetitive + n_absent.
 *   Capacity.  If max_anchors != 0 and the batch makes more anchors than that, the call returns NTK_ERR_CAPACITY before any anchor
 *              array is grown: the rows and stats.n_anchors (the number needed) are valid, no anchors are held (read answers *n = 0
 *              and empty ranges), and the caller splits the batch or raises max_occ's bite.  A batch that makes 2^32 anchors or more
 *              is refused the same way whatever max_anchors says.
 *   Spectrum.  hist[c], c = 1..n_bins - 1, is the number of keys with occ == c; hist[n_bins - 1] also takes every larger occ, and
 *              hist[0] = 0.  It is what a user picks max_occ from: minimap2 takes the occ at which the top fraction f of keys is cut.
 *   Meaning.   (What the rule means; the library does not enforce it.)  k, w, path and order belong to the lists: the caller makes both
 *              lists with the same ones, or the anchors mean nothing - the library cannot know them and does not pretend to.  On a
 *              forward-only path every strand flag is 0, so every rev is 0.  A k-mer equal to its own reverse complement carries
 *              whatever flag the path's tie rule gave it: its rev is formally defined and biologically meaningless.
 *
 * How.  Build: si_verify_kernel checks the offsets and the positions and raises a flag word; si_owner_kernel searches every entry's
 * record in the offsets; a stable radix sort (rocPRIM) orders (value -> entry index) - entry order already is (record, pos) order, so
 * stability gives the occurrence order; si_heads_kernel marks the first occurrence of each value, a scan numbers the keys, and
 * si_pack_kernel writes keys, ranges, ref and rpos.  si_spectrum_kernel walks the ranges (bins below 1024 in LDS, agent-scope adds).
 * Match: si_lookup_kernel takes one seed per thread, searches the keys (a binary search), classifies the seed and writes its anchor
 * count; an exclusive scan gives every seed's base and the total; si_rows_kernel, one wave per read, sums the rows and writes a_offsets.
 * The total is read back: the capacity rule and the growth of the anchor arrays happen there.  si_fill_kernel takes one ANCHOR per thread
 * and searches the bases for its seed, so a seed with 10 000 occurrences is spread over 10 000 threads.  si_sort_kernel takes one block
 * per read with at most 2048 anchors and sorts (ref_rev << 32 | rpos, qpos) in LDS (24 KiB); reads with more anchors are copied to
 * compact arrays (si_widen_kernel), go through two stable segmented radix sorts (rocPRIM), by qpos and then by the 64-bit key, and are
 * copied back (si_narrow_kernel).  Every kernel that loops has a grid of at most 8 blocks per compute unit.  Nothing here has been
 * tuned: the lookup by binary search, the tile length and the grid caps are first choices.
 *
 * Every call returns a status code of needletail_amd.h.  build_device, spectrum, match_device, read, stats and trim are SYNCHRONOUS:
 * they return when the work they queued on the context's stream is done.  result_device is host-side only.  A handle is used by one
 * thread at a time, like its context, and must be destroyed before its context.
 *
 * A build_device or match_device that fails halfway through its work on the device (NTK_ERR_NOMEM, NTK_ERR_HIP) leaves the handle
 * marked: read, result_device and stats return that status again until the next match_device.  The index is intact unless it was the
 * build that failed; then match_device is NTK_ERR_BAD_ARG until the next build.  Every refusal comes before any device call, except the
 * verification of the list on the device, which comes before anything held is touched.
 *
 * Memory on the device (ntk_seed_index_stats reports the sum).  The index, freed by destroy and replaced by a build: 12 B per key and 4
 * more (the keys and the starts of their ranges) and 8 B per occurrence, of the index held.  The match result: 12 B per anchor and
 * 8 + 16 B per read and 8 more (a_offsets and the rows).  Work arrays, freed by trim: the build's, 28 B per entry (sorted values, entry
 * indices before and after the sort, owners, heads and their scan); the match's, 16 B per seed and 12 more (key index, anchor count and
 * base) and 16 B per read (the long reads' segments); 24 B per anchor of the reads that have more than 2048 (their keys and their qpos,
 * twice each), nothing where no read has; the spectrum's bins, 8 B each; 4 counter words.  The anchor arrays grow by half again and 64
 * to the largest batch so far; every other array but the index's grows to exactly the largest size needed so far.  The sort's scratch,
 * rocPRIM's temporary storage, which rocPRIM sizes (about 12 B per entry or long-read anchor sorted), is held INSIDE a build_device or
 * match_device only and freed before the call returns: it is part of the call's peak and of nothing stats reports.
 */
#ifndef NEEDLETAIL_AMD_SEED_INDEX_H
#define NEEDLETAIL_AMD_SEED_INDEX_H

#include "needletail_amd.h"

#ifdef __cplusplus
extern "C" {
#endif

typedef struct ntk_seed_index ntk_seed_index;

/* (a struct tag, not a typedef: ntk_seed_index_stats is also the function that fills it) */
struct ntk_seed_index_stats {
    uint64_t n_refs;            /* records of the list the index was built from                                              */
    uint64_t n_entries;         /* occurrences the index holds                                                               */
    uint64_t n_keys;            /* distinct values                                                                           */
    uint64_t max_occ;           /* the largest occ in the index                                                              */
    uint64_t n_reads;           /* of the held match                                                                         */
    uint64_t n_seeds;           /* entries of its reads                                                                      */
    uint64_t n_anchors;         /* anchors of the match (after NTK_ERR_CAPACITY: the number needed)                          */
    uint64_t device_bytes;      /* device memory the handle holds now                                                        */
};

/* The handle holds no index and no result and works on ctx's device and stream. */
int ntk_seed_index_create(ntk_ctx *ctx, ntk_seed_index **out);
void ntk_seed_index_destroy(ntk_seed_index *s);
/* Builds the index from the list of a reference batch (synchronous); it replaces the one held and drops a held match result.  The
 * list is verified as the head comment says.  d_offsets NULL or not 8-byte aligned; with n_entries != 0, d_pos or d_values NULL or not
 * 8-byte aligned or d_info NULL or not 4-byte aligned: NTK_ERR_BAD_ARG.  n_refs == 0 or n_entries == 0 is NTK_OK and holds an empty
 * index. */
int ntk_seed_index_build_device(ntk_seed_index *s, const uint64_t *d_offsets, const uint64_t *d_pos, const uint64_t *d_values,
                                const uint32_t *d_info, uint64_t n_refs, uint64_t n_entries);
/* The occ spectrum of the index in n_bins >= 2 host words (synchronous).  Before any build or n_bins < 2: NTK_ERR_BAD_ARG. */
int ntk_seed_index_spectrum(ntk_seed_index *s, uint64_t *hist, uint32_t n_bins);
/* Matches the list of a read batch against the index (synchronous); the result replaces the one held.  The pointers as for
 * build_device; the list is verified the same way.  Before any build: NTK_ERR_BAD_ARG.  max_occ == 0: no seed is repetitive;
 * max_anchors == 0: no limit below 2^32.  An empty index, an empty read list and reads without seeds are NTK_OK with empty ranges. */
int ntk_seed_index_match_device(ntk_seed_index *s, const uint64_t *d_offsets, const uint64_t *d_pos, const uint64_t *d_values,
                                const uint32_t *d_info, uint64_t n_reads, uint64_t n_entries, uint32_t max_occ, uint64_t max_anchors);
/* The held result as a CSR in host arrays (synchronous): read q's anchors are ref_rev, rpos and qpos [a_offsets[q] .. a_offsets[q + 1]);
 * a_offsets has n_reads + 1 entries, rows 4 * n_reads; *n = the number of held anchors.  ref_rev, rpos and qpos hold `cap` anchors each:
 * cap too small is NTK_ERR_CAPACITY with *n = the size needed and NOTHING written (a_offsets and rows neither); NULL arrays with cap 0
 * ask for the size that way.  a_offsets == NULL: only *n is set; rows may be NULL.  Before any match: *n = 0 and nothing is written. */
int ntk_seed_index_read(ntk_seed_index *s, uint64_t *a_offsets, uint32_t *ref_rev, uint32_t *rpos, uint32_t *qpos, uint32_t *rows,
                        uint64_t cap, uint64_t *n);
/* The held result where it lies on the device; host-side only: queues nothing and waits for nothing.  The arrays are those of read, *n
 * the number of anchors; the pointers stay valid until the next build_device, match_device, trim or destroy.  Before any match: NULL
 * pointers, *n = 0. */
int ntk_seed_index_result_device(ntk_seed_index *s, const uint64_t **d_a_offsets, const uint32_t **d_ref_rev, const uint32_t **d_rpos,
                                 const uint32_t **d_qpos, const uint32_t **d_rows, uint64_t *n);
/* What the handle holds and what the last match did (synchronous). */
int ntk_seed_index_stats(ntk_seed_index *s, struct ntk_seed_index_stats *out);
/* Frees the match result and every work array (synchronous); THE INDEX STAYS.  read answers *n = 0 afterwards, as before any match. */
int ntk_seed_index_trim(ntk_seed_index *s);

#ifdef __cplusplus
}
#endif

#endif /* NEEDLETAIL_AMD_SEED_INDEX_H */
