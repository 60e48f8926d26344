/*
 * needletail_amd_minhash.h — MinHash sketches of device batches, to compare samples (libneedletail_amd_minhash.so): bottom-s sketches
 * (mash, finch), scaled sketches (FracMinHash, sourmash), both with abundance, their merge, and their comparison.
 *
 * Which k-mers: exactly the keys the count table of the same k and path would insert for the same call, as the cardinality sketch of
 * needletail_amd_sketch.h - k = 1..32 on every NTK_PATH_* (the value ntk_materialize_device_quality emits), k = 33..63 on
 * NTK_PATH_BYTES_CANONICAL (the two-word key {hi, lo} of needletail_amd_wide_count.h).
 *
 * The hash (fixed here, restated by the tests' host model) is that sketch's: one 64-bit hash h per key from the tables' hash fmix64
 * (the murmur3 finaliser), h = fmix64(key ^ C) for a one-word key, h = fmix64(lo ^ fmix64(hi) ^ C) for {hi, lo}, C =
 * NTK_MINHASH_XOR (the value of NTK_SKETCH_XOR).  It is this project's own hash: sketches made here compare with each other, not with
 * sourmash, mash or finch files.
 *
 * Two kinds of sketch, chosen at create (exactly one of `num` and `scaled` is non-zero):
 *   num = s    the s smallest distinct hashes seen since reset (all of them while there are fewer);
 *   scaled     every distinct hash h <= max_hash = (2^64 - 1) / scaled (integer division; scaled = 1 keeps everything).
 * Every kept hash carries a count: the number of k-mers (windows) added since reset that hashed to it, EXACTLY, whatever the split of
 * the input into calls, chunks and kernel launches.  A sketch is a function of the multiset of keys.
 *
 * How: a filter kernel hashes every key and appends the hashes at or below the threshold (see ntk_minhash_stats) to a candidate
 * buffer of `buffer_entries` hashes; when the buffer is needed, and before stats, read and merge answer, it is sorted, run-length
 * encoded and folded into the kept set, which may lower the threshold.  A launch whose appends do not fit the room left in the buffer
 * is discarded as a whole and redone in pieces that fit (n_redone counts them), so no count ever misses an occurrence.  The threshold
 * only falls, hence a hash at or below the final threshold passed every earlier filter.
 *
 * Every call returns a status code of needletail_amd.h.  reset is asynchronous on the context's stream; add_device MAY SYNCHRONISE it
 * (it reads the buffer's fill after every launch, as ntk_read_abundance_run_device reads its counters); stats, read and merge synchronise
 * it.  A handle is used by one thread at a time, like its context, and must be destroyed before its context.
 *
 * A call that fails halfway through its work on the device (NTK_ERR_NOMEM, NTK_ERR_HIP, a failure of the materialise pass) leaves the
 * handle marked: the counts could no longer be exact, so every later call but reset and destroy returns that status again, and reset
 * starts over.  Refused arguments (NTK_ERR_BAD_ARG, NTK_ERR_BAD_K, NTK_ERR_UNSUPPORTED) and NTK_ERR_CAPACITY from read change nothing.
 *
 * Known costs.  One hash at or below the threshold that occurs N times is appended N times (the count table's hot-key case,
 * DESIGN.md sections 10 and 15).  A bottom-s sketch that holds
 * fewer than num hashes has no threshold yet: everything passes, so every launch covers at most buffer_entries window ends and is
 * followed by a merge.  On data with fewer than num distinct k-mers (a low-complexity sample, or num near 2^20) that never ends - a
 * 1.5 G-base batch is about 360 launch-and-merge rounds at the default buffer; the result is exact all the same.
 *
 * Memory on the device, freed by destroy: the candidate buffer, 8 * buffer_entries bytes, and as much again for its sorted copy; the
 * temporary storage of the sort, the run-length encoding, the merge and the reduction (a few MiB at the default buffer); four arrays
 * of (hash, count) pairs, 16 B per entry, each grown by half on demand - the kept set (at most num entries, or as many as the data
 * has at or below max_hash), the runs of the sorted buffer or a foreign sketch (at most buffer_entries, or that sketch's length), and
 * the merged list and the next kept set of a merge (kept + runs each) - an allocation failure is NTK_ERR_NOMEM; for k <= 32 the
 * materialise scratch of one chunk of input (64 MiB of bases at most: 10 B per base); k = 33..63 keeps no scratch.
 */
#ifndef NEEDLETAIL_AMD_MINHASH_H
#define NEEDLETAIL_AMD_MINHASH_H

#include "needletail_amd.h"

#ifdef __cplusplus
extern "C" {
#endif

#define NTK_MINHASH_XOR 0x9E3779B97F4A7C15ull         /* C: xored into the key's hash input (= NTK_SKETCH_XOR) */
#define NTK_MINHASH_MAX_NUM (1ull << 20)              /* the largest bottom-s sketch                           */
#define NTK_MINHASH_BUFFER_DEFAULT (1ull << 22)       /* buffer_entries = 0 means this                         */
#define NTK_MINHASH_BUFFER_MIN 64ull                  /* one lane run of the k = 33..63 kernel                 */
#define NTK_MINHASH_BUFFER_MAX (1ull << 28)

typedef struct ntk_minhash ntk_minhash;

/* (struct tags, not typedefs: ntk_minhash_stats is also the function that fills it) */
struct ntk_minhash_stats {
    uint64_t n_windows;      /* EXACT number of k-mers added since reset (every call, every chunk, merges included)            */
    uint64_t n_kept;         /* hashes held                                                                                    */
    uint64_t threshold;      /* the largest hash that can still enter: max_hash with `scaled`; with `num` the num-th kept hash */
                             /* once num hashes are held, ~0 before that                                                       */
    uint64_t num, scaled;
    uint64_t buffer_entries; /* the candidate buffer's size in hashes (the default resolved)                                   */
    uint64_t n_merges;       /* times a non-empty buffer or a foreign sketch was folded into the kept set                      */
    uint64_t n_redone;       /* launches whose appends did not fit and were discarded and redone                               */
    uint32_t k, path;
};

struct ntk_minhash_comparison {
    uint64_t n_a, n_b;       /* entries of each side at or below max_hash                                 */
    uint64_t n_shared;       /* see ntk_minhash_compare                                                   */
    uint64_t n_union;
    double dot;              /* sum of ca * cb over the shared hashes                                     */
    double norm2_a, norm2_b; /* sum of ca^2 (cb^2) over the side's hashes that are counted into the union */
};

/* k = 1..32 on any NTK_PATH_*, k = 33..63 on NTK_PATH_BYTES_CANONICAL.  k = 0, k >= 64 and k > 32 on a bit path: NTK_ERR_BAD_K; no
 * such path: NTK_ERR_BAD_ARG.  Exactly one of num (at most NTK_MINHASH_MAX_NUM) and scaled is non-zero, and buffer_entries is 0 (the
 * default) or within NTK_MINHASH_BUFFER_MIN..NTK_MINHASH_BUFFER_MAX: NTK_ERR_BAD_ARG otherwise.  buffer_entries is a memory knob
 * (8 B per entry, twice): a smaller buffer means more merges, and more redone launches where many hashes pass.  The handle starts
 * empty and works on ctx's device and stream. */
int ntk_minhash_create(ntk_ctx *ctx, uint32_t k, uint32_t path, uint64_t num, uint64_t scaled, uint64_t buffer_entries,
                       ntk_minhash **out);
void ntk_minhash_destroy(ntk_minhash *m);
/* Empties the sketch: nothing kept, n_windows, n_merges and n_redone 0, the threshold as at create (async). */
int ntk_minhash_reset(ntk_minhash *m);
/* Adds every k-mer the batch emits (may synchronise the stream): the keys the table of this k and path would count in
 * ntk_kmer_table_count_device / ntk_wide_table_count_device, under the same rules.  Input: the device batch layout, alignment and
 * readable range of ntk_reduce_device.  d_qual (may be NULL) and the cutoff in p->flags bits 15:8 mask bases as
 * ntk_reduce_device_quality does.  p->k and p->path must be the handle's and every other p->flags bit 0: NTK_ERR_BAD_ARG otherwise.
 * Byte-path input that was not normalised (NTK_PATH_BYTES_CANONICAL with pre NONE / STRIP_RETURNS) is NTK_ERR_UNSUPPORTED.
 * n_bytes == 0 is NTK_OK.  Calls accumulate until ntk_minhash_reset. */
int ntk_minhash_add_device(ntk_minhash *m, const uint8_t *d_seq, const uint8_t *d_qual, uint64_t n_bytes, const ntk_params *p);
/* What the handle holds (synchronises). */
int ntk_minhash_stats(ntk_minhash *m, struct ntk_minhash_stats *out);
/* The kept hashes, strictly ascending, and their counts, into host arrays of `cap` entries each (synchronises); *n = their number.
 * cap too small: NTK_ERR_CAPACITY with *n = the size needed and nothing written; NULL arrays with cap 0 ask for the size that way. */
int ntk_minhash_read(ntk_minhash *m, uint64_t *hashes, uint64_t *counts, uint64_t cap, uint64_t *n);
/* Folds in a sketch made elsewhere (another handle, GPU or process) of the same k, path and hash, from host arrays (synchronises):
 * counts of equal hashes add, n_windows is added, and the result is cut by this handle's own rule.  hashes must be strictly ascending
 * (NTK_ERR_BAD_ARG otherwise); counts == NULL means every count is 1; n == 0 adds n_windows alone.  The counts stay exact when the
 * other sketch keeps at least what this one would: the same num or a larger one, the same scaled or a divisor of it. */
int ntk_minhash_merge(ntk_minhash *m, const uint64_t *hashes, const uint64_t *counts, uint64_t n, uint64_t n_windows);
/* Compares two sketches in host memory; plain host code, no device and no context.  Both arrays must be strictly ascending
 * (NTK_ERR_BAD_ARG otherwise, as is a NULL `out` or a NULL array with a non-zero length); ca / cb == NULL mean every count is 1.
 * Entries above max_hash are ignored on both sides: two scaled sketches of different `scaled` compare at the smaller max_hash.
 *   num == 0:  n_shared = |A n B|, n_union = |A u B|.
 *   num == s:  (mash's rule) U = the s smallest members of A u B, or all of them if there are fewer; n_union = |U|, n_shared = the
 *              number of members of U that are in both A and B.
 * dot adds ca * cb over the hashes counted in n_shared, norm2_a (norm2_b) adds ca^2 (cb^2) over the members of A (B) counted in
 * n_union, each in ascending hash order, in double.  Ratios are the caller's: Jaccard = n_shared / n_union, containment of A in B =
 * n_shared / n_a, cosine = dot / sqrt(norm2_a * norm2_b), Mash distance = -ln(2 j / (1 + j)) / k. */
int ntk_minhash_compare(const uint64_t *a, const uint64_t *ca, uint64_t na, const uint64_t *b, const uint64_t *cb, uint64_t nb,
                        uint64_t num, uint64_t max_hash, struct ntk_minhash_comparison *out);

#ifdef __cplusplus
}
#endif

#endif /* NEEDLETAIL_AMD_MINHASH_H */
