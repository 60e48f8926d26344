/*
 * needletail_amd_kmer_sets.h — exact set algebra and joint spectra of two k-mer count lists on the GPU (libneedletail_amd_kmer_sets.so):
 * intersect / union / subtract / counters-subtract with a count rule, and the comparison of two lists (how many k-mers occur a times
 * in the one and b times in the other, with the exact totals that Jaccard, containment, Bray-Curtis, QV and completeness are read
 * from).  Both are one streaming merge-join of the two lists; no hash table is probed and the union is never materialised.
 *
 * A K-MER LIST is what ntk_kmer_table_extract_device (needletail_amd_count.h) and ntk_wide_table_extract_device
 * (needletail_amd_wide_count.h) write: `keys` of n * key_words uint64 words (key_words = 1 for k <= 32; 2 for k = 33..63, each key a
 * {hi, lo} row compared by hi, then lo) and `counts` of n uint64 values, keys strictly ascending, both arrays in device memory and
 * 8-byte aligned.  Every key value is legal, 0 and 2^64 - 1 included; nothing is padded with a sentinel.  The output of apply is a
 * k-mer list again, so the result of one operation is the input of the next.  This library never touches a table and does not care
 * which k or path made the keys; the caller keeps lists of one kind together.
 *
 * Every call returns a status code of needletail_amd.h and is synchronous on the context's stream (the result size must come back).
 * A handle is used by one thread at a time, like its context, and must be destroyed before its context.  Refused arguments change
 * nothing.  The calls trust their inputs to ascend: on input that does not, the result is unspecified, but no byte outside the given
 * arrays is read or written.  ntk_kmer_sets_validate_device is the cheap pass for callers who do not know.
 *
 * There is no floating point anywhere in the library.  All sums are modulo 2^64.
 *
 * Memory on the device: 24 B per tile of NTK_KSET_TILE_WORDS / key_words merged elements (three words of scratch per tile, grown on
 * demand and freed by release or destroy), the scan's temporary storage, and 128 KiB + 64 B for the bins and sums of compare.
 */
#ifndef NEEDLETAIL_AMD_KMER_SETS_H
#define NEEDLETAIL_AMD_KMER_SETS_H

#include "needletail_amd.h"

#ifdef __cplusplus
extern "C" {
#endif

#define NTK_KSET_TILE_WORDS 2048    /* key words one block joins at a time: 2048 merged elements of narrow keys, 1024 of wide ones */
#define NTK_KSET_MAX_BINS 16384     /* n_bins_a * n_bins_b of compare: the bin limit of the tables' spectrum call */

/* op of ntk_kmer_sets_apply_device: which keys are kept, and with which count (a, b: the key's counts in A and B)
 *   INTERSECT          in A and in B                              rule(a, b)
 *   UNION              in A or in B                               in both: rule(a, b); in one: that side's count
 *   SUBTRACT           in A, not in B                             a
 *   COUNTERS_SUBTRACT  in A with a > b, an absent b being 0      a - b                                            */
#define NTK_KSET_INTERSECT 1u
#define NTK_KSET_UNION 2u
#define NTK_KSET_SUBTRACT 3u
#define NTK_KSET_COUNTERS_SUBTRACT 4u

/* rule of INTERSECT and UNION; the two subtract ops ignore it and it must be 0 there.  SUM saturates at 2^64 - 1. */
#define NTK_KSET_MIN 1u
#define NTK_KSET_MAX 2u
#define NTK_KSET_SUM 3u
#define NTK_KSET_LEFT 4u
#define NTK_KSET_RIGHT 5u

typedef struct ntk_kmer_sets ntk_kmer_sets;

/* (struct tags, not typedefs: ntk_kmer_sets_stats is also the function that fills it) */
struct ntk_kmer_sets_stats {
    uint64_t key_words;      /* 1 or 2                                             */
    uint64_t device_bytes;   /* device memory held now                             */
    uint64_t n_launches;     /* kernel launches of this library since create       */
    uint64_t n_calls;        /* validate, compare and apply calls that ran a join or a pass, since create */
};

/* What compare adds up, exactly, each sum modulo 2^64.  "shared": keys in both lists; "only": keys in that list alone. */
struct ntk_kmer_sets_totals {
    uint64_t n_a, n_b, n_shared, n_a_only, n_b_only;
    uint64_t sum_a, sum_b;                 /* all counts of each list                                  */
    uint64_t sum_a_shared, sum_b_shared;   /* each side's counts over the shared keys                  */
    uint64_t sum_a_only, sum_b_only;
    uint64_t sum_min;                      /* min(a, b) over the shared keys                           */
    uint64_t sum_max;                      /* max(a, b) over the union, an absent side counting 0      */
};

/* key_words: 1 (k <= 32) or 2 (k = 33..63); anything else is NTK_ERR_BAD_ARG.  Works on ctx's device and stream; without a device:
 * NTK_ERR_NO_DEVICE. */
int ntk_kmer_sets_create(ntk_ctx *ctx, uint32_t key_words, ntk_kmer_sets **out);
void ntk_kmer_sets_destroy(ntk_kmer_sets *h);
/* Frees the scratch that grew with the lists (the next call allocates it again). */
int ntk_kmer_sets_release(ntk_kmer_sets *h);
int ntk_kmer_sets_stats(ntk_kmer_sets *h, struct ntk_kmer_sets_stats *out);
/* *n_violations = the number of adjacent pairs with keys[i] >= keys[i + 1]: 0 on a k-mer list.  d_keys may be NULL exactly when
 * n == 0. */
int ntk_kmer_sets_validate_device(ntk_kmer_sets *h, const uint64_t *d_keys, uint64_t n, uint64_t *n_violations);
/* The joint spectrum and the totals of two lists.  hist (host memory, n_bins_a * n_bins_b words, may be NULL):
 * hist[ba * n_bins_b + bb] = the number of distinct keys of the union with ba = min(count_a, n_bins_a - 1) and
 * bb = min(count_b, n_bins_b - 1), an absent key counting 0, so hist[0] is always 0.  n_bins_a and n_bins_b are each >= 2 and their
 * product is at most NTK_KSET_MAX_BINS: NTK_ERR_BAD_ARG otherwise (also with hist == NULL).  totals may be NULL.  n_a == 0 and / or
 * n_b == 0 are ordinary inputs, and a list's arrays may be NULL exactly when its n is 0. */
int ntk_kmer_sets_compare_device(ntk_kmer_sets *h, const uint64_t *d_a_keys, const uint64_t *d_a_counts, uint64_t n_a,
                                 const uint64_t *d_b_keys, const uint64_t *d_b_counts, uint64_t n_b,
                                 uint32_t n_bins_a, uint32_t n_bins_b, uint64_t *hist, struct ntk_kmer_sets_totals *totals);
/* op(A, B) with `rule` into the caller's device arrays of `cap` entries (d_out_keys: cap * key_words words); *n = the number of
 * entries of the result, a k-mer list.  cap too small: NTK_ERR_CAPACITY with *n = the number needed and nothing written (the output
 * arrays may be NULL with cap 0 to ask for it).  An unknown op or rule, a rule other than 0 with a subtract op, a NULL list with
 * n > 0, and an output range that overlaps an input range or the other output range (a host check of the pointers) are
 * NTK_ERR_BAD_ARG. */
int ntk_kmer_sets_apply_device(ntk_kmer_sets *h, uint32_t op, uint32_t rule,
                               const uint64_t *d_a_keys, const uint64_t *d_a_counts, uint64_t n_a,
                               const uint64_t *d_b_keys, const uint64_t *d_b_counts, uint64_t n_b,
                               uint64_t *d_out_keys, uint64_t *d_out_counts, uint64_t cap, uint64_t *n);

#ifdef __cplusplus
}
#endif

#endif /* NEEDLETAIL_AMD_KMER_SETS_H */
