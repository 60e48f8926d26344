/*
 * needletail_amd_minhash_set.h — a set of MinHash sketches resident on the device, and the comparison of a block of its rows with a
 * block of columns, pair by pair, in one pass on the GPU (libneedletail_amd_minhash_set.so): N samples against N samples, or one query
 * against a database of N.
 *
 * A sketch here is what ntk_minhash_read (needletail_amd_minhash.h) returns: strictly ascending 64-bit hashes, each with a count.  This
 * library never hashes a k-mer; it compares hashes somebody else made, and it does not care which k, path or hash made them - the
 * caller keeps sketches of one kind in one set.
 *
 * Every pair's result is exactly what ntk_minhash_compare gives for it: the same n_shared, n_union, n_a and n_b, and dot, norm2_a and
 * norm2_b as sums of the same terms (each product rounded as there) in another order - equal bit for bit while every partial sum is an
 * integer below 2^53, and within a few n * 2^-53 of each other relatively otherwise.
 *
 * Every call returns a status code of needletail_amd.h.  add is host work: the sketch goes to a staging area on the host, and the next
 * compare or read uploads whatever is new with one copy per array (n_uploads counts these uploads, not the adds).  compare and read
 * synchronise the context's stream.  A handle is used by one thread at a time, like its context, and must be destroyed before its
 * context.  Refused arguments change nothing; compare never modifies a set, so a failed compare leaves both sets usable.
 *
 * Memory on the device, freed by destroy: 8 B per entry for the hashes, 8 B more per entry with `abundance`, 8 B per sketch for the
 * offsets and 8 B per sketch for the cut lengths (the arrays grow by doubling, so up to twice that), and block_pairs * 32 B of result
 * scratch (allocated by the first compare, and never for more pairs than a compare asked for).  The host holds the offsets (8 B per
 * sketch), what was added since the last upload, and a pinned mirror of the result scratch.
 */
#ifndef NEEDLETAIL_AMD_MINHASH_SET_H
#define NEEDLETAIL_AMD_MINHASH_SET_H

#include "needletail_amd.h"

#ifdef __cplusplus
extern "C" {
#endif

#define NTK_MHSET_BLOCK_DEFAULT (1ull << 20)   /* block_pairs = 0 means this: 32 MiB of result scratch */
#define NTK_MHSET_BLOCK_MIN 1ull
#define NTK_MHSET_BLOCK_MAX (1ull << 26)
#define NTK_MHSET_STAGE 2048                    /* a column sketch of at most this many hashes is searched in LDS */

typedef struct ntk_mhset ntk_mhset;

/* (a struct tag, not a typedef: ntk_mhset_stats is also the function that fills it) */
struct ntk_mhset_stats {
    uint64_t n_sketches;
    uint64_t n_entries;      /* hashes of all sketches together                                                */
    uint64_t abundance;      /* 1: counts are stored                                                           */
    uint64_t block_pairs;    /* pairs per launch (the default resolved)                                        */
    uint64_t device_bytes;   /* device memory held now                                                         */
    uint64_t n_launches;     /* launches of the pair kernel by compares with this handle as `rows`, since create */
    uint64_t n_uploads;      /* times staged sketches were copied to the device, since create                  */
};

/* abundance = 0: the set stores no counts and every count is 1 (as a NULL `ca` is for ntk_minhash_compare); 1: counts are stored; any
 * other value is NTK_ERR_BAD_ARG.  block_pairs: the number of pairs one launch covers and the size of the result scratch, a memory knob
 * (32 B per pair); 0 is NTK_MHSET_BLOCK_DEFAULT, anything else outside NTK_MHSET_BLOCK_MIN..NTK_MHSET_BLOCK_MAX is NTK_ERR_BAD_ARG.
 * The set starts empty and works on ctx's device and stream; without a device: NTK_ERR_NO_DEVICE. */
int ntk_mhset_create(ntk_ctx *ctx, uint32_t abundance, uint64_t block_pairs, ntk_mhset **out);
void ntk_mhset_destroy(ntk_mhset *s);
/* Empties the set (the device arrays are kept for the next sketches; the counters of stats go on counting). */
int ntk_mhset_reset(ntk_mhset *s);
/* Appends one sketch of n hashes, strictly ascending (NTK_ERR_BAD_ARG otherwise, the check of ntk_minhash_compare), and returns its
 * index in *index (may be NULL).  n == 0 is a valid, empty sketch; n >= 2^32 is NTK_ERR_BAD_ARG (the pair counts are 32-bit), checked
 * before the arrays are looked at.  counts == NULL means every count is 1; counts on a set without abundance: NTK_ERR_BAD_ARG.  Host
 * work only; a refused or failed add leaves the set as it was. */
int ntk_mhset_add(ntk_mhset *s, const uint64_t *hashes, const uint64_t *counts, uint64_t n, uint64_t *index);
/* Sketch `index` as it was added, from the device copy (synchronises), into host arrays of `cap` entries each; *n = its length.  cap too
 * small: NTK_ERR_CAPACITY with *n = the size needed and nothing written; NULL arrays with cap 0 ask for the size that way.  `counts` may
 * be NULL; without abundance it is filled with 1. */
int ntk_mhset_read(ntk_mhset *s, uint64_t index, uint64_t *hashes, uint64_t *counts, uint64_t cap, uint64_t *n);
int ntk_mhset_stats(ntk_mhset *s, struct ntk_mhset_stats *out);
/* Compares every r in [row0, row0 + n_rows) of `rows` with every c in [col0, col0 + n_cols) of `cols` (synchronises).  Entry
 * (r - row0) * n_cols + (c - col0) of each output matrix is the field of that name in the ntk_minhash_comparison that
 * ntk_minhash_compare(rows[r], cols[c], num, max_hash) fills; n_a[r - row0] and n_b[c - col0] are the sketches' entries at or below
 * max_hash.  All outputs are host arrays and any of them may be NULL; the second pass that norm2_b needs runs only when it is asked
 * for, and no pair is compared when no matrix is.  `rows` and `cols` may be the same handle; handles of two contexts, and a range past
 * the end of its set, are NTK_ERR_BAD_ARG.  n_rows * n_cols == 0 is NTK_OK with nothing written.  A block of more than block_pairs
 * (of `rows`) pairs is walked in sub-blocks inside the call, each one launch (two with norm2_b) and one copy back. */
int ntk_mhset_compare(ntk_mhset *rows, uint64_t row0, uint64_t n_rows, ntk_mhset *cols, uint64_t col0, uint64_t n_cols,
                      uint64_t num, uint64_t max_hash,
                      uint32_t *n_shared, uint32_t *n_union, double *dot, double *norm2_a, double *norm2_b,
                      uint64_t *n_a, uint64_t *n_b);

#ifdef __cplusplus
}
#endif

#endif /* NEEDLETAIL_AMD_MINHASH_SET_H */
