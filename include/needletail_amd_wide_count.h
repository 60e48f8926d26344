/*
 * needletail_amd_wide_count.h — exact counting of canonical k-mers with k = 33..63 on the device (libneedletail_amd_wide_count.so).
 *
 * The counterpart of needletail_amd_count.h for the k the narrow table cannot key: the user's counting loop over
 * `seq.normalize(..).canonical_kmers(k, &rc)` (reference src/lib.rs:22-31) at k = 33..63, with the 2k-bit canonical value kept in two
 * u64 words.  Only the byte path exists here: the reference's 2-bit iterator stops at k = 32.
 *
 * A key is two words {hi, lo}: hi = the first k - 32 bases, lo = the last 32 bases, both in the 2-bit code (A 0, C 1, G 2, T 3, first
 * base most significant), so the 2k-bit value is hi * 2^64 + lo.  Device arrays of keys hold 2 words per key, hi first.
 *
 * The keys are min(forward, reverse complement) of every window canonical_kmers(k, &rc) yields on normalised input: the tie rule
 * decides the reference's flag only, never the value, so a palindrome (even k) counts once per occurrence.  Every call returns a
 * status code of needletail_amd.h.  Count calls are asynchronous on the context's stream; stats, extract, spectrum and lookup
 * synchronise it.  A table is used by one thread at a time, like its context, and must be destroyed before its context.
 *
 * Memory: 24 B per slot (two key words and a u64 count).  Counting keeps no scratch.
 */
#ifndef NEEDLETAIL_AMD_WIDE_COUNT_H
#define NEEDLETAIL_AMD_WIDE_COUNT_H

#include "needletail_amd_count.h"

#ifdef __cplusplus
extern "C" {
#endif

typedef struct ntk_wide_table ntk_wide_table;

/* k = 33..63 (NTK_ERR_BAD_K otherwise); path = NTK_PATH_BYTES_CANONICAL (the bit paths stop at k = 32: NTK_ERR_BAD_K, as the core
 * answers k > 32 there).  `capacity` (1 .. 3 << 38, NTK_ERR_BAD_ARG otherwise) is the number of distinct k-mers the table must hold;
 * it gets the smallest power-of-two number of slots at which that is <= 75 % load.  The table works on ctx's device and stream. */
int ntk_wide_table_create(ntk_ctx *ctx, uint32_t k, uint32_t path, uint64_t capacity, ntk_wide_table **out);
void ntk_wide_table_destroy(ntk_wide_table *t);
/* Empties the table (async). */
int ntk_wide_table_reset(ntk_wide_table *t);
/* Counts every canonical k-mer of the batch (async).  Input: the device batch layout, alignment and readable range of
 * ntk_reduce_device: base bytes are ACGTacgtUu (U / u read as T), every other byte breaks the window, and only windows that end
 * before n_bytes count.  d_qual (may be NULL) and the cutoff in p->flags bits 15:8 turn a base whose quality byte is below the cutoff
 * into a break, as ntk_reduce_device_quality does.  p->k and p->path must be the table's and every other p->flags bit 0
 * (NTK_ERR_BAD_ARG otherwise).  pre = NTK_PRE_NORMALIZE or NTK_PRE_NORMALIZE_IUPAC (the same k-mer stream); input that was not
 * normalised (pre NONE / STRIP_RETURNS) is NTK_ERR_UNSUPPORTED, as in the narrow table.  Counts accumulate over calls until
 * ntk_wide_table_reset. */
int ntk_wide_table_count_device(ntk_wide_table *t, const uint8_t *d_seq, const uint8_t *d_qual, uint64_t n_bytes,
                                const ntk_params *p);
/* Synchronises.  Valid whether or not the table is complete. */
int ntk_wide_table_stats(ntk_wide_table *t, struct ntk_kmer_table_stats *out);
/* The pairs with count >= min_count (0 counts as 1), keys ascending as 2k-bit values, into device arrays: d_keys of 2 * cap words
 * ({hi, lo} rows), d_counts of cap; *n = the number of pairs.  cap too small: NTK_ERR_CAPACITY with *n = the number needed (d_keys /
 * d_counts may be NULL with cap 0 to ask for it).  Extract, spectrum and lookup return NTK_ERR_CAPACITY when n_dropped > 0 (extract
 * with *n = 0): an incomplete table never reads as a complete one. */
int ntk_wide_table_extract_device(ntk_wide_table *t, uint64_t min_count, uint64_t *d_keys, uint64_t *d_counts, uint64_t cap,
                                  uint64_t *n);
/* Host array hist[n_bins], n_bins = 2..16384: hist[c] = distinct keys with count c for 1 <= c < n_bins - 1, hist[n_bins - 1] =
 * those with count >= n_bins - 1, hist[0] = 0. */
int ntk_wide_table_spectrum(ntk_wide_table *t, uint64_t *hist, uint32_t n_bins);
/* d_counts[i] = count of the k-mer in d_queries[2i], d_queries[2i + 1] ({hi, lo}); device arrays.  Each query is canonicalised here,
 * so either strand reads the same count; a query with bits set above bit 2k reads 0. */
int ntk_wide_table_lookup_device(ntk_wide_table *t, const uint64_t *d_queries, uint64_t n, uint64_t *d_counts);

#ifdef __cplusplus
}
#endif

#endif /* NEEDLETAIL_AMD_WIDE_COUNT_H */
