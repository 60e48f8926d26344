/*
 * needletail_amd_count.h — exact k-mer counting on the device (libneedletail_amd_count.so).
 *
 * Replaces the user's counting loop over `seq.canonical_kmers(k, &rc)` / `seq.bit_kmers(k, canonical)` (reference
 * src/lib.rs:22-31) with a count table in device memory: canonical (or forward) k-mers, k <= 32, keyed by the packed 2-bit
 * value the batch face emits.  Read-side calls return the sorted (k-mer, count) pairs, the abundance spectrum and point
 * lookups.
 *
 * The table is a consumer of the core library's public ABI: its keys are the values ntk_materialize_device_quality emits, so
 * each path's canonical form and tie rule are the core's.  Every call returns a status code of needletail_amd.h.  Count
 * calls are asynchronous on the context's stream; stats, extract, spectrum and lookup synchronise it.  A table is used by
 * one thread at a time, like its context, and must be destroyed before its context.
 *
 * Memory: 16 B per slot (a u64 key and a u64 count), plus the scratch of one chunk of input (64 MiB of bases at most:
 * 10 B per base) while counting.
 */
#ifndef NEEDLETAIL_AMD_COUNT_H
#define NEEDLETAIL_AMD_COUNT_H

#include "needletail_amd.h"

#ifdef __cplusplus
extern "C" {
#endif

typedef struct ntk_kmer_table ntk_kmer_table;

/* (a struct tag, not a typedef: the name is also the function that fills it) */
struct ntk_kmer_table_stats {
    uint64_t n_distinct, n_total; /* distinct keys held; sum of their counts                                              */
    uint64_t n_dropped;           /* occurrences not inserted (probe limit reached): > 0 => the table is incomplete       */
    uint64_t slots;               /* hash slots (a power of two)                                                          */
    uint32_t k, path;
};

/* k = 1..32 (NTK_ERR_BAD_K otherwise); path = any NTK_PATH_*.  The key is the value the path emits: canonical on the canonical
 * paths (each with its own tie rule, which decides the flag only, never the value), forward on NTK_PATH_BITS.  `capacity` is the
 * number of distinct k-mers the table must hold; it gets the smallest power-of-two number of slots at which that is <= 75 % load.
 * The table works on ctx's device and stream. */
int ntk_kmer_table_create(ntk_ctx *ctx, uint32_t k, uint32_t path, uint64_t capacity, ntk_kmer_table **out);
void ntk_kmer_table_destroy(ntk_kmer_table *t);
/* Empties the table (async). */
int ntk_kmer_table_reset(ntk_kmer_table *t);
/* Counts every k-mer the batch emits (async).  Input: the device batch layout, alignment and readable range of ntk_reduce_device.
 * d_qual (may be NULL) and the cutoff in p->flags bits 15:8 mask bases as ntk_reduce_device_quality does.  p->k and p->path must
 * be the table's and every other p->flags bit 0 (minimizer windows are not counted; NTK_FLAG_RESET is ntk_kmer_table_reset's job):
 * NTK_ERR_BAD_ARG otherwise.  Byte-path input that was not normalised (NTK_PATH_BYTES_CANONICAL with pre NONE / STRIP_RETURNS) is
 * NTK_ERR_UNSUPPORTED, as in materialise mode.  Counts accumulate over calls until ntk_kmer_table_reset. */
int ntk_kmer_table_count_device(ntk_kmer_table *t, const uint8_t *d_seq, const uint8_t *d_qual, uint64_t n_bytes,
                                const ntk_params *p);
/* Synchronises.  Valid whether or not the table is complete. */
int ntk_kmer_table_stats(ntk_kmer_table *t, struct ntk_kmer_table_stats *out);
/* The pairs with count >= min_count (0 counts as 1), keys ascending, into device arrays of `cap` entries; *n = the number of pairs.
 * cap too small: NTK_ERR_CAPACITY with *n = the number needed (d_keys / d_counts may be NULL with cap 0 to ask for it).
 * Extract, spectrum and lookup return NTK_ERR_CAPACITY when n_dropped > 0 (extract with *n = 0): an incomplete table never reads as
 * a complete one. */
int ntk_kmer_table_extract_device(ntk_kmer_table *t, uint64_t min_count, uint64_t *d_keys, uint64_t *d_counts, uint64_t cap,
                                  uint64_t *n);
/* Host array hist[n_bins], n_bins = 2..16384: hist[c] = distinct keys with count c for 1 <= c < n_bins - 1, hist[n_bins - 1] =
 * those with count >= n_bins - 1, hist[0] = 0. */
int ntk_kmer_table_spectrum(ntk_kmer_table *t, uint64_t *hist, uint32_t n_bins);
/* d_counts[i] = count of d_queries[i] (0 when absent); device arrays of n.  Queries are taken as given: canonicalising them for a
 * canonical table is the caller's job (ntk_bit_canonical). */
int ntk_kmer_table_lookup_device(ntk_kmer_table *t, const uint64_t *d_queries, uint64_t n, uint64_t *d_counts);

#ifdef __cplusplus
}
#endif

#endif /* NEEDLETAIL_AMD_COUNT_H */
