/*
 * needletail_amd_abundance.h — per-read k-mer abundance against a count table (libneedletail_amd_abundance.so).
 *
 * The step after counting: go back over the reads and ask, per read, how abundant its k-mers are in a table of
 * needletail_amd_count.h - error / low-coverage filtering ("drop reads whose median 21-mer count is below 3"), abundance
 * normalisation (the median count of a read), contamination screening (count a reference into the table, report the share of each
 * read's k-mers it holds).  One row per record comes back on the device: the number of k-mers, how many the table holds, and the
 * minimum, median, maximum and sum of their counts.  The batch, the record offsets and the table never leave device memory.
 *
 * A consumer of the public ABIs: the k-mers are the values ntk_materialize_device_quality emits (every path, tie rule, alphabet and
 * quality mask is the core's), their counts are ntk_kmer_table_lookup_device's.  Every call returns a status code of
 * needletail_amd.h.  A handle is used by one thread at a time, like its context, and must be destroyed before its table and its
 * context.  k = 33..63 (the wide table of needletail_amd_wide_count.h) is not served here: a handle is made from a narrow table.
 *
 * Memory: scratch owned by the handle, grown on demand, kept between calls and released by ntk_read_abundance_trim /
 * ntk_read_abundance_destroy.  It is one chunk of the materialise face (10 B per base of at most 64 MiB of bases, plus a halo of
 * at most 32 bases) plus at most 8.25 B per base of the call's batch: the counts (8 B per base), the valid plane (1/8 B per base)
 * and the list of long records (8 B per 65 536 bases).
 */
#ifndef NEEDLETAIL_AMD_ABUNDANCE_H
#define NEEDLETAIL_AMD_ABUNDANCE_H

#include "needletail_amd_count.h"

#ifdef __cplusplus
extern "C" {
#endif

typedef struct ntk_read_abundance ntk_read_abundance;

/* One per record, 48 B.  With the record's n_kmers table counts sorted ascending as c[0 .. n_kmers): min = c[0],
 * median = c[n_kmers / 2] (integer division: the upper median), max = c[n_kmers - 1].  Exact 64-bit integers throughout.  A record
 * that emits no k-mer (empty, shorter than k, all N) has an all-zero row. */
struct ntk_read_abundance_row {
    uint64_t n_kmers;          /* k-mers the record emits: exactly the windows ntk_kmer_table_count_device would insert */
    uint64_t n_present;        /* of those: table count >= min_count                                                   */
    uint64_t min, median, max; /* over the n_kmers table counts, an absent k-mer counting 0                            */
    uint64_t sum;              /* of the n_kmers counts, mod 2^64                                                      */
};

/* Borrows `table`, which must have been created on `ctx` (the handle works on ctx's device and stream) and must outlive the
 * handle.  NULL pointers: NTK_ERR_BAD_ARG.  Reads the table's k and path (ntk_kmer_table_stats), so it synchronises. */
int ntk_read_abundance_create(ntk_ctx *ctx, ntk_kmer_table *table, ntk_read_abundance **out);
void ntk_read_abundance_destroy(ntk_read_abundance *a);
/* d_rows[r] = the row of record r, r = 0 .. n_records - 1 (device memory, 8-byte aligned).
 *
 * Input: the device batch layout, alignment and readable range of ntk_reduce_device, plus the packer's record offsets on the
 * device: d_offsets[0 .. n_records], d_offsets[0] = 0, d_offsets[n_records] = n_bytes, record r = the bytes
 * [d_offsets[r], d_offsets[r + 1]) whose last byte is the record's break byte (what ntk_batch_buffers returns, uploaded).  An empty
 * record is one break byte.  d_qual (may be NULL) and the cutoff in p->flags bits 15:8 mask bases as
 * ntk_kmer_table_count_device does.  An offset beyond n_bytes is read as n_bytes; no byte outside the batch is touched.
 *
 * Which k-mers: exactly the values ntk_materialize_device_quality marks valid for p.  A window never spans a break byte, so a
 * record's k-mers are those whose last byte lies inside the record.  p->k and p->path must be the table's and every p->flags bit
 * other than the cutoff 0 (no minimizer window, no NTK_FLAG_RESET): NTK_ERR_BAD_ARG otherwise.  Byte-path input that was not
 * normalised (NTK_PATH_BYTES_CANONICAL with pre NONE / STRIP_RETURNS) is NTK_ERR_UNSUPPORTED, as for the table.  A NULL d_seq,
 * d_offsets or d_rows with non-zero sizes, or a misaligned d_seq / d_qual, is NTK_ERR_BAD_ARG.
 *
 * min_count 0 counts as 1 (the rule of ntk_kmer_table_extract_device).  A table with n_dropped > 0 gives NTK_ERR_CAPACITY and
 * writes no row: an incomplete table never reads as a complete one.  n_records == 0 or n_bytes == 0 is NTK_OK and touches nothing.
 *
 * Synchronous: the call returns after the rows are written (the table's lookup synchronises the stream once per 64 MiB chunk
 * anyway).  A record may be longer than a chunk. */
int ntk_read_abundance_run_device(ntk_read_abundance *a, const uint8_t *d_seq, const uint8_t *d_qual, uint64_t n_bytes,
                                  const uint64_t *d_offsets, uint64_t n_records, const ntk_params *p, uint64_t min_count,
                                  struct ntk_read_abundance_row *d_rows);
/* Frees the scratch kept between calls (synchronises); the next call allocates again. */
int ntk_read_abundance_trim(ntk_read_abundance *a);

#ifdef __cplusplus
}
#endif

#endif /* NEEDLETAIL_AMD_ABUNDANCE_H */
