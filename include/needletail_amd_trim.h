/*
 * needletail_amd_trim.h — trim reads by k-mer abundance and write the kept reads out as a batch (libneedletail_amd_trim.so).
 *
 * The step after counting and per-read abundance: cut each read at its first low-abundance k-mer (khmer's filter-abund /
 * trim-low-abund), or keep its longest run of solid k-mers (the solid-region step of k-mer error correctors), drop what is too short,
 * and hand the surviving reads to the next stage as a device batch that ntk_kmer_table_count_device, ntk_read_abundance_run_device
 * and the calls below take as it is.  The batch, the record offsets, the table and the output never leave device memory.
 *
 * A consumer of the public ABIs: the k-mers are the values ntk_materialize_device_quality emits, their counts are
 * ntk_kmer_table_lookup_device's.  Every call returns a status code of needletail_amd.h.  A handle is used by one thread at a time,
 * like its context, and must be destroyed before its table and its context.  k = 33..63 (the wide table of
 * needletail_amd_wide_count.h) is not served here: a handle is made from a narrow table.
 *
 * Memory: scratch owned by the handle, grown on demand, kept between calls and released by ntk_read_trim_release /
 * ntk_read_trim_destroy.  It is one chunk of the materialise face (10 B per base of at most 64 MiB of bases, plus a halo of at most
 * 32 bases), the table counts of ONE chunk (8 B per base of at most 64 MiB of bases: there is no batch-long count array), and two bit
 * planes of the call's batch, the solid plane and the valid plane (1/8 B per base each, plus 16 B).  ntk_read_trim_compact_device
 * adds 16 B per record plus 16 B for its scan, the scan's own temporary storage (a few KiB per million records), and 8 B per
 * 16 384 bases for a list of long records.
 */
#ifndef NEEDLETAIL_AMD_TRIM_H
#define NEEDLETAIL_AMD_TRIM_H

#include "needletail_amd_count.h"

#ifdef __cplusplus
extern "C" {
#endif

typedef struct ntk_read_trim ntk_read_trim;

/* How the kept interval of a record is chosen (below). */
enum {
    NTK_TRIM_PREFIX = 0,  /* cut the read at its first weak window (khmer's rule) */
    NTK_TRIM_LONGEST = 1  /* keep the longest run of solid windows                */
};

/* One per record, 32 B.  Exact integers.
 *
 * Record r has L bytes before its break byte.  The window ending at record position j (k - 1 <= j < L) is SOLID when
 * ntk_materialize_device_quality marks it valid for p AND its table count is >= min_count; otherwise it is WEAK (a window over an
 * N, a masked quality or a non-base byte is weak).
 *   NTK_TRIM_PREFIX:  j* = the first weak window end, or L when there is none.  Kept = [0, j*) when j* > k - 1, otherwise nothing.
 *   NTK_TRIM_LONGEST: the longest maximal run of solid windows, ending at j0 .. j1 (the leftmost run wins a tie).
 *                     Kept = [j0 - k + 1, j1 + 1).  No solid window: nothing.
 * min_length 0 counts as k; a kept interval shorter than min_length becomes empty.  A kept interval therefore holds at least one
 * window, and all its windows are solid: trimming the output batch again with the same table and min_count keeps every record
 * whole. */
struct ntk_read_trim_row {
    uint64_t start;   /* first kept byte, relative to the record's first byte; 0 when nothing is kept                         */
    uint64_t length;  /* kept bytes; 0 when nothing is kept                                                                  */
    uint64_t n_kmers; /* windows the record emits: ntk_read_abundance_row.n_kmers                                            */
    uint64_t n_solid; /* of those: table count >= min_count: ntk_read_abundance_row.n_present.  Both before min_length empties */
};

/* Borrows `table`, which must have been created on `ctx` (the handle works on ctx's device and stream) and must outlive the
 * handle.  NULL pointers: NTK_ERR_BAD_ARG.  Reads the table's k and path (ntk_kmer_table_stats), so it synchronises. */
int ntk_read_trim_create(ntk_ctx *ctx, ntk_kmer_table *table, ntk_read_trim **out);
void ntk_read_trim_destroy(ntk_read_trim *t);
/* Frees the scratch kept between calls (synchronises); the next call allocates again. */
int ntk_read_trim_release(ntk_read_trim *t);
/* d_rows[r] = the row of record r, r = 0 .. n_records - 1 (device memory, 8-byte aligned).
 *
 * Input, p, d_qual and the cutoff, alignment, the clamping of offsets to n_bytes and every error rule are
 * ntk_read_abundance_run_device's: the device batch layout, alignment and readable range of ntk_reduce_device, plus the packer's
 * record offsets on the device: d_offsets[0 .. n_records], record r = the bytes [d_offsets[r], d_offsets[r + 1]) whose last byte is
 * the record's break byte.  d_qual (may be NULL) and the cutoff in p->flags bits 15:8 mask bases as ntk_kmer_table_count_device
 * does.  An offset beyond n_bytes is read as n_bytes; no byte outside the batch is touched.  p->k and p->path must be the table's and
 * every p->flags bit other than the cutoff 0: NTK_ERR_BAD_ARG otherwise.  Byte-path input that was not normalised
 * (NTK_PATH_BYTES_CANONICAL with pre NONE / STRIP_RETURNS) is NTK_ERR_UNSUPPORTED.  A NULL d_seq, d_offsets or d_rows with non-zero
 * sizes, or a misaligned d_seq / d_qual / d_offsets / d_rows, is NTK_ERR_BAD_ARG.  mode is NTK_TRIM_PREFIX or NTK_TRIM_LONGEST;
 * any other value is NTK_ERR_BAD_ARG.
 *
 * min_count 0 counts as 1.  A table with n_dropped > 0 gives NTK_ERR_CAPACITY and writes no row.  n_records == 0 or n_bytes == 0 is
 * NTK_OK and touches nothing.
 *
 * Synchronous: the call returns after the rows are written (the table's lookup synchronises the stream once per 64 MiB chunk
 * anyway).  A record may be longer than a chunk. */
int ntk_read_trim_run_device(ntk_read_trim *t, const uint8_t *d_seq, const uint8_t *d_qual, uint64_t n_bytes,
                             const uint64_t *d_offsets, uint64_t n_records, const ntk_params *p, uint64_t min_count, uint32_t mode,
                             uint64_t min_length, struct ntk_read_trim_row *d_rows);
/* Writes the records with length > 0 out as a batch, in input order: output record i is the kept bytes of its input record plus
 * one '\n' break byte.  d_out_offsets[0 .. n_out] are its offsets (d_out_offsets[n_out] = *out_n_bytes), d_out_source[i] the input
 * index of output record i, and d_out_seq is padded with '\n' up to round_up(*out_n_bytes, 16): the output goes straight back into
 * ntk_kmer_table_count_device, ntk_read_abundance_run_device, ntk_read_trim_run_device and this call.
 *
 * d_aux / d_out_aux: both NULL, or a parallel stream of d_seq's layout (the quality bytes) and its output; it is cut with the same
 * intervals, the byte under an output break byte is the byte under the source record's break byte, and it is padded as d_out_seq.
 *
 * Capacity: out_cap_bytes >= round_up(*out_n_bytes, 16) and out_cap_records >= *out_n_records are needed (d_out_offsets holds
 * out_cap_records + 1 words, d_out_source out_cap_records); round_up(n_bytes, 16) bytes and n_records records always suffice.
 * Too small: NTK_ERR_CAPACITY with the output's bytes and records in *out_n_bytes / *out_n_records and nothing written;
 * d_out_seq / d_out_aux / d_out_offsets / d_out_source may be NULL with both capacities 0 to ask for the sizes.  An output of no
 * record is NTK_OK with 0 and 0.
 *
 * d_rows need not come from ntk_read_trim_run_device: any rows with start + length <= L are legal; a row beyond that is clamped
 * on the device (start to L, then length to L - start) and no byte outside the batch is read.  d_seq and d_aux as above (16-byte
 * aligned, readable up to round_up(n_bytes, 16)); d_out_seq / d_out_aux 16-byte aligned; d_offsets, d_rows, d_out_offsets and
 * d_out_source 8-byte aligned: NTK_ERR_BAD_ARG otherwise, as for NULL d_seq / d_offsets / d_rows / out_n_bytes / out_n_records or
 * only one of d_aux / d_out_aux.  n_records == 0 or n_bytes == 0: NTK_OK, 0 and 0.  Synchronous. */
int ntk_read_trim_compact_device(ntk_read_trim *t, const uint8_t *d_seq, const uint8_t *d_aux, uint64_t n_bytes,
                                 const uint64_t *d_offsets, uint64_t n_records, const struct ntk_read_trim_row *d_rows,
                                 uint8_t *d_out_seq, uint8_t *d_out_aux, uint64_t out_cap_bytes, uint64_t *d_out_offsets,
                                 uint64_t *d_out_source, uint64_t out_cap_records, uint64_t *out_n_bytes, uint64_t *out_n_records);

#ifdef __cplusplus
}
#endif

#endif /* NEEDLETAIL_AMD_TRIM_H */
