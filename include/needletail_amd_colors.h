/*
 * needletail_amd_colors.h — a coloured k-mer index on the GPU and the read screen against it (libneedletail_amd_colors.so).
 *
 * Which of N references does each read belong to: host / phiX / adapter depletion, contamination screens, binning reads by strain,
 * choosing the closest of several assemblies.  The index maps a k-mer to the SET of references ("colours", at most 64) that hold it,
 * one bit each; ntk_kmer_colors_run_device goes over a device batch once and writes, per record, how many of its k-mers every colour
 * holds, how many it holds alone, and the best and second-best colour.  Exact 64-bit integers throughout: no estimate, no floating
 * point.
 *
 * A consumer of the core's public ABI: the k-mers of a record are the values ntk_materialize_device_quality emits (every path, tie
 * rule, alphabet and quality mask is the core's), k = 1..32 on every NTK_PATH_*.  The keys that are added are taken as given, as
 * ntk_kmer_table_lookup_device takes its queries: the lists ntk_kmer_table_extract_device and ntk_kmer_sets_apply_device leave on the
 * device are the usual source, on the same k and path as the reads.  Every call returns a status code of needletail_amd.h.  A handle
 * is used by one thread at a time, like its context, and must be destroyed before its context.
 *
 * The index: keys[slots] and masks[slots], 16 B per slot, slots = the smallest power of two at which `capacity` is at most 75 % load;
 * slot = fmix64(key) & (slots - 1), then linear probing over at most min(slots, 4096) slots.  A key is written once, its mask only
 * gains bits.
 *
 * Memory on the device, owned by the handle: the index (16 B per slot) and 68 words of statistics, from create to destroy; and the
 * scratch of ntk_kmer_colors_run_device, grown on demand, kept between calls and freed by ntk_kmer_colors_release or destroy: one
 * chunk of the materialise face (8.25 B per base of at most 64 MiB of bases plus a halo of at most 32 bases, rounded up to 16) and the
 * list of long records (8 B per 16 384 bases of the batch, plus 16 B).  No array is proportional to the bases of the batch: the
 * lookup is fused into the per-record kernel, which reads the chunk's values where the core left them.
 */
#ifndef NEEDLETAIL_AMD_COLORS_H
#define NEEDLETAIL_AMD_COLORS_H

#include "needletail_amd.h"

#ifdef __cplusplus
extern "C" {
#endif

#define NTK_COLORS_MAX 64u
#define NTK_COLORS_NONE 0xFFFFFFFFFFFFFFFFull /* best / second of a row: no such colour */

typedef struct ntk_kmer_colors ntk_kmer_colors;

/* (struct tags, not typedefs: ntk_kmer_colors_stats is also the function that fills it) */
struct ntk_kmer_colors_stats {
    uint64_t n_keys;         /* distinct keys the index holds                                                       */
    uint64_t n_dropped;      /* occurrences that reached the probe bound: the index is incomplete while this is > 0 */
    uint64_t n_masked_bits;  /* bits at or above n_colors that per-key masks carried (cleared before the OR)        */
    uint64_t slots;
    uint64_t device_bytes;   /* device memory held now                                                              */
    uint64_t n_launches;     /* kernel launches of this library since create                                        */
    uint64_t per_color[64];  /* keys that hold each bit                                                             */
    uint32_t n_colors, k, path, reserved;
};

/* One per record, 40 B.  With m(x) the index's mask of k-mer x (0 when absent). */
struct ntk_kmer_colors_row {
    uint64_t n_kmers;   /* k-mers the record emits: exactly the windows ntk_kmer_table_count_device would insert           */
    uint64_t n_hit;     /* of those: m != 0                                                                                 */
    uint64_t n_single;  /* of those: m has exactly one bit                                                                  */
    uint64_t best;      /* the colour with the most hits, ties to the smallest colour; NTK_COLORS_NONE when n_hit == 0      */
    uint64_t second;    /* the best of the other colours by the same rule; NTK_COLORS_NONE when no other colour has a hit   */
};

/* An empty index of n_colors = 1..NTK_COLORS_MAX colours for `capacity` >= 1 distinct keys of k = 1..32 (otherwise NTK_ERR_BAD_K) on
 * `path`.  NULL pointers, a path that does not exist, n_colors 0 or above 64, capacity 0 or above 3 * 2^38: NTK_ERR_BAD_ARG. */
int ntk_kmer_colors_create(ntk_ctx *ctx, uint32_t k, uint32_t path, uint32_t n_colors, uint64_t capacity, ntk_kmer_colors **out);
void ntk_kmer_colors_destroy(ntk_kmer_colors *h);
/* Empties the index (queued on the stream). */
int ntk_kmer_colors_reset(ntk_kmer_colors *h);
/* For i = 0 .. n - 1: ORs d_masks[i] into the entry of d_keys[i], inserting the key if it is absent; with d_masks == NULL it ORs `mask`
 * for every key ("add reference c": mask = 1 << c with the list of c).  Device arrays, 8-byte aligned; keys need not ascend and may
 * repeat.  Queued on the stream.  A `mask` with a bit at or above n_colors (d_masks == NULL) is NTK_ERR_BAD_ARG; such bits of a
 * d_masks[i] are cleared on the device and counted in n_masked_bits.  A key whose mask is then 0 is not inserted.  An occurrence that
 * finds no slot within the probe bound is counted in n_dropped.  n == 0 is NTK_OK. */
int ntk_kmer_colors_add_device(ntk_kmer_colors *h, const uint64_t *d_keys, const uint64_t *d_masks, uint64_t mask, uint64_t n);
/* Synchronises; per_color comes from a pass over the index. */
int ntk_kmer_colors_stats(ntk_kmer_colors *h, struct ntk_kmer_colors_stats *out);
/* d_masks[i] = the mask of d_queries[i], 0 when absent.  NTK_ERR_CAPACITY when n_dropped > 0, and nothing is written: an incomplete
 * index never reads as a complete one.  Synchronous. */
int ntk_kmer_colors_lookup_device(ntk_kmer_colors *h, const uint64_t *d_queries, uint64_t n, uint64_t *d_masks);
/* The screen.  d_rows[r] = the row of record r; d_hits[r * n_colors + c] = the number of the record's k-mers with bit c in m(x);
 * d_single[r * n_colors + c] = those with m(x) == 1 << c exactly (d_single may be NULL).  Device memory, 8-byte aligned.  A record
 * that emits no k-mer (empty, shorter than k, all N) has all-zero counts and best = second = NTK_COLORS_NONE.
 *
 * Input: the device batch layout, alignment and readable range of ntk_reduce_device, plus the packer's record offsets on the device:
 * d_offsets[0 .. n_records], d_offsets[0] = 0, d_offsets[n_records] = n_bytes, record r = the bytes [d_offsets[r], d_offsets[r + 1])
 * whose last byte is the record's break byte (what ntk_batch_buffers returns, uploaded).  An empty record is one break byte.  d_qual
 * (may be NULL) and the cutoff in p->flags bits 15:8 mask bases as ntk_kmer_table_count_device does.  An offset beyond n_bytes is read
 * as n_bytes; no byte outside the batch is touched.
 *
 * Which k-mers: exactly the values ntk_materialize_device_quality marks valid for p.  A window never spans a break byte, so a
 * record's k-mers are those whose last byte lies inside the record.  p->k and p->path must be the handle's and every p->flags bit
 * other than the cutoff 0: NTK_ERR_BAD_ARG otherwise.  Byte-path input that was not normalised (NTK_PATH_BYTES_CANONICAL with pre
 * NONE / STRIP_RETURNS) is NTK_ERR_UNSUPPORTED.  A NULL d_seq, d_offsets, d_rows or d_hits with non-zero sizes, or a misaligned
 * pointer, is NTK_ERR_BAD_ARG.  An index with n_dropped > 0 gives NTK_ERR_CAPACITY and nothing is written.  n_records == 0 or
 * n_bytes == 0 is NTK_OK and touches nothing.
 *
 * Synchronous: the call returns after everything is written.  A record may be longer than a 64 MiB chunk. */
int ntk_kmer_colors_run_device(ntk_kmer_colors *h, const uint8_t *d_seq, const uint8_t *d_qual, uint64_t n_bytes,
                               const uint64_t *d_offsets, uint64_t n_records, const ntk_params *p,
                               struct ntk_kmer_colors_row *d_rows, uint64_t *d_hits, uint64_t *d_single);
/* Frees the scratch ntk_kmer_colors_run_device grew (synchronises); the index stays. */
int ntk_kmer_colors_release(ntk_kmer_colors *h);

#ifdef __cplusplus
}
#endif

#endif /* NEEDLETAIL_AMD_COLORS_H */
