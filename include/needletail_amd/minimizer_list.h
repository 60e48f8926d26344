/*
 * needletail_amd/minimizer_list.h — the (w, k) windowed minimizers of every record of a device batch as lists
 * (libneedletail_amd_minimizer_list.so): per record the positions, values and strands of its minimizers with the number of windows
 * each one won - what minimap2's mm_sketch and mashmap hand to seeding, and where KMC- and Jellyfish-style partitioning cut
 * super-k-mers.  ntk_minimizers_reduce_device of needletail_amd.h digests the same minimizers into counters; this library keeps them.
 * The result is a CSR that stays on the device and can be read back.  It is exact and deterministic.
 *
 * THE RULE.  Fix k = 1..32, w = 1..NTK_MINIMIZER_LIST_W_MAX, a path (any NTK_PATH_*) and an order.
 *   Keys.      The values ntk_materialize_device_quality marks valid are the keys (the rule of needletail_amd_record_minhash.h: the same
 *              pre, quality stream and cutoff); the strand flag is that face's rc plane.  A k-mer is named by its window END byte e.
 *   Windows.   A window is w consecutive valid window ends - on a normalised batch w + k - 1 good bases.  Break bytes, N and masked
 *              bases end windows.  The window that ends at e holds the k-mers that end at e - w + 1 .. e.
 *   Minimizer. The minimizer of a window is its LEFTMOST k-mer whose key is smallest under the order:
 *              NTK_MINIMIZER_LIST_LEX   the value itself.  On a canonical path this is sequence::minimizer(window, k) of every window,
 *                                       i.e. what ntk_minimizers_reduce_device digests; the strand flag is that k-mer's own iterator
 *                                       flag under the path's tie rule.
 *              NTK_MINIMIZER_LIST_HASH  fmix64(value ^ NTK_MINIMIZER_LIST_XOR), the hash of the two MinHash libraries: a bijection,
 *                                       so equal hashes are equal values and "leftmost" stays well defined.  The random order that
 *                                       minimap2-style users expect; the lexicographic one over-samples poly-A.
 *   Entries.   Consecutive windows that pick the same k-mer are ONE entry:
 *                pos    start of the k-mer relative to its record's start (u64);
 *                value  the key as materialised, never the hash (u64);
 *                info   u32: bit 0 = the strand flag, bits 31:1 = span.
 *   Span.      span is the number of consecutive windows the entry won, 1 <= span <= w: the windows that end at e .. e + span - 1,
 *              e its first window end.  Those windows together are the entry's super-k-mer: span + w + k - 2 bases that end at
 *              e + span - 1.
 *   Ordering.  Inside a run of windows the positions strictly increase; entries are held in ascending order of first window end.
 *   Records.   The n_records + 1 record starts the batch packer reports (ntk_batch_buffers), on the device, non-decreasing; an offset
 *              beyond n_bytes reads as n_bytes; every record's last byte is its break byte.  Offsets only ATTRIBUTE, they never cut a
 *              window - the break bytes do that.  offsets_out[r] = the number of held entries whose first window end is below
 *              min(offsets[r], n_bytes); record r's entries are [offsets_out[r], offsets_out[r + 1]), and pos is relative to the last
 *              record start at or before the first window end (to the batch's start where there is none).  The sum of span over all
 *              held entries is the number of windows of the batch: on a canonical path in LEX order n_total of
 *              ntk_minimizers_reduce_device, whatever the offsets.  OFFSETS THAT ARE NOT THE PACKER'S ARE NOT VERIFIED: entries in
 *              front of offsets[0] or behind offsets[n_records] are held outside every record's range, and a pos in a record that
 *              starts inside a window wraps.
 *
 * Input: what ntk_record_minhash_run_device takes - a device batch in the layout, alignment and readable range of ntk_reduce_device.  A
 * record may be longer than the 64 Mi bases that are materialised per pass.  Records do not span calls.
 *
 * How.  Chunk by chunk of the materialise face.  A chunk after the first is materialised from a halo in front of it (a multiple of 16,
 * at least k + w - 1 bytes: the window one end before the chunk is whole there, and its choice decides whether the chunk's first window
 * opens an entry) and w - 1 window ends FURTHER than its own, so that an entry that opens in a chunk's last ends finds its whole span in
 * the same pass; no entry is completed later.  ml_select_kernel: a block of 256 threads takes a tile of 1024 window ends plus w in front
 * of them into LDS as (key, slot) pairs, doubles M_2q[x] = min(M_q[x - q], M_q[x]) up to the largest power of two <= w, takes every window
 * as two overlapping ranges (log2 w steps for any w; the pair is unique, so overlap is exact), and writes per end a 2-byte word: the
 * distance to the picked end, "whole" and "opens an entry"; it counts the opening ends of its tile.  ml_scan_kernel scans the tiles'
 * counts (one block), then ml_scatter_kernel ranks the opening ends inside a tile and writes pos, value, info and the first window end; the span
 * is read from the words of the next w - 1 ends.  ml_offsets_kernel searches the record starts in the ascending first-window-end list.
 * LDS 15 KiB per block; the grid of the two tile kernels is at most 8 blocks per compute unit, and they loop.  None of this has been
 * tuned: the tile length, the LDS and the occupancy are first choices.
 *
 * Every call returns a status code of needletail_amd.h.  run_device, read, stats and trim are SYNCHRONOUS: they return when the work
 * they queued on the context's stream is done.  result_device is host-side only.  A handle is used by one thread at a time, like its
 * context, and must be destroyed before its context.
 *
 * A run_device that fails halfway through its work on the device (NTK_ERR_NOMEM, NTK_ERR_HIP, a failure of the materialise pass)
 * leaves the handle marked: read, result_device and stats return that status again until the next run_device, which starts over.
 * Refused arguments (NTK_ERR_BAD_ARG, NTK_ERR_BAD_K, NTK_ERR_UNSUPPORTED) and NTK_ERR_CAPACITY from read change nothing: the held
 * result stays.  Every refusal comes before any device call.
 *
 * Memory on the device, freed by trim and destroy (ntk_minimizer_list_stats reports the sum): the materialise scratch of one chunk
 * (8.25 B per base; 64 Mi bases plus a halo of at most 288 and a tail of at most 255 bases); the held list, 20 B per entry plus 8 B per
 * record; and the compaction's work arrays: the first window ends, 8 B per entry; the window ends' words, 2 B per base of one chunk; the
 * tiles' counts and their scan, 8 B per 1024 bases of one chunk; and 2 counter words.  The arrays per entry and per record grow by half
 * again and 64.  No array is proportional to the bases of the batch beyond one chunk.
 */
#ifndef NEEDLETAIL_AMD_MINIMIZER_LIST_H
#define NEEDLETAIL_AMD_MINIMIZER_LIST_H

#include "needletail_amd.h"

#ifdef __cplusplus
extern "C" {
#endif

#define NTK_MINIMIZER_LIST_LEX 0u
#define NTK_MINIMIZER_LIST_HASH 1u
#define NTK_MINIMIZER_LIST_W_MAX 256u
#define NTK_MINIMIZER_LIST_XOR 0x9E3779B97F4A7C15ull      /* = NTK_MINHASH_XOR: the hash is that library's */

typedef struct ntk_minimizer_list ntk_minimizer_list;

/* (a struct tag, not a typedef: ntk_minimizer_list_stats is also the function that fills it) */
struct ntk_minimizer_list_stats {
    uint64_t n_records;         /* of the held result                                                                       */
    uint64_t n_entries;         /* held entries                                                                             */
    uint64_t n_windows;         /* windows of the batch: the sum of span over the held entries                              */
    uint64_t n_chunks;          /* chunks the last run materialised                                                         */
    uint64_t device_bytes;      /* device memory the handle holds now                                                       */
    uint32_t k, path, w, order;
};

/* k = 1..32 on any NTK_PATH_*; k = 0 and k >= 33: NTK_ERR_BAD_K; no such path, w = 0, w > NTK_MINIMIZER_LIST_W_MAX or order > 1:
 * NTK_ERR_BAD_ARG.  The handle holds no result and works on ctx's device and stream. */
int ntk_minimizer_list_create(ntk_ctx *ctx, uint32_t k, uint32_t path, uint32_t w, uint32_t order, ntk_minimizer_list **out);
void ntk_minimizer_list_destroy(ntk_minimizer_list *m);
/* Lists the minimizers of every record of the batch (synchronous); the result replaces the one held.  d_qual (may be NULL) and the
 * cutoff in p->flags bits 15:8 mask bases as ntk_reduce_device_quality does.  p->k and p->path must be the handle's and every other
 * p->flags bit 0 (w is the handle's): NTK_ERR_BAD_ARG otherwise.  Byte-path input that was not normalised (NTK_PATH_BYTES_CANONICAL with
 * pre NONE / STRIP_RETURNS) is NTK_ERR_UNSUPPORTED.  n_records == 0 or n_bytes == 0 is NTK_OK and holds n_records empty ranges.  d_seq
 * or d_qual not 16-byte aligned, d_offsets NULL or not 8-byte aligned, n_records >= 2^32: NTK_ERR_BAD_ARG. */
int ntk_minimizer_list_run_device(ntk_minimizer_list *m, const uint8_t *d_seq, const uint8_t *d_qual, uint64_t n_bytes,
                                  const uint64_t *d_offsets, uint64_t n_records, const ntk_params *p);
/* The held result as a CSR in host arrays (synchronous): record r's entries are pos, values and info [offsets[r] .. offsets[r + 1]);
 * offsets has n_records + 1 entries; *n = the number of held entries.  pos, values and info hold `cap` entries each: cap too small is
 * NTK_ERR_CAPACITY with *n = the size needed and NOTHING written (offsets neither); NULL arrays with cap 0 ask for the size that way.
 * offsets == NULL: only *n is set.  Before any run: *n = 0 and nothing is written. */
int ntk_minimizer_list_read(ntk_minimizer_list *m, uint64_t *offsets, uint64_t *pos, uint64_t *values, uint32_t *info,
                            uint64_t cap, uint64_t *n);
/* The held result where it lies on the device; host-side only: queues nothing and waits for nothing.  The arrays are those of read, *n
 * the number of entries; the pointers stay valid until the next run_device, trim or destroy.  Before any run: NULL pointers, *n = 0. */
int ntk_minimizer_list_result_device(ntk_minimizer_list *m, const uint64_t **d_offsets, const uint64_t **d_pos,
                                     const uint64_t **d_values, const uint32_t **d_info, uint64_t *n);
/* What the handle holds and what the last run did (synchronous). */
int ntk_minimizer_list_stats(ntk_minimizer_list *m, struct ntk_minimizer_list_stats *out);
/* Frees every device array, the held result included (synchronous): read answers *n = 0 afterwards, as before any run. */
int ntk_minimizer_list_trim(ntk_minimizer_list *m);

#ifdef __cplusplus
}
#endif

#endif /* NEEDLETAIL_AMD_MINIMIZER_LIST_H */
