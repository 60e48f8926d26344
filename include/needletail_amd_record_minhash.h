/*
 * needletail_amd_record_minhash.h — one MinHash sketch per record of a device batch, all of them in one call
 * (libneedletail_amd_record_minhash.so): a multi-FASTA of genomes, a set of contigs, long reads for an overlap screen - the jobs of
 * `mash sketch -i` and `sourmash sketch --singleton`.  The sketches are needletail_amd_minhash.h's (bottom-s or scaled, with abundance),
 * and the result is what ntk_mhset_add of needletail_amd_minhash_set.h takes.
 *
 * THE RULE.  After ntk_record_minhash_run_device, record r's sketch is exactly what an ntk_minhash of the same k, path and kind holds
 * after reset + add_device on a batch of that record alone (same pre, quality stream and cutoff): the same keys (the values
 * ntk_materialize_device_quality marks valid, k = 1..32), the same hash h = fmix64(key ^ NTK_MINHASH_XOR), the kept hashes strictly
 * ascending, behind each the EXACT number of the record's k-mers that hashed to it, cut to the num smallest or to every h <=
 * (2^64 - 1) / scaled, and n_windows[r] the exact number of k-mers the record emits.  A record's k-mers are those whose last byte lies
 * inside the record and whose first byte does too: the window ends [offsets[r] + k - 1, offsets[r + 1] - 1), as in
 * needletail_amd_abundance.h - the record's last byte is its break byte.
 *
 * Input: what ntk_read_abundance_run_device takes - a device batch in the layout, alignment and readable range of ntk_reduce_device,
 * and the n_records + 1 record starts the batch packer reports (ntk_batch_buffers), on the device, non-decreasing.  An offset beyond
 * n_bytes reads as n_bytes.  A record may be longer than the 64 Mi bases that are materialised per pass.  Records do not span calls.
 *
 * How.  Chunk by chunk of the materialise face, a filter kernel finds every window's record from the offsets (one search per wave,
 * then it advances), hashes the value and appends (record, hash) where h <= tau[r], a PER-RECORD threshold, to a candidate buffer of
 * `buffer_entries` pairs (12 B each).  A launch whose appends do not fit is discarded whole and redone in pieces that fit (n_redone),
 * so nothing is ever dropped.  The buffer is sorted by (record, hash), equal pairs are counted, the list is combined with the kept
 * (record, hash, count) list and cut to the first `num` per record.
 *   scaled: tau[r] = max_hash for every record; one round.
 *   num:    a record has no threshold of its own until it is sketched, so it is guessed and verified.  A record of at most
 *           NTK_RECORD_MINHASH_ALLPASS * num candidate window ends (or fewer than the guess expects to pass) takes tau = ~0: everything
 *           passes.  A longer one takes the tau below which 2 * num + 16 of its hashes are expected.  After the round a record is
 *           ACCEPTED iff tau[r] == ~0 or it holds at least num distinct hashes <= tau[r]: then its num smallest and their counts are
 *           exact.  Every other record (repetitive, low-complexity: fewer distinct k-mers than any guess assumes) goes into the next
 *           round with a raised threshold, ending at ~0; only its windows are scanned again, and only for the hashes above the old
 *           threshold.  n_rounds and n_retried_records count that.
 * No value pads the buffer, so the legal hash 2^64 - 1 is a hash like any other.
 *
 * Every call returns a status code of needletail_amd.h.  run_device, read, stats and trim are SYNCHRONOUS: they return when the work
 * they queued on the context's stream is done.  A handle is used by one thread at a time, like its context, and must be destroyed
 * before its context.
 *
 * A run_device that fails halfway through its work on the device (NTK_ERR_NOMEM, NTK_ERR_HIP, a failure of the materialise pass)
 * leaves the handle marked: read and stats return that status again until the next run_device, which starts over.  Refused arguments
 * (NTK_ERR_BAD_ARG, NTK_ERR_BAD_K, NTK_ERR_UNSUPPORTED) and NTK_ERR_CAPACITY from read change nothing: the held result stays.
 *
 * Known costs.  A hash at or below its record's threshold that occurs N times in the record is appended N times (the hot-key case of
 * needletail_amd_minhash.h).  A record that ends at tau = ~0 costs 12 B and a sort per window.  A batch of several chunks that needs a
 * further round is materialised again for it.  In a further round every block of the retry kernel walks the whole list of retried
 * records (two loads each), so a batch in which most of 100 000 records are low-complexity pays about 2 * 10^8 such loads per round, and
 * there can be up to 33 rounds.  In the first round a wave steps over the record starts inside its tiles one by one: a long run of
 * empty records (equal offsets) is walked serially, by the wave and again by each lane of a tile that holds a start.  None of these
 * cases has been timed.  The sum of all sketch sizes of one call, plus buffer_entries, must stay below 2^32
 * (NTK_ERR_CAPACITY).
 *
 * Memory on the device, freed by trim and destroy (ntk_record_minhash_stats reports the sum): the materialise scratch of one chunk
 * (8.25 B per base, 64 Mi bases at most); the candidate buffer, 12 B * buffer_entries; per record 33 B (thresholds, state, retry list,
 * window count, sketch start); the kept list, 20 B per kept entry; and the work arrays of a fold, about 90 B per entry folded (the
 * buffer's fill plus the kept entries of the records it touches) with rocPRIM's temporary storage.
 */
#ifndef NEEDLETAIL_AMD_RECORD_MINHASH_H
#define NEEDLETAIL_AMD_RECORD_MINHASH_H

#include "needletail_amd.h"

#ifdef __cplusplus
extern "C" {
#endif

#define NTK_RECORD_MINHASH_XOR 0x9E3779B97F4A7C15ull      /* = NTK_MINHASH_XOR: the hash is that library's            */
#define NTK_RECORD_MINHASH_MAX_NUM (1ull << 20)           /* = NTK_MINHASH_MAX_NUM                                    */
#define NTK_RECORD_MINHASH_ALLPASS 4ull                   /* records of at most ALLPASS * num window ends: tau = ~0   */
#define NTK_RECORD_MINHASH_BUFFER_DEFAULT (1ull << 24)    /* buffer_entries = 0 means this                            */
#define NTK_RECORD_MINHASH_BUFFER_MIN 256ull              /* one wave's tile of window ends                           */
#define NTK_RECORD_MINHASH_BUFFER_MAX (1ull << 30)

typedef struct ntk_record_minhash ntk_record_minhash;

/* (a struct tag, not a typedef: ntk_record_minhash_stats is also the function that fills it) */
struct ntk_record_minhash_stats {
    uint64_t n_records;         /* of the held result                                                                       */
    uint64_t n_entries;         /* kept hashes of all its records: offsets[n_records]                                       */
    uint64_t n_windows;         /* k-mers of all its records (the sum of n_windows[r])                                      */
    uint64_t num, scaled;
    uint64_t buffer_entries;    /* the candidate buffer's size in pairs (the default resolved)                              */
    uint64_t n_rounds;          /* rounds of the last run: 1, or more where records were retried; 0 before any run          */
    uint64_t n_retried_records; /* records of the last run that were not accepted after its first round                     */
    uint64_t n_redone;          /* launches of the last run whose appends did not fit and were discarded and redone         */
    uint64_t device_bytes;      /* device memory the handle holds now                                                       */
    uint32_t k, path;
};

/* k = 1..32 on any NTK_PATH_*; k = 0 and k >= 33: NTK_ERR_BAD_K; no such path: NTK_ERR_BAD_ARG.  Exactly one of num (at most
 * NTK_RECORD_MINHASH_MAX_NUM) and scaled is non-zero, and buffer_entries is 0 (the default) or within NTK_RECORD_MINHASH_BUFFER_MIN ..
 * NTK_RECORD_MINHASH_BUFFER_MAX: NTK_ERR_BAD_ARG otherwise.  buffer_entries is a memory knob only (12 B per pair): a smaller buffer
 * means more folds, and more redone launches where many hashes pass.  The handle holds no result and works on ctx's device and
 * stream. */
int ntk_record_minhash_create(ntk_ctx *ctx, uint32_t k, uint32_t path, uint64_t num, uint64_t scaled, uint64_t buffer_entries,
                              ntk_record_minhash **out);
void ntk_record_minhash_destroy(ntk_record_minhash *m);
/* Sketches every record of the batch (synchronous); the result replaces the one held.  d_qual (may be NULL) and the cutoff in
 * p->flags bits 15:8 mask bases as ntk_reduce_device_quality does.  p->k and p->path must be the handle's and every other p->flags bit
 * 0: NTK_ERR_BAD_ARG otherwise.  Byte-path input that was not normalised (NTK_PATH_BYTES_CANONICAL with pre NONE / STRIP_RETURNS) is
 * NTK_ERR_UNSUPPORTED.  n_records == 0 or n_bytes == 0 is NTK_OK and holds n_records empty sketches.  d_seq or d_qual not 16-byte
 * aligned, d_offsets NULL or not 8-byte aligned, n_records >= 2^32: NTK_ERR_BAD_ARG. */
int ntk_record_minhash_run_device(ntk_record_minhash *m, const uint8_t *d_seq, const uint8_t *d_qual, uint64_t n_bytes,
                                  const uint64_t *d_offsets, uint64_t n_records, const ntk_params *p);
/* The held result as a CSR in host arrays (synchronous): record r's hashes, strictly ascending, and their counts are
 * hashes[offsets[r] .. offsets[r + 1]) and counts[...]; offsets has n_records + 1 entries, n_windows (may be NULL) n_records;
 * *n = offsets[n_records].  hashes and counts hold `cap` entries each: cap too small is NTK_ERR_CAPACITY with *n = the size needed
 * and NOTHING written (offsets and n_windows neither); NULL arrays with cap 0 ask for the size that way.  offsets == NULL: only *n is set.
 * Before any run: *n = 0 and nothing is written. */
int ntk_record_minhash_read(ntk_record_minhash *m, uint64_t *offsets, uint64_t *n_windows, uint64_t *hashes, uint64_t *counts,
                            uint64_t cap, uint64_t *n);
/* What the handle holds and what the last run did (synchronous). */
int ntk_record_minhash_stats(ntk_record_minhash *m, struct ntk_record_minhash_stats *out);
/* Frees every device array, the held result included (synchronous): read answers *n = 0 afterwards, as before any run. */
int ntk_record_minhash_trim(ntk_record_minhash *m);

#ifdef __cplusplus
}
#endif

#endif /* NEEDLETAIL_AMD_RECORD_MINHASH_H */
