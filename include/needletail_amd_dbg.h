/*
 * needletail_amd_dbg.h — the compacted de Bruijn graph of a k-mer list on the GPU (libneedletail_amd_dbg.so): the edge byte of every
 * k-mer with exact degree totals, the unitigs (maximal non-branching paths and isolated cycles) with their lengths and summed counts,
 * and the unitigs spelled out as a device batch that the count tables, the sketches, MinHash and the trimmer take as it is.
 *
 * THE INPUT is a k-mer list as needletail_amd_kmer_sets.h defines it, with key_words = 1, of CANONICAL keys: what
 * ntk_kmer_table_extract_device writes for a table on a canonical path, and what every result of ntk_kmer_sets_apply_device on such
 * lists is.  k is odd, 3..31 (an even k, or one outside that range, is NTK_ERR_BAD_K: with an odd k no k-mer is its own reverse
 * complement and no rule below has a tie); n <= 2^31 - 1 (more: NTK_ERR_UNSUPPORTED).  Encoding: A C G T = 0 1 2 3, the first base
 * most significant, complement = code ^ 3; a key is the smaller of a k-mer's value and its reverse complement's.
 *
 * THE RULE.  s = the string of key x.
 *   Half-edge (x, side, c), side 0 / 1, c = 0..3, leads to the string t = s[1:] + c (side 0) or rc(s)[1:] + c (side 1); its target is
 *   y = canon(t).  Bit 4 * side + c of x's EDGE BYTE is set iff y is in the list, y == x included.
 *   Its mate is (y, side', c'): side' = 1 if t is y's canonical string, else 0; c' = the complement of the first base of the string x
 *   was extended from.  The mate's target is x, so a bit is set iff its mate's is.
 *   A half-edge is a LINK iff its bit is the only bit of its nibble, y != x, and the mate's nibble has exactly one bit.  Links pair
 *   up and every (k-mer, side) has at most one: the link graph is a disjoint union of paths and cycles, the UNITIGS (a lone k-mer is a
 *   path of one).
 *   A path is spelled from the end k-mer with the smaller key; a single k-mer as its canonical string; a cycle from its smallest key
 *   in canonical orientation, leaving through that key's side 0, and open: L k-mers, L + k - 1 bases.  Unitigs are numbered by
 *   ascending key of their first k-mer.
 *
 * Every call returns a status code of needletail_amd.h and is synchronous on the context's stream.  A handle is used by one thread at
 * a time, like its context, and must be destroyed before its context.  Refused arguments change nothing.  The calls trust the list:
 * on one that does not ascend or holds keys that are not canonical the answer is unspecified, but no byte outside the given arrays is
 * read or written (ntk_kmer_sets_validate_device is the cheap pass for callers who do not know).  No floating point; sums are modulo
 * 2^64.
 *
 * Memory on the device, owned by the handle, grown on demand and freed by release or destroy: the prefix directory (4 B per entry,
 * fewer than 2 n + 2 entries) and 9 B per k-mer for adjacency; NTK_DBG_UNITIG_BYTES_PER_KMER per k-mer more for unitigs; 8 B per
 * unitig for spell; rocPRIM's temporary storage; 256 B of sums.
 */
#ifndef NEEDLETAIL_AMD_DBG_H
#define NEEDLETAIL_AMD_DBG_H

#include "needletail_amd.h"

#ifdef __cplusplus
extern "C" {
#endif

#define NTK_DBG_K_MIN 3u
#define NTK_DBG_K_MAX 31u
#define NTK_DBG_N_MAX 0x7FFFFFFFull        /* keys of a list                                                                  */
#define NTK_DBG_UNITIG_BYTES_PER_KMER 96u  /* scratch of ntk_dbg_unitigs_device beyond adjacency's, per k-mer                 */
#define NTK_DBG_FLAG_CYCLE 1ull            /* flags of a unitig row: bit 0; bits 8..11 and 12..15 are the two end degrees     */

typedef struct ntk_dbg ntk_dbg;

/* (struct tags, not typedefs: ntk_dbg_stats is also the function that fills it) */
struct ntk_dbg_stats {
    uint64_t k;
    uint64_t device_bytes;   /* device memory held now                                                  */
    uint64_t n_launches;     /* kernel launches of this library since create (rocPRIM's not counted)    */
    uint64_t n_calls;        /* adjacency, unitigs and spell calls that ran on the device, since create */
    uint64_t n_rounds;       /* pointer-doubling rounds of the last ntk_dbg_unitigs_device call         */
};

/* Exact integers. */
struct ntk_dbg_totals {
    uint64_t n_half_edges;     /* set bits of all edge bytes                                                 */
    uint64_t deg_hist[5][5];   /* k-mers by [set bits of side 0][set bits of side 1]                         */
    uint64_t n_isolated;       /* both sides empty                                                           */
    uint64_t n_tips;           /* one side empty, the other not                                              */
    uint64_t n_branching;      /* some side with more than one bit                                           */
    uint64_t n_self;           /* set bits whose target is the k-mer itself                                  */
    uint64_t n_links;          /* half-edges that are links (an even number)                                 */
};

/* One per k-mer, 8 B. */
struct ntk_dbg_kmer_row {
    uint32_t unitig;     /* the unitig the k-mer is on                                                                            */
    uint32_t pos_flip;   /* its position there << 1 | flipped; flipped: it appears in the spelling as its reverse complement      */
};

/* One per unitig, 32 B. */
struct ntk_dbg_unitig_row {
    uint64_t start_index;  /* index in the list of the unitig's first k-mer                                                       */
    uint64_t n_kmers;      /* L; the unitig has L + k - 1 bases                                                                    */
    uint64_t sum_counts;   /* of its k-mers, modulo 2^64                                                                           */
    uint64_t flags;        /* bit 0: a cycle; bits 8..11: set bits of the nibble behind the first k-mer (the side the spelling does
                              not leave it through); bits 12..15: set bits of the nibble past the last k-mer.  Both are 1 on a cycle */
};

/* k odd, 3..31: NTK_ERR_BAD_K otherwise (checked before the device is looked at).  Works on ctx's device and stream; without a device:
 * NTK_ERR_NO_DEVICE. */
int ntk_dbg_create(ntk_ctx *ctx, uint32_t k, ntk_dbg **out);
void ntk_dbg_destroy(ntk_dbg *h);
/* Frees the scratch that grew with the lists (the next call allocates it again). */
int ntk_dbg_release(ntk_dbg *h);
int ntk_dbg_stats(ntk_dbg *h, struct ntk_dbg_stats *out);
/* d_edges[i] = the edge byte of key i (device memory, n bytes; may be NULL: the totals alone); totals (host memory) may be NULL.
 * d_keys 8-byte aligned, NULL exactly when n == 0 (then the totals are all 0).  n > NTK_DBG_N_MAX: NTK_ERR_UNSUPPORTED. */
int ntk_dbg_adjacency_device(ntk_dbg *h, const uint64_t *d_keys, uint64_t n, uint8_t *d_edges, struct ntk_dbg_totals *totals);
/* The unitigs of the list.  d_kmer_rows[i] (n rows, 8-byte aligned) places key i; d_unitig_rows[u] (cap_unitigs rows, 8-byte aligned)
 * describes unitig u; *n_unitigs = their number, *n_bases = the sum of n_kmers + k - 1 over them.  d_counts: the counts of the list
 * (8-byte aligned).  cap_unitigs too small: NTK_ERR_CAPACITY with *n_unitigs = the number needed, *n_bases set, and nothing written;
 * d_kmer_rows and d_unitig_rows may be NULL with cap_unitigs 0 to ask for it (n always suffices).  n == 0: NTK_OK, 0 and 0. */
int ntk_dbg_unitigs_device(ntk_dbg *h, const uint64_t *d_keys, const uint64_t *d_counts, uint64_t n,
                           struct ntk_dbg_kmer_row *d_kmer_rows, struct ntk_dbg_unitig_row *d_unitig_rows, uint64_t cap_unitigs,
                           uint64_t *n_unitigs, uint64_t *n_bases);
/* Spells the unitigs as upper-case bytes in the device-batch layout of ntk_read_trim_compact_device's output: record u is unitig u's
 * n_kmers + k - 1 bases and one '\n' break byte, d_offsets_out[0 .. n_unitigs] are the record starts (the last one = *out_n_bytes),
 * and d_seq_out is padded with '\n' up to round_up(*out_n_bytes, 16).  Capacity, as there: cap_bytes >= round_up(*out_n_bytes, 16)
 * and cap_records >= n_unitigs are needed (d_offsets_out holds cap_records + 1 words); too small: NTK_ERR_CAPACITY with
 * *out_n_bytes / *out_n_records set and nothing written; d_seq_out and d_offsets_out may be NULL with both capacities 0 to ask.
 * d_seq_out 16-byte aligned, the other arrays 8-byte aligned.  The rows are ntk_dbg_unitigs_device's for the same list; other rows
 * give unspecified bytes, but nothing outside the given arrays is touched.  n == 0 or n_unitigs == 0: NTK_OK, 0 and 0. */
int ntk_dbg_spell_device(ntk_dbg *h, const uint64_t *d_keys, uint64_t n, const struct ntk_dbg_kmer_row *d_kmer_rows,
                         const struct ntk_dbg_unitig_row *d_unitig_rows, uint64_t n_unitigs, uint8_t *d_seq_out, uint64_t cap_bytes,
                         uint64_t *d_offsets_out, uint64_t cap_records, uint64_t *out_n_bytes, uint64_t *out_n_records);

#ifdef __cplusplus
}
#endif

#endif /* NEEDLETAIL_AMD_DBG_H */
