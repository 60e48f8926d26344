/*
 * needletail_amd_sketch.h — how many distinct k-mers does a batch hold?  A HyperLogLog sketch on the device
 * (libneedletail_amd_sketch.so), made to size the count tables of needletail_amd_count.h / needletail_amd_wide_count.h.
 *
 * Both tables are fixed-size and take `capacity`, the number of distinct k-mers they must hold, which nobody knows before counting.
 * The sketch answers it in a first cheap pass over the same device batches: sketch -> ntk_kmer_sketch_estimate -> `capacity` ->
 * ntk_kmer_table_create / ntk_wide_table_create -> count.  The capacity it gives is never too small (5 standard errors of the
 * estimator above the estimate) and costs at most one doubling of the table.
 *
 * Which k-mers: exactly the keys the matching table would insert for the same call - k = 1..32 on every NTK_PATH_* (the value
 * ntk_materialize_device_quality emits: canonical on the canonical paths, forward on NTK_PATH_BITS), k = 33..63 on
 * NTK_PATH_BYTES_CANONICAL (the two-word key {hi, lo} of needletail_amd_wide_count.h).
 *
 * The sketch (fixed here, restated by the tests' host model): m = 2^14 registers of one byte.  One 64-bit hash h per key, from the
 * tables' hash fmix64 (the murmur3 finaliser): h = fmix64(key ^ C) for a one-word key, h = fmix64(lo ^ fmix64(hi) ^ C) for {hi, lo},
 * C = NTK_SKETCH_XOR (so that key 0, AAA...A, does not hash to 0).  Register index = the top NTK_SKETCH_P bits of h; rank = 1 + the
 * number of leading zeros of the remaining 50 bits (51 when they are all zero); a register holds the largest rank seen.  The
 * registers are a function of the SET of keys: the order of the k-mers, the split into calls and batches, and repeats do not change
 * them, and two sketches merge by element-wise max.
 *
 * Every call returns a status code of needletail_amd.h.  reset and add_device are asynchronous on the context's stream; registers,
 * merge and estimate synchronise it.  A sketch is used by one thread at a time, like its context, and must be destroyed before its
 * context.  Memory: 64 KiB of registers on the device, plus for k <= 32 the materialise scratch of one chunk of input (64 MiB of
 * bases at most: 10 B per base), freed by destroy; k = 33..63 keeps no scratch.
 */
#ifndef NEEDLETAIL_AMD_SKETCH_H
#define NEEDLETAIL_AMD_SKETCH_H

#include "needletail_amd.h"

#ifdef __cplusplus
extern "C" {
#endif

#define NTK_SKETCH_P 14                           /* index bits                     */
#define NTK_SKETCH_REGISTERS (1u << NTK_SKETCH_P) /* m = 16384                      */
#define NTK_SKETCH_MAX_RANK 51                    /* 64 - NTK_SKETCH_P + 1          */
#define NTK_SKETCH_XOR 0x9E3779B97F4A7C15ull      /* C: xored into the key's hash input */

typedef struct ntk_kmer_sketch ntk_kmer_sketch;

/* (a struct tag, not a typedef: the name is also the function that fills it) */
struct ntk_kmer_sketch_estimate {
    double distinct;         /* the estimate of the number of distinct k-mers added since reset                          */
    uint64_t n_windows;      /* EXACT number of k-mers added since reset (every call, every chunk, merges included)      */
    uint64_t capacity;       /* what to pass to ntk_kmer_table_create / ntk_wide_table_create                            */
    uint32_t zero_registers; /* registers still 0 (the estimate is the linear-counting one when > 0 and small, see below) */
    uint32_t k, path;
};

/* k = 1..32 on any NTK_PATH_*, k = 33..63 on NTK_PATH_BYTES_CANONICAL.  k = 0, k >= 64 and k > 32 on a bit path: NTK_ERR_BAD_K; no
 * such path: NTK_ERR_BAD_ARG.  The sketch starts empty and works on ctx's device and stream. */
int ntk_kmer_sketch_create(ntk_ctx *ctx, uint32_t k, uint32_t path, ntk_kmer_sketch **out);
void ntk_kmer_sketch_destroy(ntk_kmer_sketch *s);
/* Empties the sketch: every register 0, n_windows 0 (async). */
int ntk_kmer_sketch_reset(ntk_kmer_sketch *s);
/* Adds every k-mer the batch emits (async): the keys the table of this k and path would count in ntk_kmer_table_count_device /
 * ntk_wide_table_count_device, under the same rules.  Input: the device batch layout, alignment and readable range of
 * ntk_reduce_device.  d_qual (may be NULL) and the cutoff in p->flags bits 15:8 mask bases as ntk_reduce_device_quality does.  p->k
 * and p->path must be the sketch's and every other p->flags bit 0: NTK_ERR_BAD_ARG otherwise.  Byte-path input that was not
 * normalised (NTK_PATH_BYTES_CANONICAL with pre NONE / STRIP_RETURNS) is NTK_ERR_UNSUPPORTED.  n_bytes == 0 is NTK_OK.  Calls
 * accumulate until ntk_kmer_sketch_reset. */
int ntk_kmer_sketch_add_device(ntk_kmer_sketch *s, const uint8_t *d_seq, const uint8_t *d_qual, uint64_t n_bytes,
                               const ntk_params *p);
/* The registers as NTK_SKETCH_REGISTERS bytes in host memory (synchronises). */
int ntk_kmer_sketch_registers(ntk_kmer_sketch *s, uint8_t *regs);
/* Folds in a sketch made elsewhere (another context, GPU or process) of the same k and path: element-wise max with its
 * NTK_SKETCH_REGISTERS bytes in host memory, and its n_windows added (synchronises).  A byte above NTK_SKETCH_MAX_RANK or a NULL
 * pointer is NTK_ERR_BAD_ARG.  n_windows must be that sketch's complete count: the capacity is clamped to the total. */
int ntk_kmer_sketch_merge(ntk_kmer_sketch *s, const uint8_t *regs, uint64_t n_windows);
/* The estimate and the capacity (synchronises).  Host arithmetic in double on the registers alone, so anyone holding the registers
 * can repeat it: with c[r] = the number of registers equal to r, Z = sum over r = 51 down to 0 of c[r] * 2^-r (added in that order),
 * E = a m^2 / Z with a = 0.7213 / (1 + 1.079 / m); when E <= 2.5 m and V = c[0] > 0, E = m ln(m / V) (linear counting).  Hashes of
 * 64 bits need no large-range correction.
 * capacity = ceil(E * (1 + 5 * 1.04 / sqrt(m))) + 8, then at most n_windows, at most 4^k where k < 32, and at least 1 (the tables
 * refuse 0; an empty sketch says 1).  1.04 / sqrt(m) = 0.8125 % is the estimator's relative standard error. */
int ntk_kmer_sketch_estimate(ntk_kmer_sketch *s, struct ntk_kmer_sketch_estimate *out);

#ifdef __cplusplus
}
#endif

#endif /* NEEDLETAIL_AMD_SKETCH_H */
