// What every consumer of the core's public ABI shares (the two count tables through ntk_count_common.hpp, the sketch, MinHash, per-read
// abundance and trimming directly): the hash, the wave and block sums, the launch helpers, the handle's base with the checks of a batch
// call, how a handle owns device and pinned memory (ntk_device_mem.hpp), the scratch of the materialise face with the walk over a
// batch's chunks (ntk_chunks.hpp), and the record rule of the two libraries that read records.  Everything is in an anonymous namespace, so each library keeps a private copy and exports nothing new.
// DESIGN.md section 16.
#pragma once

#include "../../include/needletail_amd.h"
#include "ntk_chunks.hpp"

#include <hip/hip_runtime.h>

#define CT_HIPCHK(expr)                      \
    do {                                     \
        hipError_t e__ = (expr);             \
        if (e__ != hipSuccess) {             \
            (void)hipGetLastError();         \
            return NTK_ERR_HIP;              \
        }                                    \
    } while (0)

#include "ntk_device_mem.hpp"

namespace {

constexpr int kThreads = 256;

__host__ __device__ inline uint64_t fmix64(uint64_t x)
{
    x ^= x >> 33; x *= 0xff51afd7ed558ccdull;
    x ^= x >> 33; x *= 0xc4ceb9fe1a85ec53ull;
    x ^= x >> 33;
    return x;
}

__device__ inline uint64_t wave_sum(uint64_t v)
{
    for (int off = 32; off > 0; off >>= 1) v += __shfl_xor(v, off, 64);
    return v;
}

__device__ inline void add_agent(uint64_t *p, uint64_t v)
{
    (void)__hip_atomic_fetch_add(p, v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}

__device__ inline uint32_t block_sum_u32(uint32_t v, uint32_t *lds)
{
    for (int off = 32; off > 0; off >>= 1) v += __shfl_xor(v, off, 64);
    if ((threadIdx.x & 63) == 0) lds[threadIdx.x >> 6] = v;
    __syncthreads();
    uint32_t s = 0;
    for (int w = 0; w < kThreads / 64; w++) s += lds[w];
    return s;
}

// a wave-uniform value, said so
__device__ inline uint64_t uniform(uint64_t v)
{
    const uint32_t lo = __builtin_amdgcn_readfirstlane((uint32_t)v), hi = __builtin_amdgcn_readfirstlane((uint32_t)(v >> 32));
    return ((uint64_t)hi << 32) | lo;
}

// the candidate window ends [lo, hi) of record r of a batch with its n_records + 1 record starts; an offset beyond the batch is read
// as its end
__device__ inline void record_span(const uint64_t *offsets, uint64_t n_bytes, uint32_t k, uint64_t r, uint64_t &lo, uint64_t &hi)
{
    uint64_t b = offsets[r], e = offsets[r + 1];
    if (e > n_bytes) e = n_bytes;
    if (b > e) b = e;
    hi = e ? e - 1 : 0;   // the last byte is the break byte
    lo = b + k - 1;
    if (lo > hi) lo = hi;
}

inline unsigned grid_for(uint64_t items, unsigned block, unsigned cap)
{
    const uint64_t b = (items + block - 1) / block;
    return (unsigned)(b > cap ? cap : (b ? b : 1));
}

int alloc_status(hipError_t e)
{
    (void)hipGetLastError();
    return e == hipErrorOutOfMemory || e == hipErrorMemoryAllocation ? NTK_ERR_NOMEM : NTK_ERR_HIP;
}

// What every handle starts with: the context it works on, that context's device and stream, and the k and path it serves.
struct Consumer {
    ntk_ctx *ctx = nullptr;
    int device = 0, n_cu = 256;
    hipStream_t stream = nullptr;
    uint32_t k = 0, path = 0;

    // the context's device (made current) and stream; no allocation
    int bind(ntk_ctx *c, uint32_t k_, uint32_t path_)
    {
        void *s = nullptr;
        int rc = ntk_ctx_stream(c, &device, &s);
        if (rc) return rc;
        ctx = c; stream = (hipStream_t)s; k = k_; path = path_;
        hipError_t e = hipSetDevice(device);
        if (e == hipSuccess) e = hipDeviceGetAttribute(&n_cu, hipDeviceAttributeMultiprocessorCount, device);
        if (e != hipSuccess) { (void)hipGetLastError(); return NTK_ERR_HIP; }
        return NTK_OK;
    }
};

// The checks of a call that takes a batch, in two parts, since an empty batch is answered NTK_OK between them.  First the handle and
// the params, which must be the handle's ...
inline int check_batch_params(const Consumer *h, const ntk_params *p)
{
    if (!h || !p) return NTK_ERR_BAD_ARG;
    if (p->k != h->k || p->path != h->path || (p->flags & ~0xFF00u) != 0 || p->pre > NTK_PRE_NORMALIZE_IUPAC) return NTK_ERR_BAD_ARG;
    if (p->path == NTK_PATH_BYTES_CANONICAL && p->pre < NTK_PRE_NORMALIZE) return NTK_ERR_UNSUPPORTED;
    return NTK_OK;
}

// ... then the batch's pointers: 16-byte aligned, the quality bytes optional
inline int check_batch_pointers(const uint8_t *d_seq, const uint8_t *d_qual)
{
    return !d_seq || ((uintptr_t)d_seq & 15) || ((uintptr_t)d_qual & 15) ? NTK_ERR_BAD_ARG : NTK_OK;
}

// The quality mask of a batch call, for the kernels that read the quality bytes themselves: the cutoff of the params' flags and the
// bytes it applies to (no cutoff or no bytes: no mask).
template <class Args>
inline void set_quality(Args &a, const ntk_params *p, const uint8_t *d_qual)
{
    a.cutoff = (p->flags >> 8) & 0xFF;
    a.qual = a.cutoff ? d_qual : nullptr;
    if (!a.qual) a.cutoff = 0;
}

// The scratch of one chunk of the core's materialise face (values, valid plane, strand plane: 10 B per base), grown on demand.  Owned by
// whatever consumes that face chunk by chunk.
struct MaterialiseScratch {
    DeviceArray<uint64_t> d_values;
    DeviceArray<uint16_t> d_valid16, d_rc16;

    uint64_t bytes() const { return d_rc16.cap * 16; }   // bases it holds (a multiple of 16)
    uint64_t device_bytes() const { return d_values.bytes() + d_valid16.bytes() + d_rc16.bytes(); }

    void release() { d_values.release(); d_valid16.release(); d_rc16.release(); }

    int ensure(hipStream_t stream, uint64_t len)
    {
        const uint64_t need = (len + 15) & ~(uint64_t)15;
        int rc = d_values.ensure(stream, need, grow_exact);
        if (!rc) rc = d_valid16.ensure(stream, need / 16, grow_exact);
        if (!rc) rc = d_rc16.ensure(stream, need / 16, grow_exact);
        return rc;
    }
};

// The walk over the chunks of a batch of n_bytes > 0: the scratch is grown to the longest chunk, then every chunk is materialised into it
// (the handle's device is current again afterwards) and handed to body(chunk), which queues its work on the scratch before the next
// chunk's replaces it.  The first status that is not NTK_OK ends the walk.
template <class Body>
int for_each_chunk(const Consumer &h, MaterialiseScratch &scratch, const uint8_t *d_seq, const uint8_t *d_qual, uint64_t n_bytes,
                   const ntk_params *p, Body body)
{
    int rc = scratch.ensure(h.stream, chunk_scratch_bases(n_bytes, h.k));
    for (uint64_t start = 0; !rc && start < n_bytes; start += kChunkBases) {
        const Chunk c = chunk_at(n_bytes, h.k, start);
        rc = ntk_materialize_device_quality(h.ctx, d_seq + c.base, d_qual ? d_qual + c.base : nullptr, c.len(), p, scratch.d_values.p,
                                            scratch.d_valid16.p, scratch.d_rc16.p);
        if (rc) return rc;
        CT_HIPCHK(hipSetDevice(h.device));
        rc = body(c);
    }
    return rc;
}

}  // namespace
