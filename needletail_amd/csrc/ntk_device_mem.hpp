// How a handle owns memory: a device array grown on demand, a pinned stage with its two synchronising round trips, and rocPRIM's
// temporary storage.  Whoever includes it defines CT_HIPCHK and alloc_status first - ntk_consumer.hpp for the libraries on the core's
// ABI, ntk_api.hip for the core, whose versions record the error for ntk_last_hip_error.  The only place under csrc/ that allocates or
// frees (ntk_pinned_alloc hands its memory to the caller and is the exception).  Everything is in an anonymous namespace like the rest
// of the scaffold.  DESIGN.md section 16.
#pragma once

#include <hip/hip_runtime.h>

#include <cstddef>
#include <cstdint>

namespace {

int alloc_status(hipError_t e);

// What an array that has to grow to `need` elements from `have` grows to: a library's choice per array.
using Growth = uint64_t (*)(uint64_t have, uint64_t need);
inline uint64_t grow_exact(uint64_t, uint64_t need) { return need; }
inline uint64_t grow_half_again(uint64_t, uint64_t need) { return need + need / 2 + 64; }
inline uint64_t grow_quarter_again(uint64_t, uint64_t need) { return need + need / 4; }                 // the core's pinned stage
inline uint64_t grow_quarter_again_4k(uint64_t, uint64_t need) { return need + need / 4 + 4096; }       // the core's scratch and banks
inline uint64_t grow_doubling(uint64_t have, uint64_t need)   // from 1024
{
    uint64_t want = have ? have : 1024;
    while (want < need) want *= 2;
    return want;
}

template <class T>
struct DeviceArray {
    T *p = nullptr;
    uint64_t cap = 0;   // elements

    uint64_t bytes() const { return cap * sizeof(T); }

    // once the stream is idle
    void release()
    {
        if (p) (void)hipFree(p);
        p = nullptr; cap = 0;
    }

    // Room for `need` elements; an array that is large enough costs no HIP call.  THE ONE RULE for replacing an array: the stream is
    // synchronised before the old one is freed, since queued kernels may still use it.  keep == 0: the old array is freed before the new
    // one is allocated (the scratch arrays are 8 B per base: both at once would double the peak), and a failure leaves the array empty.
    // keep > 0: the new array is allocated and the first `keep` elements are copied before the old one is freed, and a failure leaves
    // the old array as it was.
    int ensure(hipStream_t stream, uint64_t need, Growth growth, uint64_t keep = 0)
    {
        if (need <= cap) return NTK_OK;
        const uint64_t want = growth(cap, need);
        T *fresh = nullptr;
        if (keep == 0) {
            if (p) CT_HIPCHK(hipStreamSynchronize(stream));
            release();
        }
        const hipError_t e = hipMalloc((void **)&fresh, want * sizeof(T));
        if (e != hipSuccess) return alloc_status(e);
        if (keep) {
            if (hipMemcpyAsync(fresh, p, keep * sizeof(T), hipMemcpyDeviceToDevice, stream) != hipSuccess ||
                hipStreamSynchronize(stream) != hipSuccess) {
                (void)hipGetLastError();
                (void)hipFree(fresh);
                return NTK_ERR_HIP;
            }
            release();
        }
        p = fresh; cap = want;
        return NTK_OK;
    }
};

// Pinned host elements: the stage of a handle's read-backs and small writes.
template <class T>
struct Pinned {
    T *p = nullptr;
    uint64_t cap = 0;   // elements

    uint64_t bytes() const { return cap * sizeof(T); }

    void release()
    {
        if (p) (void)hipHostFree(p);
        p = nullptr; cap = 0;
    }

    // n elements, whatever it held before (the stream is idle)
    int alloc(uint64_t n)
    {
        release();
        const hipError_t e = hipHostMalloc((void **)&p, n * sizeof(T), hipHostMallocDefault);
        if (e != hipSuccess) { p = nullptr; return alloc_status(e); }
        cap = n;
        return NTK_OK;
    }

    // room for `need` elements (the stream is idle); a stage that is large enough costs no HIP call
    int ensure(uint64_t need, Growth growth) { return need <= cap ? NTK_OK : alloc(growth(cap, need)); }

    // n device elements into the stage from element `at` on (synchronises)
    int read(hipStream_t stream, const T *d, uint64_t n, uint64_t at = 0)
    {
        CT_HIPCHK(hipMemcpyAsync(p + at, d, n * sizeof(T), hipMemcpyDeviceToHost, stream));
        CT_HIPCHK(hipStreamSynchronize(stream));
        return NTK_OK;
    }

    // n device elements := the stage's from element `at` on (synchronises: the stage is free again)
    int write(hipStream_t stream, T *d, uint64_t n, uint64_t at = 0)
    {
        CT_HIPCHK(hipMemcpyAsync(d, p + at, n * sizeof(T), hipMemcpyHostToDevice, stream));
        CT_HIPCHK(hipStreamSynchronize(stream));
        return NTK_OK;
    }
};

// run(tmp, bytes): a rocPRIM call; first its size query, then the call on `tmp`, grown by the library's policy to hold what the query
// said (at least one byte)
template <class Run>
int with_tmp(DeviceArray<char> &tmp, hipStream_t stream, Growth growth, Run run)
{
    size_t bytes = 0;
    CT_HIPCHK(run(nullptr, bytes));
    const int rc = tmp.ensure(stream, bytes ? bytes : 1, growth);
    if (rc) return rc;
    CT_HIPCHK(run((void *)tmp.p, bytes));
    return NTK_OK;
}

}  // namespace
