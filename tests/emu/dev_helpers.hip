// dev_helpers.hip — TEST-ONLY: the two-faced helpers of needletail_amd/csrc/ntk_tile.hpp (a gfx950 builtin or inline assembly under
// __HIP_DEVICE_COMPILE__, a C restatement for the host emulation of tests/emu/) evaluated element-wise over input arrays, so that
// tests/test_gpu_tile_helpers.py can hold the two sides of every split against each other.  The file is built twice from this one source:
// with hipcc for gfx950 (dh_eval copies the arrays to the device and runs ONE block of 256 threads over them, every access bounds-checked)
// and with g++ (-x c++: the `#else` branches run in a plain loop).  Not part of the product library.
//
// int dh_eval(op, imm, a, b, c, d, out0, out1, out2, n): out*[i] = f(a[i], b[i], c[i], d[i]); 0, -2 unknown op / immediate, -3 n > 65536,
// -100 - e on HIP error e.
#include <stdint.h>
#if defined(__HIPCC__)
#include <hip/hip_runtime.h>   // (before ntk_tile.hpp: NTK_HD needs __forceinline__)
#endif

#include "../../needletail_amd/csrc/ntk_tile.hpp"

using namespace ntk;

enum { DH_BITOP3 = 0, DH_PERM = 1, DH_ALIGNBIT = 2, DH_ADD_SELF = 3, DH_BREV32 = 4, DH_DOT4 = 5, DH_KEY_MIN_F = 6, DH_QUALITY_BREAK = 7,
       DH_LOWER_WATCH = 8, DH_ENCODE16 = 9, DH_ENCODE16_SV2 = 10, DH_KEY_FIELDS_F = 11 };
constexpr uint32_t kDhMaxN = 1u << 16;

struct DhOut { uint32_t o0, o1, o2; };

template <int TT>
NTK_HD DhOut dh_bitop3(uint32_t a, uint32_t b, uint32_t c) { return DhOut{bitop3<TT>(a, b, c), 0u, 0u}; }

// One element.  ok = false: unknown op / immediate (uniform over the call).
NTK_HD DhOut dh_one(int op, uint32_t imm, uint32_t a, uint32_t b, uint32_t c, uint32_t d, bool &ok)
{
    ok = true;
    switch (op) {
    case DH_BITOP3:   // imm = the truth table: every one the headers use
        switch (imm) {
#define DH_TT(T) case T: return dh_bitop3<T>(a, b, c);
        DH_TT(0xCA) DH_TT(0xEA) DH_TT(0xA8) DH_TT(0xE8) DH_TT(0xF2) DH_TT(0xF4) DH_TT(0x35) DH_TT(0xFE)
#undef DH_TT
        default: ok = false; return DhOut{0u, 0u, 0u};
        }
    case DH_PERM: return DhOut{perm(a, b, c), 0u, 0u};                       // (hi, lo, selector)
    case DH_ALIGNBIT: return DhOut{alignbit(a, b, c), 0u, 0u};               // (hi, lo, shift)
    case DH_ADD_SELF: return DhOut{add_self(a), 0u, 0u};
    case DH_BREV32: return DhOut{brev32(a), 0u, 0u};
    case DH_DOT4: return DhOut{dot4(a, b, c), 0u, 0u};
    case DH_KEY_MIN_F: {                                                     // l = (a : b), r = (c : d)
        KeyF l, r;
        l.k = ((uint64_t)a << 32) | b; r.k = ((uint64_t)c << 32) | d;
        const KeyF m = key_min(l, r);
        return DhOut{(uint32_t)(m.k >> 32), (uint32_t)m.k, 0u};
    }
    case DH_QUALITY_BREAK: return DhOut{quality_break(a, b, c, d), 0u, 0u};  // (sequence, quality, add, sel)
    case DH_LOWER_WATCH: return DhOut{lower_watch_or(a, b), 0u, 0u};         // (lc, m)
    case DH_ENCODE16: {                                                      // composites of the helpers above, as the kernels call them
        const Enc e = imm ? encode16<true>(Raw16{a, b, c, d}) : encode16<false>(Raw16{a, b, c, d});
        return DhOut{e.code, e.rcode, e.bad};
    }
    case DH_ENCODE16_SV2: {
        const EncSV2 e = imm ? encode16_sv2<true>(Raw16{a, b, c, d}) : encode16_sv2<false>(Raw16{a, b, c, d});
        return DhOut{e.code, e.rcode, bad16_from_letters(e.ex, e.uu)};
    }
    case DH_KEY_FIELDS_F: {
        KeyF k; k.k = ((uint64_t)a << 32) | b;
        DhOut o;
        key_fields(k, o.o0, o.o1, o.o2);
        return o;
    }
    default: ok = false; return DhOut{0u, 0u, 0u};
    }
}

#if defined(__HIPCC__)

__global__ __launch_bounds__(256) void dh_kernel(int op, uint32_t imm, const uint32_t *a, const uint32_t *b, const uint32_t *c, const uint32_t *d,
                                                 uint32_t *o0, uint32_t *o1, uint32_t *o2, uint32_t n, int *bad)
{
    for (uint32_t i = threadIdx.x; i < n; i += blockDim.x) {   // one block; i < n guards every access
        bool ok;
        const DhOut r = dh_one(op, imm, a[i], b[i], c[i], d[i], ok);
        if (!ok) { if (i == 0) *bad = 1; return; }
        o0[i] = r.o0; o1[i] = r.o1; o2[i] = r.o2;
    }
}

extern "C" int dh_is_device(void) { return 1; }

extern "C" int dh_eval(int op, uint32_t imm, const uint32_t *a, const uint32_t *b, const uint32_t *c, const uint32_t *d, uint32_t *o0, uint32_t *o1,
                       uint32_t *o2, uint32_t n)
{
    if (n > kDhMaxN) return -3;
    if (n == 0) return 0;
    const size_t bytes = (size_t)n * sizeof(uint32_t);
    uint32_t *buf = nullptr;   // 4 inputs, 3 outputs, one flag word
    hipError_t e = hipMalloc((void **)&buf, 7 * bytes + sizeof(int));
    if (e != hipSuccess) return -100 - (int)e;
    const uint32_t *in[4] = {a, b, c, d};
    for (int i = 0; i < 4 && e == hipSuccess; i++) e = hipMemcpy(buf + (size_t)i * n, in[i], bytes, hipMemcpyHostToDevice);
    if (e == hipSuccess) e = hipMemset(buf + (size_t)4 * n, 0, 3 * bytes + sizeof(int));
    int bad = 0;
    if (e == hipSuccess) {
        int *d_bad = (int *)(buf + (size_t)7 * n);
        hipLaunchKernelGGL(dh_kernel, dim3(1), dim3(256), 0, 0, op, imm, buf, buf + n, buf + (size_t)2 * n, buf + (size_t)3 * n, buf + (size_t)4 * n,
                           buf + (size_t)5 * n, buf + (size_t)6 * n, n, d_bad);
        e = hipGetLastError();
        if (e == hipSuccess) e = hipDeviceSynchronize();
        if (e == hipSuccess) e = hipMemcpy(&bad, d_bad, sizeof(int), hipMemcpyDeviceToHost);
    }
    uint32_t *out[3] = {o0, o1, o2};
    for (int i = 0; i < 3 && e == hipSuccess; i++) e = hipMemcpy(out[i], buf + (size_t)(4 + i) * n, bytes, hipMemcpyDeviceToHost);
    (void)hipFree(buf);
    if (e != hipSuccess) return -100 - (int)e;
    return bad ? -2 : 0;
}

#else

extern "C" int dh_is_device(void) { return 0; }

extern "C" int dh_eval(int op, uint32_t imm, const uint32_t *a, const uint32_t *b, const uint32_t *c, const uint32_t *d, uint32_t *o0, uint32_t *o1,
                       uint32_t *o2, uint32_t n)
{
    if (n > kDhMaxN) return -3;
    for (uint32_t i = 0; i < n; i++) {
        bool ok;
        const DhOut r = dh_one(op, imm, a[i], b[i], c[i], d[i], ok);
        if (!ok) return -2;
        o0[i] = r.o0; o1[i] = r.o1; o2[i] = r.o2;
    }
    return 0;
}

#endif
