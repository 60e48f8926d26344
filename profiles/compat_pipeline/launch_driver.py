"""The fixed driver of profiles/compat_pipeline/README.md section 3: the five batched Sequence-trait calls on the record list of
tests/test_gpu_parity.py::test_batched_compat_face_matches_the_iterators_per_record at the default chunk and at 97 and 4096 bytes, then one
call of each with a capacity that is too small (ntk_minimizer_batch has none).  Run it under `rocprofv3 --kernel-trace`; reduce_trace.py
turns the trace into the (kernel, grid, workgroup, LDS) list.  NEEDLETAIL_AMD_LIB selects the build."""
import ctypes as C
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests")]
import needletail_amd as nt  # noqa: E402
from needletail_amd import _lib as L  # noqa: E402
import _compat_scale as CS  # noqa: E402

records = CS.parity_item_records()
long_enough = [r for r in records if len(r) >= 8]
ctx = nt.Context(0)
sums = []
for chunk in (0, 97, 4096):
    ctx.set_option(L.OPT_COMPAT_CHUNK_BYTES, chunk)
    for k in (4, 21):
        counts, pos, flg = nt.canonical_kmers_batch(records, k, ctx)
        sums.append(int(counts.sum()) + int(pos.sum(dtype=np.uint64)) + int(flg.sum()))
        counts, pos, val, flg = nt.bit_kmers_batch(records, k, True, ctx)
        sums.append(int(counts.sum()) + int(val.sum(dtype=np.uint64)))
        sums.append(nt.canonical_kmers_planes(records, k, ctx).total)
        sums.append(nt.bit_kmers_planes(records, k, False, ctx).total)
    mins, pos, flg = nt.minimizer_batch(long_enough, 8, ctx, with_positions=True)
    sums.append(int(np.asarray(pos).sum()) + int(np.asarray(flg).sum()))

# capacities that are too small: every call reports NTK_ERR_CAPACITY (5) and the count it needs
lib = L.lib()
seq = b"".join(records)
n = len(records)
offs = np.zeros(n + 1, dtype=np.uint64)
np.cumsum([len(r) for r in records], out=offs[1:])
for chunk in (0, 97):
    ctx.set_option(L.OPT_COMPAT_CHUNK_BYTES, chunk)
    cap = 100
    cnt, p, v, f, tot = np.zeros(n, dtype=np.uint64), np.zeros(cap, dtype=np.uint64), np.zeros(cap, dtype=np.uint64), np.zeros(cap, dtype=np.uint8), C.c_uint64(0)
    rc = lib.ntk_canonical_kmers_batch(ctx._h, seq, offs.ctypes.data, n, 21, cnt.ctypes.data, p.ctypes.data, f.ctypes.data, cap, C.byref(tot))
    sums += [rc, tot.value, int(cnt.sum())]
    rc = lib.ntk_bit_kmers_batch(ctx._h, seq, offs.ctypes.data, n, 21, 1, cnt.ctypes.data, p.ctypes.data, v.ctypes.data, f.ctypes.data, cap, C.byref(tot))
    sums += [rc, tot.value, int(cnt.sum())]
    rb, v16, r16, vals, nw = np.zeros(n + 1, dtype=np.uint64), np.zeros(4, dtype=np.uint16), np.zeros(4, dtype=np.uint16), np.zeros(64, dtype=np.uint64), C.c_uint64(0)
    rc = lib.ntk_canonical_kmers_batch_planes(ctx._h, seq, offs.ctypes.data, n, 21, rb.ctypes.data, v16.ctypes.data, r16.ctypes.data, 4, C.byref(nw), C.byref(tot))
    sums += [rc, nw.value]
    rc = lib.ntk_bit_kmers_batch_planes(ctx._h, seq, offs.ctypes.data, n, 21, 1, rb.ctypes.data, v16.ctypes.data, r16.ctypes.data, vals.ctypes.data, 4,
                                        C.byref(nw), C.byref(tot))
    sums += [rc, nw.value]
ctx.close()
print("driver results", sums)
