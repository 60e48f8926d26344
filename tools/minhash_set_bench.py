"""What the all-pairs comparison of a set of MinHash sketches costs on the device (include/needletail_amd_minhash_set.h) beside the
only route there was before: ntk_minhash_compare pair by pair on one host thread.

Workloads (synthetic sorted hashes, seeded; a quarter of every sketch is drawn from a core all sketches share):
  a        4096 bottom-1000 sketches, no counts: the full matrix (n_shared, n_union; num = 1000), and one row against all
  b        the same with counts, all five outputs (the second pass for norm2_b included)
  c        512 scaled sketches of about 50 000 hashes: the path beyond the LDS stage (num = 0, n_shared and n_union)
  stage    1024 sketches of exactly STAGE hashes against 1024 of STAGE + 1: the same template searching LDS and global memory

Before anything is timed, 4096 sampled pairs of each workload are checked against minhashing.compare.  Then: one warm-up call and the best
of --reps calls under a host clock around the raw C call (which synchronises), outputs preallocated.  The host route is timed in the same
process on --host-pairs sampled pairs of the same workload through the raw C call and scaled to all pairs; the cost of the bare foreign
call (the same number of calls on empty sketches) is reported beside it and subtracted.  One JSON line per measurement.

--trace W: the process for `rocprofv3 --kernel-trace --stats -- python tools/minhash_set_bench.py --trace a` (a run of its own): the set
of workload W, one warm-up compare and one compare, nothing else."""
import argparse
import ctypes as C
import json
import os
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import needletail_amd as nt  # noqa: E402
from needletail_amd import minhash_sets, minhashing  # noqa: E402

ALL = (1 << 64) - 1
WORKLOADS = {
    "a": dict(n=4096, length=1000, abundance=False, num=1000, want=("n_shared", "n_union")),
    "b": dict(n=4096, length=1000, abundance=True, num=1000, want=minhash_sets.MATRICES),
    "c": dict(n=512, length=50000, abundance=False, num=0, want=("n_shared", "n_union")),
}


def synth(seed, n, length, shared=0.25, jitter=0):
    """n sketches of `length` hashes (minus up to `jitter`): a `shared` part picked from a core of twice that size, the rest its own."""
    rng = np.random.default_rng(seed)
    m = int(length * shared)
    core = np.unique(rng.integers(0, 1 << 64, 2 * m + 8, dtype=np.uint64))[:2 * m]
    out = []
    for _ in range(n):
        size = length - (int(rng.integers(0, jitter + 1)) if jitter else 0)
        own = rng.integers(0, 1 << 64, size - m, dtype=np.uint64)
        h = np.unique(np.concatenate([own, rng.choice(core, m, replace=False)]))
        while h.size < size:   # a collision among 64-bit values: all but impossible
            h = np.unique(np.concatenate([h, rng.integers(0, 1 << 64, size - h.size, dtype=np.uint64)]))
        out.append((h, rng.integers(1, 1 << 16, h.size, dtype=np.uint64)))
    return out


def fill(ctx, sketches, abundance):
    s = nt.MinHashSet(abundance, ctx)
    for h, c in sketches:
        s.add((h, c if abundance else None))
    return s


class Outputs:
    """Preallocated outputs of one compare and the raw call on them."""

    def __init__(self, rows, nr, cols, nc, num, want):
        self.rows, self.cols, self.nr, self.nc, self.num = rows, cols, nr, nc, num
        self.m = {name: np.zeros((nr, nc), dtype=minhash_sets._DTYPES[name]) for name in want}
        self.n_a, self.n_b = np.zeros(nr, dtype=np.uint64), np.zeros(nc, dtype=np.uint64)
        self.args = [self.m[name].ctypes.data if name in self.m else None for name in minhash_sets.MATRICES]

    def run(self, r0=0, c0=0):
        rc = minhash_sets.lib().ntk_mhset_compare(self.rows._h, r0, self.nr, self.cols._h, c0, self.nc, self.num, ALL, *self.args,
                                                  self.n_a.ctypes.data, self.n_b.ctypes.data)
        if rc:
            raise nt.NtkError(rc, "ntk_mhset_compare")


def best_ms(step, reps):
    step()   # warm-up
    times = []
    for _ in range(reps):
        t0 = time.perf_counter()
        step()
        times.append((time.perf_counter() - t0) * 1e3)
    return min(times), [round(t, 3) for t in times]


def check_sample(out, rows_sk, cols_sk, abundance, seed, n=4096):
    rng = np.random.default_rng(seed)
    for r, c in zip(rng.integers(0, out.nr, n), rng.integers(0, out.nc, n)):
        (a, ca), (b, cb) = rows_sk[r], cols_sk[c]
        want = minhashing.compare(a, ca if abundance else None, b, cb if abundance else None, out.num, ALL)
        for name, m in out.m.items():
            assert m[r, c] == want[name], (name, r, c, m[r, c], want[name])
        assert out.n_a[r] == want["n_a"] and out.n_b[c] == want["n_b"]


def host_route(rows_sk, cols_sk, abundance, num, n_pairs, seed):
    """ntk_minhash_compare on n_pairs sampled pairs, one thread: (ms for them, ms of as many calls on empty sketches)."""
    lib, out = minhashing.lib(), minhashing.Comparison()
    rng = np.random.default_rng(seed)
    pairs = []
    for r, c in zip(rng.integers(0, len(rows_sk), n_pairs), rng.integers(0, len(cols_sk), n_pairs)):
        (a, ca), (b, cb) = rows_sk[r], cols_sk[c]
        pairs.append((a.ctypes.data, ca.ctypes.data if abundance else None, a.size, b.ctypes.data, cb.ctypes.data if abundance else None, b.size))
    ref, fn = C.byref(out), lib.ntk_minhash_compare
    t0 = time.perf_counter()
    for pa, pca, na, pb, pcb, nb in pairs:
        fn(pa, pca, na, pb, pcb, nb, num, ALL, ref)
    t1 = time.perf_counter()
    for pa, pca, na, pb, pcb, nb in pairs:
        fn(pa, pca, 0, pb, pcb, 0, num, ALL, ref)
    t2 = time.perf_counter()
    return (t1 - t0) * 1e3, (t2 - t1) * 1e3


def copy_ms(n_bytes, reps=5):
    """A device-to-pinned-host copy of n_bytes, best of reps: what the copy back of that many result bytes costs on its own."""
    src, dst = torch.empty(n_bytes, dtype=torch.uint8, device="cuda"), torch.empty(n_bytes, dtype=torch.uint8).pin_memory()
    times = []
    for _ in range(reps + 1):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        dst.copy_(src, non_blocking=True)
        torch.cuda.synchronize()
        times.append((time.perf_counter() - t0) * 1e3)
    return min(times[1:])


def emit(**row):
    print(json.dumps(row), flush=True)


def run_workload(ctx, name, w, reps, host_pairs):
    sk = synth(0x5E70 + ord(name), w["n"], w["length"], jitter=w["length"] // 20 if name == "c" else 0)
    lengths = np.array([h.size for h, _ in sk], dtype=np.float64)
    n = w["n"]
    with fill(ctx, sk, w["abundance"]) as s:
        full = Outputs(s, n, s, n, w["num"], w["want"])
        full.run()
        check_sample(full, sk, sk, w["abundance"], 1)
        launches = s.stats()["n_launches"]
        best, times = best_ms(full.run, reps)
        steps = 2.0 * n * lengths.sum()   # the sum of |A| + |B| over all pairs
        host_ms, call_ms = host_route(sk, sk, w["abundance"], w["num"], host_pairs, 2)
        host_all = (host_ms - call_ms) * (n * n / host_pairs)
        result_bytes = n * n * (32 if "norm2_b" in w["want"] else 8)
        emit(workload=name, what="full matrix", n=n, mean_length=round(float(lengths.mean()), 1), abundance=w["abundance"], num=w["num"],
             outputs=list(w["want"]), pairs=n * n, launches_per_call=launches, whole_call_ms=round(best, 3), all_ms=times,
             pairs_per_s=round(n * n / best * 1e3), merge_steps_per_s=round(steps / best * 1e3),
             copy_alone_ms=round(copy_ms(result_bytes), 3), result_bytes=result_bytes,
             host_pairs=host_pairs, host_ms=round(host_ms, 3), host_bare_calls_ms=round(call_ms, 3), host_all_pairs_ms=round(host_all, 1),
             host_over_16_ms=round(host_all / 16, 1), gate_ratio=round(host_all / 16 / best, 2), gate_met=bool(best < host_all / 16),
             device_bytes=s.stats()["device_bytes"])
        if name == "a":
            row = Outputs(s, 1, s, n, w["num"], w["want"])
            row.run(r0=7)
            check_sample(row, sk[7:8], sk, w["abundance"], 3, n=512)
            best, times = best_ms(lambda: row.run(r0=7), reps)
            emit(workload=name, what="one row against all", pairs=n, whole_call_ms=round(best, 3), all_ms=times, pairs_per_s=round(n / best * 1e3))


def run_stage(ctx, reps):
    """The two paths of the one template: columns of exactly STAGE hashes are searched in LDS, of STAGE + 1 in global memory."""
    L = minhash_sets.STAGE
    rows = synth(0x5E80, 1024, 1000)
    for length in (L, L + 1):
        cols = synth(0x5E81, 1024, length)
        with fill(ctx, rows, False) as r, fill(ctx, cols, False) as c:
            out = Outputs(r, 1024, c, 1024, 0, ("n_shared", "n_union"))
            out.run()
            check_sample(out, rows, cols, False, 4, n=1024)
            best, times = best_ms(out.run, reps)
            emit(workload="stage", column_length=length, path="LDS" if length <= L else "global", pairs=1 << 20, whole_call_ms=round(best, 3),
                 all_ms=times, pairs_per_s=round((1 << 20) / best * 1e3))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--host-pairs", type=int, default=1 << 16)
    ap.add_argument("--only", default="a,b,c,stage")
    ap.add_argument("--trace", choices=sorted(WORKLOADS), default=None)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("minhash_set_bench: no GPU; nothing is measured without one")
    ctx = nt.Context(0, stream=torch.cuda.current_stream().cuda_stream)
    if a.trace:
        w = WORKLOADS[a.trace]
        sk = synth(0x5E70 + ord(a.trace), w["n"], w["length"], jitter=w["length"] // 20 if a.trace == "c" else 0)
        with fill(ctx, sk, w["abundance"]) as s:
            out = Outputs(s, w["n"], s, w["n"], w["num"], w["want"])
            out.run()
            out.run()
            emit(trace=a.trace, n_launches=s.stats()["n_launches"])
    else:
        for name in a.only.split(","):
            if name == "stage":
                run_stage(ctx, a.reps)
            else:
                run_workload(ctx, name, WORKLOADS[name], a.reps, a.host_pairs)
    ctx.close()


if __name__ == "__main__":
    main()
