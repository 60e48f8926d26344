#!/usr/bin/env python3
"""Times the per-record MinHash call (needletail_amd.RecordMinHash) against the two routes there were before it, on one GPU, in one
process, the routes alternated, best of `--repeat` after a warm-up; one JSON line per workload and kind.

  new      RecordMinHash.run_device on the whole batch, then sketches() (the CSR on the host); run_device alone is reported too
  loop     one KmerMinHash, per record reset / add_records / hashes: the only route to the same result before.  It is timed on the
           first --loop-records records and scaled to all of them (it is linear in the records: each pays its own upload, launch
           ladder, merge and read); the sample's sketches are checked against the new route's
  single   one KmerMinHash.add_device over the whole batch as ONE sketch, then hashes(): what hashing and filtering the same bases
           costs with no per-record work

Workloads (k = 21, random bases made on the device, every record followed by its break byte):
  A  4096 records x 100 kb        B  100 000 records x 10 kb
Kinds: num = 1000 and scaled = 1000.

  python tools/record_minhash_bench.py [--workload A|B|all] [--repeat 5] [--loop-records 256] [--trace A:num]
--trace runs the new route alone, a warm-up and one call, for a profiler run of its own."""
import argparse
import json
import os
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import needletail_amd as nt  # noqa: E402

K = 21
WORKLOADS = {"A": (4096, 100_000), "B": (100_000, 10_000)}
KINDS = {"num": dict(num=1000), "scaled": dict(scaled=1000)}
PATH, PRE = nt.PATH_BYTES_CANONICAL, nt.PRE_NORMALIZE


def make_batch(n_records: int, length: int, seed: int):
    """(device batch, n_bytes, device offsets): random ACGT records, one break byte behind each."""
    g = torch.Generator(device="cuda")
    g.manual_seed(seed)
    n_bytes = n_records * (length + 1)
    dev = torch.full(((n_bytes + 15) // 16 * 16 + 64,), ord("\n"), dtype=torch.uint8, device="cuda")
    rows = dev[:n_bytes].view(n_records, length + 1)
    lut = torch.tensor(list(b"ACGT"), dtype=torch.uint8, device="cuda")
    for r0 in range(0, n_records, 1024):   # in pieces: the int64 indices of one piece stay small
        r1 = min(n_records, r0 + 1024)
        rows[r0:r1, :length] = lut[torch.randint(0, 4, (r1 - r0, length), generator=g, device="cuda")]
    off = torch.arange(n_records + 1, dtype=torch.int64, device="cuda") * (length + 1)
    torch.cuda.synchronize()
    return dev, n_bytes, off


def timed(fn):
    torch.cuda.synchronize()
    t = time.perf_counter()
    out = fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t) * 1e3, out


def bench(name: str, kind: str, repeat: int, loop_records: int, ctx) -> dict:
    n_records, length = WORKLOADS[name]
    dev, n_bytes, off = make_batch(n_records, length, 0xBE7C + n_records)
    sample = min(loop_records, n_records)
    host = dev[:sample * (length + 1)].cpu().numpy().reshape(sample, length + 1)[:, :length]
    records = [row.tobytes() for row in host]
    out = {"workload": name, "kind": kind, "k": K, "n_records": n_records, "record_bases": length, "n_bytes": n_bytes,
           "loop_records": sample}
    with nt.RecordMinHash(K, PATH, ctx=ctx, **KINDS[kind]) as rmh, nt.KmerMinHash(K, PATH, ctx=ctx, **KINDS[kind]) as mh:
        def new():
            rmh.run_device(dev, n_bytes, off, n_records, PRE)
            return rmh.sketches()

        def loop():
            got = []
            for r in records:
                mh.reset()
                mh.add_records([r], PRE)
                got.append(mh.hashes())
            return got

        def single():
            mh.reset()
            mh.add_device(dev, n_bytes, PRE)
            return mh.hashes()

        # warm-up, and the check of the sample before anything is timed
        offsets, windows, hashes, counts = new()
        for r, (h, c) in enumerate(loop()):
            lo, hi = int(offsets[r]), int(offsets[r + 1])
            assert np.array_equal(hashes[lo:hi], h) and np.array_equal(counts[lo:hi], c), (name, kind, r)
        single()
        assert int(windows.sum()) == n_records * (length - K + 1)
        times = {"new": [], "run_device": [], "loop": [], "single": []}
        for _ in range(repeat):
            times["new"].append(timed(new)[0])
            times["run_device"].append(timed(lambda: rmh.run_device(dev, n_bytes, off, n_records, PRE))[0])
            times["loop"].append(timed(loop)[0] * n_records / sample)
            times["single"].append(timed(single)[0])
        for route, ts in times.items():
            out[route + "_ms"] = round(min(ts), 3)
            out[route + "_ms_all"] = [round(t, 3) for t in ts]
        st = rmh.stats()
        out.update({key: st[key] for key in ("n_entries", "n_rounds", "n_retried_records", "n_redone", "device_bytes", "buffer_entries")})
        out["gate_loop"] = bool(out["new_ms"] < out["loop_ms"])
        out["new_over_single"] = round(out["new_ms"] / out["single_ms"], 3)
        out["run_device_over_single"] = round(out["run_device_ms"] / out["single_ms"], 3)
    return out


def trace(name: str, kind: str, ctx):
    n_records, length = WORKLOADS[name]
    dev, n_bytes, off = make_batch(n_records, length, 0xBE7C + n_records)
    with nt.RecordMinHash(K, PATH, ctx=ctx, **KINDS[kind]) as rmh:
        for _ in range(2):
            rmh.run_device(dev, n_bytes, off, n_records, PRE)
        print(json.dumps({"trace": f"{name}:{kind}", **rmh.stats()}), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--workload", default="all", choices=["A", "B", "all"])
    ap.add_argument("--repeat", type=int, default=5)
    ap.add_argument("--loop-records", type=int, default=256)
    ap.add_argument("--trace", default=None, help="WORKLOAD:KIND, e.g. A:num")
    a = ap.parse_args()
    with nt.Context(0) as ctx:
        if a.trace:
            trace(*a.trace.split(":"), ctx)
            return
        for name in (("A", "B") if a.workload == "all" else (a.workload,)):
            for kind in KINDS:
                print(json.dumps(bench(name, kind, a.repeat, a.loop_records, ctx)), flush=True)


if __name__ == "__main__":
    main()
