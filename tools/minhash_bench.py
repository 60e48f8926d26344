"""What a MinHash sketch of a device batch costs (include/needletail_amd_minhash.h) beside the k-mer sketch of the same batch.

Workloads: the config-2 batch (10M x 150 bp synthetic reads, byte path after normalize) at k = 21 and k = 51, num = 1000 and
scaled = 1000, default buffer; with --genome also reads sampled error-free from a seeded random 1 Mb genome (every kept hash repeats
about 1500 times); with --host-route a scaled = 1000 sketch of 1M reads against the host route it replaces (materialise on the device,
copy the values to the host, hash and numpy.unique there).

Default mode: the whole add_device call under a host clock that ends in a stream synchronise, KmerSketch and KmerMinHash alternating,
one warm-up pass of each and then --reps repetitions; one JSON line per workload with every repetition, n_merges, n_redone and the time
of the final merge (stats() right after the pass).
--gate KIND: the trace process of the kernel-time gate, for `rocprofv3 --kernel-trace --stats -- python tools/minhash_bench.py --gate
num` (a run of its own): per k, a warm-up pass of each and then one pass of each on the same batch, nothing else."""
import argparse
import json
import os
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))

import needletail_amd as nt  # noqa: E402
from count_bench import genome_reads  # noqa: E402

BYTE_PATH = (nt.PATH_BYTES_CANONICAL, nt.PRE_NORMALIZE)
KINDS = {"num": dict(num=1000), "scaled": dict(scaled=1000)}
XOR = 0x9E3779B97F4A7C15


def clocked(ctx, step) -> float:
    """Milliseconds of a step under the host clock, ending in a stream synchronise."""
    ctx.synchronize()
    t0 = time.perf_counter()
    step()
    ctx.synchronize()
    return (time.perf_counter() - t0) * 1e3


def run(ctx, name, dev, nbytes, k, kind, reps):
    path, pre = BYTE_PATH
    with nt.KmerSketch(k, path, ctx) as sk, nt.KmerMinHash(k, path, ctx=ctx, **kind) as mh:
        rows = {"sketch": [], "minhash": [], "final_merge": []}
        for r in range(reps + 1):   # the first repetition warms up
            sk.reset()
            mh.reset()
            a = clocked(ctx, lambda: sk.add_device(dev, nbytes, pre))
            b = clocked(ctx, lambda: mh.add_device(dev, nbytes, pre))
            c = clocked(ctx, mh.stats)
            if r:
                rows["sketch"].append(round(a, 3)); rows["minhash"].append(round(b, 3)); rows["final_merge"].append(round(c, 3))
        st, est = mh.stats(), sk.estimate()
        h, c = mh.hashes()
    assert st["n_windows"] == est["n_windows"] and np.all(h[1:] > h[:-1])
    out = {"workload": name, "k": k, **kind, "bases": nbytes, "n_windows": st["n_windows"], "n_kept": st["n_kept"],
           "n_merges": st["n_merges"], "n_redone": st["n_redone"], "buffer_entries": st["buffer_entries"],
           "mean_count": round(float(c.mean()), 2) if c.size else 0.0, "max_count": int(c.max()) if c.size else 0}
    for key, v in rows.items():
        out[key + "_ms"] = v
    out["minhash_over_sketch_best"] = round(min(rows["minhash"]) / min(rows["sketch"]), 4)
    return out


def gate(ctx, dev, nbytes, kind):
    path, pre = BYTE_PATH
    for k in (21, 51):
        with nt.KmerSketch(k, path, ctx) as sk, nt.KmerMinHash(k, path, ctx=ctx, **kind) as mh:
            for _ in range(2):   # the warm-up pass of each, then the pass
                sk.reset()
                mh.reset()
                sk.add_device(dev, nbytes, pre)
                mh.add_device(dev, nbytes, pre)
                ctx.synchronize()
            st = mh.stats()
            print(json.dumps({"gate": kind, "k": k, "n_windows": st["n_windows"], "n_kept": st["n_kept"], "n_merges": st["n_merges"],
                              "n_redone": st["n_redone"]}), flush=True)


def fmix64(x):
    x = x.copy()
    with np.errstate(over="ignore"):
        x ^= x >> np.uint64(33); x *= np.uint64(0xff51afd7ed558ccd)
        x ^= x >> np.uint64(33); x *= np.uint64(0xc4ceb9fe1a85ec53)
        x ^= x >> np.uint64(33)
    return x


def host_route(ctx, dev, n_reads, L, k, scaled, reps):
    """The route a user had before: values and valid plane off the device, hash and unique on the host."""
    path, pre = BYTE_PATH
    nbytes = n_reads * (L + 1)
    padded = (nbytes + 15) // 16 * 16
    values = torch.empty(padded, dtype=torch.int64, device="cuda")
    valid = torch.empty(padded // 16, dtype=torch.int16, device="cuda")
    rc = torch.empty(padded // 16, dtype=torch.int16, device="cuda")
    max_hash = np.uint64(((1 << 64) - 1) // scaled)

    def host():
        ctx.materialize_device(dev, nbytes, k, path, pre, values, valid, rc)
        ctx.synchronize()
        v = values.cpu().numpy().view(np.uint64)[:nbytes]
        bits = np.unpackbits(valid.cpu().numpy().view(np.uint16).byteswap().view(np.uint8))[:nbytes].astype(bool)
        h = fmix64(v[bits] ^ np.uint64(XOR))
        return np.unique(h[h <= max_hash], return_counts=True)

    with nt.KmerMinHash(k, path, scaled=scaled, ctx=ctx) as mh:
        rows = {"device": [], "host": []}
        for r in range(reps + 1):
            mh.reset()
            a = clocked(ctx, lambda: (mh.add_device(dev, nbytes, pre), mh.hashes()))
            t0 = time.perf_counter()
            want = host()
            b = (time.perf_counter() - t0) * 1e3
            if r:
                rows["device"].append(round(a, 3)); rows["host"].append(round(b, 3))
        h, c = mh.hashes()
    assert np.array_equal(h, want[0]) and np.array_equal(c, want[1].astype(np.uint64)), "the two routes disagree"
    return {"workload": "host_route", "k": k, "scaled": scaled, "reads": n_reads, "n_kept": int(h.size), "device_ms": rows["device"],
            "host_ms": rows["host"], "host_over_device_best": round(min(rows["host"]) / min(rows["device"]), 1)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--gate", choices=sorted(KINDS), default=None)
    ap.add_argument("--genome", action="store_true")
    ap.add_argument("--host-route", action="store_true")
    ap.add_argument("--reads", type=int, default=10_000_000)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("minhash_bench: no GPU; nothing is measured without one")
    ctx = nt.Context(0, stream=torch.cuda.current_stream().cuda_stream)
    L, n_reads = 150, a.reads
    nbytes = n_reads * (L + 1)
    dev = torch.empty(nbytes + 1024, dtype=torch.uint8, device="cuda")
    ctx.synth_reads_device(0x5EED0002, 0, n_reads, L, 1, dev)
    ctx.synchronize()
    if a.gate:
        gate(ctx, dev, nbytes, KINDS[a.gate])
    else:
        for k in (21, 51):
            for kind in KINDS.values():
                print(json.dumps(run(ctx, "config2", dev, nbytes, k, kind, a.reps)), flush=True)
        if a.host_route:
            print(json.dumps(host_route(ctx, dev, min(n_reads, 1_000_000), L, 21, 1000, 2)), flush=True)
        if a.genome:
            genome_reads(dev, 0x6E0E, 1_000_000, n_reads, L)
            torch.cuda.synchronize()
            for k in (21, 51):
                for kind in KINDS.values():
                    print(json.dumps(run(ctx, "genome", dev, nbytes, k, kind, a.reps)), flush=True)
    ctx.close()


if __name__ == "__main__":
    main()
