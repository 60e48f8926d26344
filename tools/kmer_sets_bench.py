#!/usr/bin/env python3
"""Times the exact k-mer set algebra (needletail_amd.KmerSet) against the only route there was before it, on one GPU, in one process,
the routes alternated, best of `--repeat` after a warm-up; one JSON line per workload.

  device   compare(bins 256 x 8) and union(SUM) on two device-resident lists, their results copied back (the histogram and totals;
           the union's keys and counts).  Also timed: the two from_table extracts that feed them, and union without the copy back.
  host     the parent's route: items() of both tables to the host, then numpy: searchsorted for the join, add.at for the joint
           histogram, concatenate + argsort for the union.  Timed once with the two items() included and once from host arrays
           (--host-repeat times; it is seconds long at size).

Inputs: two tables of reads sampled from one seeded random genome (the method of tools/count_bench.py's generator) with substitution
errors, so that most distinct k-mers are error k-mers seen once; the two read sets are drawn independently, so they share the genome's
k-mers and nearly none of the errors'.  --genome and --coverage size them; the defaults (a 22 Mb genome, 30 x) give 1.03 x 10^8
distinct k-mers per table at k = 21; --genome 15000000 gives 1.01 x 10^8 at k = 41.
--k 41 runs the wide tables (the host route is narrow-only: numpy has no two-word key).

  python tools/kmer_sets_bench.py [--k 21] [--genome 22000000] [--coverage 30] [--error 0.01] [--repeat 5] [--host-repeat 1] [--trace]
--trace runs the device route alone (extracts, compare, union), a warm-up and one pass, for a profiler run of its own.

The gate: compare and union(SUM) from device-resident lists, copy back included, faster than the host route from host arrays."""
import argparse
import json
import os
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import needletail_amd as nt  # noqa: E402

L = 150
PATH, PRE = nt.PATH_BYTES_CANONICAL, nt.PRE_NORMALIZE
BINS = (256, 8)


def reads_with_errors(seed: int, genome_seed: int, genome_len: int, n_reads: int, error: float):
    """A device batch of n_reads reads of L bases sampled from the seeded random genome (the method of tools/count_bench.py's
    genome_reads; the read starts and the errors are the set's own), every base replaced by a random one with probability `error`
    (a quarter of those replacements restore the base), one break byte behind each read."""
    n_bytes = n_reads * (L + 1)
    dev = torch.full(((n_bytes + 15) // 16 * 16 + 64,), ord("\n"), dtype=torch.uint8, device="cuda")
    g = torch.Generator(device="cuda")
    g.manual_seed(genome_seed)
    acgt = torch.tensor(list(b"ACGT"), dtype=torch.uint8, device="cuda")
    genome = acgt[torch.randint(0, 4, (genome_len,), generator=g, device="cuda")]
    g.manual_seed(seed)
    view = dev[:n_bytes].view(n_reads, L + 1)
    off = torch.arange(L, device="cuda")
    for lo in range(0, n_reads, 1_000_000):
        hi = min(n_reads, lo + 1_000_000)
        starts = torch.randint(0, genome_len - L + 1, (hi - lo,), generator=g, device="cuda")
        hit = torch.rand((hi - lo, L), generator=g, device="cuda") < error
        sub = acgt[torch.randint(0, 4, (hi - lo, L), generator=g, device="cuda")]
        view[lo:hi, :L] = torch.where(hit, sub, genome[starts[:, None] + off])
    torch.cuda.synchronize()
    return dev, n_bytes


def timed(fn):
    torch.cuda.synchronize()
    t = time.perf_counter()
    out = fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t) * 1e3, out


def host_join(a, ca, b, cb):
    """The parent's route from host arrays (narrow keys): the joint histogram with the totals it needs, and union(SUM)."""
    pos = np.searchsorted(b, a)
    hit = pos < b.size
    hit[hit] = b[pos[hit]] == a[hit]
    twin = np.zeros(a.size, dtype=np.uint64)
    twin[hit] = cb[pos[hit]]
    only_b = np.ones(b.size, dtype=bool)
    only_b[pos[hit]] = False
    hist = np.zeros(BINS, dtype=np.uint64)
    np.add.at(hist, (np.minimum(ca, BINS[0] - 1).astype(np.int64), np.minimum(twin, BINS[1] - 1).astype(np.int64)), 1)
    np.add.at(hist, (np.zeros(int(only_b.sum()), dtype=np.int64), np.minimum(cb[only_b], BINS[1] - 1).astype(np.int64)), 1)
    totals = {"n_shared": int(hit.sum()), "sum_a": int(ca.sum()), "sum_b": int(cb.sum()), "sum_min": int(np.minimum(ca[hit], twin[hit]).sum())}
    keys = np.concatenate([a, b[only_b]])
    s = ca + twin
    s[s < ca] = np.uint64((1 << 64) - 1)
    counts = np.concatenate([s, cb[only_b]])
    order = np.argsort(keys, kind="stable")
    return hist, totals, keys[order], counts[order]


def bench(a):
    table = nt.KmerTable if a.k <= 32 else nt.WideKmerTable
    kw = 1 if a.k <= 32 else 2
    n_reads = a.genome * a.coverage // L
    out = {"k": a.k, "genome": a.genome, "coverage": a.coverage, "error": a.error, "n_reads": n_reads, "repeat": a.repeat}
    with nt.Context(0) as ctx:
        tables = []
        for seed in (1, 2):
            dev, n_bytes = reads_with_errors(0xE440 + seed, 0x6E0, a.genome, n_reads, a.error)
            t = table(a.k, PATH, int(a.genome + n_reads * L * a.error * a.k * 1.1), ctx)
            t.count_device(dev, n_bytes, PRE)
            ctx.synchronize()
            assert t.stats()["n_dropped"] == 0
            tables.append(t)
            del dev
        torch.cuda.empty_cache()

        def extracts():
            return nt.KmerSet.from_table(tables[0]), nt.KmerSet.from_table(tables[1])

        sa, sb = extracts()
        out.update(n_a=len(sa), n_b=len(sb))
        print(f"tables counted and extracted: {len(sa)} and {len(sb)} distinct k-mers", file=sys.stderr, flush=True)

        def compare():
            return sa.compare(sb, *BINS)

        def union_device():
            return sa.union(sb, "sum")

        def union():
            u = sa.union(sb, "sum")
            return u.items()

        if a.trace:
            for _ in range(2):
                x, y = extracts()
                x.compare(y, *BINS)
                x.union(y, "sum").close()
                x.close(), y.close()
            print(json.dumps({"trace": True, **out}), flush=True)
            return
        hist, totals = compare()
        u_keys, u_counts = union()
        out.update(n_shared=totals["n_shared"], n_union=int(u_counts.size), hist_1_0=int(hist[1, 0]))
        if kw == 1:   # the host route, checked against the device route before anything is timed
            host = [t.items() for t in tables]
            h_hist, h_totals, h_keys, h_counts = host_join(host[0][0], host[0][1], host[1][0], host[1][1])
            assert np.array_equal(h_hist, hist) and all(totals[name] == v for name, v in h_totals.items())
            assert np.array_equal(h_keys, u_keys) and np.array_equal(h_counts, u_counts)
            del h_keys, h_counts
            print("the host route agrees with the device route", file=sys.stderr, flush=True)
        del u_keys, u_counts
        times = {"compare": [], "union": [], "union_device": [], "extracts": [], "host_arrays": [], "host_with_items": []}
        for r in range(a.repeat):
            times["compare"].append(timed(compare)[0])
            times["union"].append(timed(union)[0])
            ms, u = timed(union_device)
            times["union_device"].append(ms)
            u.close()
            del u
            ms, pair = timed(extracts)
            times["extracts"].append(ms)
            for s in pair:
                s.close()
            del pair
            print(f"repetition {r}: compare {times['compare'][-1]:.2f} ms, union {times['union'][-1]:.2f} ms", file=sys.stderr, flush=True)
            if kw == 1 and r < a.host_repeat:
                times["host_arrays"].append(timed(lambda: host_join(host[0][0], host[0][1], host[1][0], host[1][1]))[0])
                ms, items = timed(lambda: [t.items() for t in tables])
                times["host_with_items"].append(ms + times["host_arrays"][-1])
                del items
        for route, ts in times.items():
            if ts:
                out[route + "_ms"] = round(min(ts), 3)
                out[route + "_ms_all"] = [round(t, 3) for t in ts]
        entry = kw * 8 + 8
        moved = {"compare": (len(sa) + len(sb)) * entry, "union_device": (len(sa) + len(sb) + out["n_union"]) * entry}
        for route, nbytes in moved.items():
            out[route + "_bytes"] = nbytes
            out[route + "_tb_per_s"] = round(nbytes / out[route + "_ms"] / 1e9, 4)
            out[route + "_of_8_tb_per_s"] = round(nbytes / out[route + "_ms"] / 1e9 / 8.0, 4)
        if kw == 1:
            out["host_over_device"] = round(out["host_arrays_ms"] / (out["compare_ms"] + out["union_ms"]), 2)
            out["gate"] = bool(out["compare_ms"] + out["union_ms"] < out["host_arrays_ms"])
        out["stats"] = sa.stats()
        print(json.dumps(out), flush=True)
        for s in (sa, sb):
            s.close()
        for t in tables:
            t.close()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--k", type=int, default=21)
    ap.add_argument("--genome", type=int, default=22_000_000)
    ap.add_argument("--coverage", type=int, default=30)
    ap.add_argument("--error", type=float, default=0.01)
    ap.add_argument("--repeat", type=int, default=5)
    ap.add_argument("--host-repeat", type=int, default=1)
    ap.add_argument("--trace", action="store_true")
    bench(ap.parse_args())


if __name__ == "__main__":
    main()
