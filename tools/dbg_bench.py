#!/usr/bin/env python3
"""Times the de Bruijn graph of a count table's k-mer list (needletail_amd.KmerGraph) on one GPU, in one process, best of `--repeat`
after a warm-up; one JSON line per min_count.

  device   adjacency (edge bytes and totals), unitigs (k-mer rows, unitig rows) and spell (the batch and its offsets) on the
           device-resident list, every result copied back to the host.
  host     the only route there was before: the list on the host, the edge bytes by numpy searchsorted (eight searches), then the
           walk of tests/_dbg_model.py (a dict of strings, one walk per unitig).  The walk is Python: it is timed on a random subsample
           of --walk-keys keys of the list (0: the whole list), and so is the searchsorted part unless --host-full; the line says
           which was used (host_keys).  The device route always runs the whole list.

The list: a k = 21 table of reads of L = 150 sampled from a seeded random genome with substitution errors (the generator of
tools/kmer_sets_bench.py), extracted at min_count 1 and 2.  Defaults: a 22 Mb genome at 30 x, 4.4 M reads.

  python tools/dbg_bench.py [--k 21] [--genome 22000000] [--coverage 30] [--error 0.01] [--repeat 5] [--walk-keys 1000000] [--trace]
--trace runs the device route alone, a warm-up and one pass, for a profiler run of its own.

The gate: the device route on the whole list, copies back included, faster than the host route from host arrays (on its subsample:
a host route that loses on fewer keys loses on all of them)."""
import argparse
import json
import os
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

import needletail_amd as nt  # noqa: E402
from kmer_sets_bench import reads_with_errors, timed, L  # noqa: E402

PATH, PRE = nt.PATH_BYTES_CANONICAL, nt.PRE_NORMALIZE


def host_edges(keys: np.ndarray, k: int) -> np.ndarray:
    """The edge bytes from a host list: numpy, eight searches."""
    mask = np.uint64((1 << (2 * k)) - 1)

    def rc(v):
        out = np.zeros_like(v)
        v = ~v & mask
        for _ in range(k):
            out = (out << np.uint64(2)) | (v & np.uint64(3))
            v = v >> np.uint64(2)
        return out

    edges = np.zeros(keys.size, dtype=np.uint8)
    rk = rc(keys)
    for side, u in enumerate((keys, rk)):
        for c in range(4):
            t = ((u << np.uint64(2)) & mask) | np.uint64(c)
            y = np.minimum(t, rc(t))
            pos = np.searchsorted(keys, y)
            hit = pos < keys.size
            hit[hit] = keys[pos[hit]] == y[hit]
            edges |= (hit.astype(np.uint8) << np.uint8(4 * side + c))
    return edges


def device_route(s):
    with nt.KmerGraph(s) as g:
        edges = g.edges().cpu()
        totals = g.totals()
        u = g.unitigs()
        rows = (u.kmer_rows.cpu(), u.unitig_rows.cpu())
        seq, n_bytes, offsets, n_records = g.unitig_batch()
        out = (seq[:n_bytes].cpu(), offsets.cpu())
        stats = g.stats()
    return edges, totals, u.n_unitigs, u.n_bases, rows, out, stats


def bench(a):
    import _dbg_model as DM
    n_reads = a.genome * a.coverage // L
    with nt.Context(0) as ctx:
        dev, n_bytes = reads_with_errors(0xE441, 0x6E0, a.genome, n_reads, a.error)
        table = nt.KmerTable(a.k, PATH, int(a.genome + n_reads * L * a.error * a.k * 1.1), ctx)
        table.count_device(dev, n_bytes, PRE)
        ctx.synchronize()
        assert table.stats()["n_dropped"] == 0
        del dev
        torch.cuda.empty_cache()
        for min_count in a.min_counts:
            s = nt.KmerSet.from_table(table, min_count)
            n = len(s)
            out = {"k": a.k, "genome": a.genome, "coverage": a.coverage, "error": a.error, "n_reads": n_reads, "min_count": min_count, "n": n,
                   "repeat": a.repeat}
            print(f"min_count {min_count}: {n} k-mers", file=sys.stderr, flush=True)
            edges, totals, n_unitigs, n_bases, rows, batch, stats = device_route(s)   # the warm-up
            if a.trace:
                device_route(s)
                print(json.dumps({"trace": True, **out}), flush=True)
                continue
            out.update(n_unitigs=n_unitigs, n_bases=n_bases, n_rounds=stats["n_rounds"], device_bytes=stats["device_bytes"],
                       n_launches=stats["n_launches"], **{key: v for key, v in totals.items() if key != "deg_hist"})
            out["n_cycles"] = int((rows[1][:, 3] & 1).sum())
            out["longest_unitig_kmers"] = int(rows[1][:, 1].max()) if n_unitigs else 0
            ts = [timed(lambda: device_route(s))[0] for _ in range(a.repeat)]
            out["device_ms"], out["device_ms_all"] = round(min(ts), 3), [round(t, 3) for t in ts]
            # the parts, each with its copies back, on a graph of their own
            parts = {"adjacency": [], "unitigs": [], "spell": []}
            for _ in range(a.repeat):
                with nt.KmerGraph(s) as g:
                    parts["adjacency"].append(timed(lambda: (g.edges().cpu(), g.totals()))[0])
                    parts["unitigs"].append(timed(lambda: [t.cpu() for t in list(g.unitigs())[:2]])[0])
                    parts["spell"].append(timed(lambda: [t.cpu() for t in g.unitig_batch()[0:3:2]])[0])
            for name, v in parts.items():
                out[name + "_ms"] = round(min(v), 3)
            # bytes the kernels move, from the array sizes: per k-mer 8 + 1 + 8 for the edge bytes and targets and
            # about 8 * 3 * 8 of searches; per state and round 12 read in order, 12 gathered, 12 written
            out["rank_bytes"] = 2 * n * 36 * stats["n_rounds"]
            out["rank_bytes_over_unitigs_call_of_8_tb_per_s"] = round(out["rank_bytes"] / (out["unitigs_ms"] * 1e-3) / 8e12, 4)
            # the host route
            keys, counts = s.items()
            host_keys = keys
            if a.walk_keys and a.walk_keys < n:
                pick = np.sort(np.random.default_rng(1).choice(n, a.walk_keys, replace=False))
                host_keys = keys[pick]
            ms_edges, h_edges = timed(lambda: host_edges(keys if a.host_full else host_keys, a.k))
            if a.host_full or host_keys is keys:
                assert np.array_equal(h_edges, edges.numpy()), "the host edge bytes are the device's"
            ms_walk, model = timed(lambda: DM.Graph(host_keys, np.ones(host_keys.size, dtype=np.uint64), a.k))
            if host_keys is keys:
                assert np.array_equal(model.unitig_rows[:, :2], rows[1].numpy().view(np.uint64)[:, :2])
            out.update(host_keys=int(host_keys.size), host_edges_keys=int(keys.size if a.host_full else host_keys.size),
                       host_edges_ms=round(ms_edges, 1), host_walk_ms=round(ms_walk, 1), host_ms=round(ms_edges + ms_walk, 1))
            out["host_over_device"] = round(out["host_ms"] / out["device_ms"], 2)
            out["gate"] = bool(out["device_ms"] < out["host_ms"])
            print(json.dumps(out), flush=True)
            s.close()
        table.close()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--k", type=int, default=21)
    ap.add_argument("--genome", type=int, default=22_000_000)
    ap.add_argument("--coverage", type=int, default=30)
    ap.add_argument("--error", type=float, default=0.01)
    ap.add_argument("--repeat", type=int, default=5)
    ap.add_argument("--walk-keys", type=int, default=1_000_000)
    ap.add_argument("--host-full", action="store_true")
    ap.add_argument("--min-counts", type=int, nargs="+", default=[1, 2])
    ap.add_argument("--trace", action="store_true")
    bench(ap.parse_args())


if __name__ == "__main__":
    main()
