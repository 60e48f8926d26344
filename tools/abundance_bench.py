"""What the per-read abundance call costs (include/needletail_amd_abundance.h): the whole run_device call on the host clock (the call
ends synchronised), warmed up, several repetitions with their spread.

  (a) config2:   the config-2 batch (10 M x 150 bp synthetic reads, byte path after normalize) at k = 21, against a table counted from the
                 same batch and sized by the sketch;
  (b) config3:   config 3's shape (10 kb contigs, k = 31, bit-packed canonical path after strip_returns), likewise against its own
                 table.  --contigs (default 100 000, a tenth of config 3): the table of the full 10 G nearly all-distinct 31-mers would need
                 2^34 slots of 16 B, more than the device holds;
  (c) genome:    10 M x 150 bp reads sampled error-free from a seeded random 1 Mb genome (tools/count_bench.py's), k = 21, against their
                 own table: ~1 300x coverage, so the counts differ inside nearly every read and the median selection runs its passes
                 (the synthetic reads of (a) and (b) are nearly all distinct: every count is 1 and min == max ends the selection);
  (d) single70m: one record of 75.5 M bases (a 2 000-base genome read round and round) between two short ones, against a table of that
                 genome: the record goes through ra_block_kernel alone.

Prints one JSON line per workload.  --quick: one repetition, for a kernel-trace run
(rocprofv3 --kernel-trace --stats -- python tools/abundance_bench.py --quick --only config2 config3 genome), whose per-kernel totals give the
gate: the ra_* kernels together take no longer than kt_lookup_kernel over the same run."""
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


def offsets_of_equal_records(n_records, record_len):
    return torch.arange(n_records + 1, dtype=torch.int64, device="cuda") * (record_len + 1)


def run(ctx, name, dev, nbytes, d_off, n_records, k, path, pre, reps, min_count=3, table_bytes=None):
    """table_bytes: count only the batch's first bytes into the table (default: all of it)."""
    counted = nbytes if table_bytes is None else table_bytes
    with nt.KmerSketch(k, path, ctx) as sk:
        sk.add_device(dev, counted, pre)
        est = sk.estimate()
        with sk.table() as t, nt.ReadAbundance(t) as ra:
            t.count_device(dev, counted, pre)
            st = t.stats()
            assert st["n_dropped"] == 0
            ms, rows = [], None
            for r in range(reps + 1):   # the first repetition warms up (and allocates the scratch)
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                rows = ra.run_device(dev, nbytes, d_off, n_records, pre, min_count=min_count)
                dt = (time.perf_counter() - t0) * 1e3
                if r:
                    ms.append(dt)
            # what came back, as a plausibility check of the run itself (the tests hold the rows to the oracle)
            n_kmers, present = int(rows[:, 0].sum()), int(rows[:, 1].sum())
            assert n_kmers == est["n_windows"] if table_bytes is None else n_kmers > 0
            head = rows[: min(n_records, 3)].cpu().numpy().view(np.uint64).tolist()
    best = min(ms)
    return {"workload": name, "k": k, "bases": nbytes, "n_records": n_records, "n_kmers": n_kmers, "n_present": present,
            "min_count": min_count, "n_distinct": st["n_distinct"], "slots": st["slots"],
            "run_device_ms": round(best, 3), "run_device_all_ms": [round(v, 3) for v in ms],
            "spread": round((max(ms) - best) / best, 4), "gbases_per_s": round(nbytes / best / 1e6, 2), "first_rows": head}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--quick", action="store_true")
    ap.add_argument("--only", nargs="+", choices=["config2", "config3", "genome", "single70m"], default=None)
    ap.add_argument("--contigs", type=int, default=100_000)
    a = ap.parse_args()
    reps = 1 if a.quick else a.reps
    want = a.only or ["config2", "config3", "genome", "single70m"]
    ctx = nt.Context(0, stream=torch.cuda.current_stream().cuda_stream)
    if "config2" in want:
        L, n_reads = 150, 10_000_000
        nbytes = n_reads * (L + 1)
        dev = torch.empty(nbytes + 1024, dtype=torch.uint8, device="cuda")
        ctx.synth_reads_device(0x5EED0002, 0, n_reads, L, 1, dev)
        torch.cuda.synchronize()
        print(json.dumps(run(ctx, "config2", dev, nbytes, offsets_of_equal_records(n_reads, L), n_reads, 21, nt.PATH_BYTES_CANONICAL,
                             nt.PRE_NORMALIZE, reps)), flush=True)
        del dev
        torch.cuda.empty_cache()
    if "config3" in want:
        L, n_reads = 10_000, a.contigs
        nbytes = n_reads * (L + 1)
        dev = torch.empty(nbytes + 2048, dtype=torch.uint8, device="cuda")
        ctx.synth_reads_device(0x5EED0003, 0, n_reads, L, 1, dev)
        torch.cuda.synchronize()
        print(json.dumps(run(ctx, f"config3 shape, {n_reads} x 10 kb", dev, nbytes, offsets_of_equal_records(n_reads, L), n_reads, 31,
                             nt.PATH_BITS_CANONICAL, nt.PRE_STRIP_RETURNS, reps)), flush=True)
        del dev
        torch.cuda.empty_cache()
    if "genome" in want:
        L, n_reads = 150, 10_000_000
        nbytes = n_reads * (L + 1)
        dev = torch.empty(nbytes + 1024, dtype=torch.uint8, device="cuda")
        genome_reads(dev, 0x6E0E, 1_000_000, n_reads, L)
        torch.cuda.synchronize()
        print(json.dumps(run(ctx, "genome", dev, nbytes, offsets_of_equal_records(n_reads, L), n_reads, 21, nt.PATH_BYTES_CANONICAL,
                             nt.PRE_NORMALIZE, reps)), flush=True)
        del dev
        torch.cuda.empty_cache()
    if "single70m" in want:
        rng = np.random.default_rng(0x70)
        genome = np.frombuffer(b"ACGT", dtype=np.uint8)[rng.integers(0, 4, 2000)]
        # the table's batch first: 600 reads of the circular genome at uneven depth, then a short record, the long one, a short one
        reads = [np.tile(genome, 2)[s:s + n] for s, n in zip(rng.integers(0, 2000, 600) ** 2 // 2000, rng.integers(40, 200, 600))]
        head = b"".join(r.tobytes() + b"\n" for r in reads)
        big = 500_000 * 151
        lens = [len(r) for r in reads] + [100, big, 100]
        nbytes = sum(lens) + len(lens)
        dev = torch.full((nbytes + 1024,), ord("\n"), dtype=torch.uint8, device="cuda")
        dev[:len(head)] = torch.from_numpy(np.frombuffer(head, dtype=np.uint8).copy()).cuda()
        g = torch.from_numpy(genome.copy()).cuda()
        at = len(head)
        for n in lens[len(reads):]:
            dev[at:at + n] = g.repeat(n // 2000 + 1)[:n]
            at += n + 1
        d_off = torch.from_numpy(np.concatenate([[0], np.cumsum(np.array(lens) + 1)]).astype(np.int64)).cuda()
        torch.cuda.synchronize()
        print(json.dumps(run(ctx, "single70m", dev, nbytes, d_off, len(lens), 21, nt.PATH_BYTES_CANONICAL, nt.PRE_NORMALIZE, reps,
                             min_count=2, table_bytes=len(head))), flush=True)
    ctx.close()


if __name__ == "__main__":
    main()
