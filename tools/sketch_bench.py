"""What the k-mer sketch costs and what it saves (include/needletail_amd_sketch.h), timed with device events on the context's stream.

  (a) config2: the config-2 batch (10M x 150 bp synthetic reads, byte path after normalize) at k = 21: ~1.3 G nearly all-distinct keys;
  (b) genome:  reads sampled error-free from a seeded random 1 Mb genome, ~1.5 Gbases, at k = 21: ~1 M distinct keys;
  (c) config2_wide: the config-2 batch at k = 51 (the wide walker and the wide table).

For each, in one process and alternating within every repetition (one warm-up repetition, then the best of --reps):
  sketch        reset + add_device: the first pass;
  count_sized   reset + count_device of a table created with the sketch's capacity: the second pass;
  count_bases   reset + count_device of a table created with capacity = bases, the size a caller without the sketch has to guess.
Prints one JSON line per workload.  --quick: one repetition, for a kernel-trace run (rocprofv3 --kernel-trace --stats -- python ...)."""
import argparse
import json
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))

import needletail_amd as nt  # noqa: E402
from count_bench import genome_reads  # noqa: E402


def timed(stream, *steps):
    """Milliseconds of each step, run back to back on the stream."""
    ev = [torch.cuda.Event(enable_timing=True) for _ in range(len(steps) + 1)]
    ev[0].record(stream)
    for i, step in enumerate(steps):
        step()
        ev[i + 1].record(stream)
    ev[-1].synchronize()
    return [ev[i].elapsed_time(ev[i + 1]) for i in range(len(steps))]


def run(ctx, name, dev, nbytes, k, path, pre, reps):
    stream = torch.cuda.current_stream()
    table = nt.KmerTable if k <= 32 else nt.WideKmerTable
    with nt.KmerSketch(k, path, ctx) as sk:
        sk.add_device(dev, nbytes, pre)
        est = sk.estimate()
        with sk.table() as sized, table(k, path, nbytes, ctx) as guessed:
            rows = {"sketch": [], "count_sized": [], "count_bases": []}
            for r in range(reps + 1):   # the first repetition warms up
                got = {"sketch": timed(stream, sk.reset, lambda: sk.add_device(dev, nbytes, pre)),
                       "count_sized": timed(stream, sized.reset, lambda: sized.count_device(dev, nbytes, pre)),
                       "count_bases": timed(stream, guessed.reset, lambda: guessed.count_device(dev, nbytes, pre))}
                if r:
                    for key, v in got.items():
                        rows[key].append(v)
            st, sg = sized.stats(), guessed.stats()
            assert sk.estimate() == est and st["n_dropped"] == 0 and sg["n_dropped"] == 0 and st["n_distinct"] == sg["n_distinct"]
    best = {key: min(v, key=sum) for key, v in rows.items()}   # [reset ms, pass ms] of the repetition with the smallest sum
    out = {"workload": name, "k": k, "bases": nbytes, "n_windows": est["n_windows"], "estimate": round(est["distinct"], 1),
           "n_distinct": st["n_distinct"], "estimate_over_exact": round(est["distinct"] / st["n_distinct"], 5),
           "capacity": est["capacity"], "slots_sized": st["slots"], "slots_bases": sg["slots"]}
    for key, (reset_ms, pass_ms) in best.items():
        out[key + "_reset_ms"], out[key + "_ms"] = round(reset_ms, 3), round(pass_ms, 3)
        out[key + "_all_ms"] = [round(sum(v), 3) for v in rows[key]]
    two_pass = sum(best["sketch"]) + sum(best["count_sized"])
    out["sketch_over_count_sized"] = round(sum(best["sketch"]) / sum(best["count_sized"]), 4)
    out["two_pass_ms"], out["guessed_ms"] = round(two_pass, 3), round(sum(best["count_bases"]), 3)
    out["sketch_gbases_per_s"] = round(nbytes / best["sketch"][1] / 1e6, 1)
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--quick", action="store_true")
    ap.add_argument("--only", choices=["config2", "genome", "config2_wide"], default=None)
    a = ap.parse_args()
    reps = 1 if a.quick else a.reps
    ctx = nt.Context(0, stream=torch.cuda.current_stream().cuda_stream)
    L, n_reads = 150, 10_000_000
    nbytes = n_reads * (L + 1)
    dev = torch.empty(nbytes + 1024, dtype=torch.uint8, device="cuda")
    byte_path = (nt.PATH_BYTES_CANONICAL, nt.PRE_NORMALIZE)
    if a.only in (None, "config2", "config2_wide"):
        ctx.synth_reads_device(0x5EED0002, 0, n_reads, L, 1, dev)
        if a.only != "config2_wide":
            print(json.dumps(run(ctx, "config2", dev, nbytes, 21, *byte_path, reps)), flush=True)
        if a.only != "config2":
            print(json.dumps(run(ctx, "config2_wide", dev, nbytes, 51, *byte_path, reps)), flush=True)
    if a.only in (None, "genome"):
        genome_reads(dev, 0x6E0E, 1_000_000, n_reads, L)
        torch.cuda.synchronize()
        print(json.dumps(run(ctx, "genome", dev, nbytes, 21, *byte_path, reps)), flush=True)
    ctx.close()


if __name__ == "__main__":
    main()
