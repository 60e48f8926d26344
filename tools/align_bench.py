#!/usr/bin/env python3
"""Times the base-level alignment of reported chains (needletail_amd.ChainAlignments) on one GPU, in one process, on the two workloads
of tools/chain_bench.py with errors planted into the reads - exact substrings would make no DP segment:

  short   1 M reads of 150 bp on a 100 Mbase random reference.
  long    2 000 reads of 5 000 bp on records of diverged tandem copies of one unit.

`--error-ppm` of the read bases (20 000 by default: 2 %) are substituted by another base, on the device, with a fixed seed; lengths
stay, so the record offsets do.  Substitutions alone are planted: the gaps between the anchors around them are the DP segments.

Every call of the library is synchronous, so a host clock around each call is the call's time: a warm-up first (the arrays grow
there), then `--repeat` rounds; the median, the spread (min and max) and every single time are reported.  One JSON line per workload:
run_ms (ChainAlignments.run on the chains, anchors and reported chains the three handles before it hold, zero-copy), the stats
(n_dp_segments, dp_cells, n_groups, the device memory held), cell updates per second (dp_cells over the median run), and beside them,
from the same session on the same build, chain_ms and mapping_ms (AnchorChains.run and ChainMappings.run of that workload).  --trace
makes a warm-up and one run alone, for a kernel trace of its own.

  python tools/align_bench.py [--workload short|long|both] [--repeat 5] [--error-ppm 20000] [--trace] [--reads N]"""
import argparse
import json
import os
import statistics
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import needletail_amd as nt  # noqa: E402
import chain_bench as CB  # noqa: E402
import seed_index_bench as SB  # noqa: E402

K, W, PATH, PRE = CB.K, CB.W, CB.PATH, CB.PRE
ERROR_SEED = 0xA119


def plant_errors(reads, n_bytes, ppm):
    """Substitute `ppm` per million of the A, C, G, T bytes of the batch by one of the three other bases, in place."""
    import torch
    gen = torch.Generator(device=reads.device).manual_seed(ERROR_SEED)
    view = reads[:n_bytes]
    lut = torch.full((256,), 4, dtype=torch.int64, device=reads.device)
    for i, c in enumerate(b"ACGT"):
        lut[c] = i
    code = lut[view.to(torch.int64)]
    hit = (torch.randint(0, 1_000_000, (n_bytes,), generator=gen, device=reads.device) < ppm) & (code < 4)
    shift = torch.randint(1, 4, (n_bytes,), generator=gen, device=reads.device)
    bases = torch.tensor(list(b"ACGT"), dtype=torch.uint8, device=reads.device)
    view[hit] = bases[(code[hit] + shift[hit]) % 4]
    torch.cuda.synchronize()
    return int(hit.sum())


def bench(name, data, n_records, n_reads, cutoff_ppm, a):
    refs, r_off, r_bytes, reads, q_off, q_bytes, rec, start = data
    n_errors = plant_errors(reads, q_bytes, a.error_ppm)
    with nt.Context(0) as ctx, nt.MinimizerList(K, PATH, W, nt.HASH, ctx) as r_ml, nt.MinimizerList(K, PATH, W, nt.HASH, ctx) as q_ml, \
            nt.SeedIndex(ctx) as si, nt.AnchorChains(ctx) as ch, nt.ChainMappings(ctx) as mp, nt.ChainAlignments(ctx) as al:
        r_ml.run_device(refs, r_bytes, r_off, n_records, PRE)
        q_ml.run_device(reads, q_bytes, q_off, n_reads, PRE)
        si.build(r_ml)
        si.match(q_ml, si.occ_cutoff(cutoff_ppm) if cutoff_ppm else 0)
        batches = (refs, r_bytes, r_off, n_records), (reads, q_bytes, q_off, n_reads)
        calls = {"chain": lambda: ch.run(si, K), "mapping": lambda: mp.run(ch, si, K), "run": lambda: al.run(*batches, ch, si, mp, K)}
        for fn in calls.values():   # the warm-up
            fn()
        if a.trace:
            calls["run"]()
            print(json.dumps({"workload": name, "trace": True, **al.stats()}), flush=True)
            return
        times = {key: [] for key in calls}
        for _ in range(a.repeat):
            for key, fn in calls.items():
                times[key].append(SB.timed(fn))
        st = al.stats()
        out = {"workload": name, "k": K, "w": W, "records": n_records, "reads": n_reads, "error_ppm": a.error_ppm, "errors": n_errors,
               "a": 2, "b": 4, "q": 4, "e": 2, "band_pad": 64, "max_seg": 2048}
        for key, ts in times.items():
            out[key + "_ms"] = round(statistics.median(ts), 3)
            out[key + "_ms_min"], out[key + "_ms_max"] = round(min(ts), 3), round(max(ts), 3)
            out[key + "_ms_all"] = [round(t, 3) for t in ts]
        out.update(st)
        out["gcups"] = round(st["dp_cells"] / out["run_ms"] / 1e6, 3)
        out["run_over_chain"] = round(out["run_ms"] / out["chain_ms"], 3)
        rows = al.read()[0]
        cols = rows[:, 2:6].sum()
        out["identity"] = round(float(rows[:, 2].sum()) / max(int(cols), 1), 5)
        print(json.dumps(out), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--workload", choices=("short", "long", "both"), default="both")
    ap.add_argument("--mbases", type=int, default=100)
    ap.add_argument("--records", type=int, default=1000)
    ap.add_argument("--reads", type=int, default=1_000_000)
    ap.add_argument("--long-records", type=int, default=250)
    ap.add_argument("--long-reads", type=int, default=2000)
    ap.add_argument("--copies", type=int, default=20)
    ap.add_argument("--repeat", type=int, default=5)
    ap.add_argument("--error-ppm", type=int, default=20000)
    ap.add_argument("--trace", action="store_true", help="a warm-up and one run alone")
    a = ap.parse_args()
    if a.workload in ("short", "both"):
        bench("short", SB.make_data(a.mbases * 1_000_000, a.records, a.reads), a.records, a.reads, SB.CUTOFF_PPM, a)
    if a.workload in ("long", "both"):
        bench("long", CB.make_long(a.long_records, a.copies, a.long_reads), a.long_records, a.long_reads, 0, a)


if __name__ == "__main__":
    main()
