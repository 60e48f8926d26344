#!/usr/bin/env python3
"""Times the marking of primary and secondary chains (needletail_amd.ChainMappings) on one GPU, in one process, on the two workloads of
tools/chain_bench.py, made on the device with torch:

  short   1 M reads of 150 bp on a 100 Mbase random reference: many reads, one or two chains each.
  long    2 000 reads of 5 000 bp on records of diverged tandem copies of one unit: hundreds of chains per read, most of them on the
          same stretch of the read - the quadratic side of the parent rule.

Every call of the library is synchronous, so a host clock around each call is the call's time: a warm-up first (the arrays grow
there), then `--repeat` rounds, the best and every single time reported.  One JSON line per workload: run_ms (ChainMappings.run on the
chains the AnchorChains and the anchors the SeedIndex hold, zero-copy), read_ms (ChainMappings.read), chain_ms beside them (the
AnchorChains.run that made the chains), the stats (chains, primaries, kept secondaries, the chains of the busiest read), chains per
second, the share of reads whose rank-0 chain lies on the record and strand they were cut from, the histogram of its mapping quality in
three bins, and the device memory held.  --trace makes a warm-up and one run alone, for a kernel trace of its own.

  python tools/mapping_bench.py [--workload short|long|both] [--repeat 5] [--trace] [--reads N] [--copies 20]"""
import argparse
import json
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import needletail_amd as nt  # noqa: E402
import chain_bench as CB  # noqa: E402
import seed_index_bench as SB  # noqa: E402

K, W, PATH, PRE = CB.K, CB.W, CB.PATH, CB.PRE


def top_on_origin(c_offsets, result, rec):
    """The share of reads whose rank-0 chain lies on the record they were cut from, forward; the mapq of those chains in three bins."""
    rows, order, _, _, read_rows = result
    has = read_rows[:, 0] > 0
    top = rows[order[c_offsets[:-1][has].astype(np.int64)]]
    good = int(np.sum(top[:, 4] == (rec[has].astype(np.uint32) << 1)))
    q = top[:, 12]
    return round(good / max(rec.size, 1), 5), {"0": int(np.sum(q == 0)), "1..59": int(np.sum((q > 0) & (q < 60))), "60": int(np.sum(q == 60))}


def bench(name, data, n_records, n_reads, cutoff_ppm, a):
    refs, r_off, r_bytes, reads, q_off, q_bytes, rec, start = data
    with nt.Context(0) as ctx, nt.MinimizerList(K, PATH, W, nt.HASH, ctx) as r_ml, nt.MinimizerList(K, PATH, W, nt.HASH, ctx) as q_ml, \
            nt.SeedIndex(ctx) as si, nt.AnchorChains(ctx) as ch, nt.ChainMappings(ctx) as mp:
        r_ml.run_device(refs, r_bytes, r_off, n_records, PRE)
        q_ml.run_device(reads, q_bytes, q_off, n_reads, PRE)
        si.build(r_ml)
        si.match(q_ml, si.occ_cutoff(cutoff_ppm) if cutoff_ppm else 0)
        calls = {"chain": lambda: ch.run(si, K), "run": lambda: mp.run(ch, si, K), "read": mp.read}
        for fn in calls.values():   # the warm-up
            fn()
        if a.trace:
            calls["run"]()
            print(json.dumps({"workload": name, "trace": True, **mp.stats()}), flush=True)
            return
        times = {key: [] for key in calls}
        for _ in range(a.repeat):
            for key, fn in calls.items():
                times[key].append(SB.timed(fn))
        st = mp.stats()
        out = {"workload": name, "k": K, "w": W, "records": n_records, "reads": n_reads, "mask_level_pm": 500, "pri_ratio_pm": 800, "best_n": 5,
               "min_chain_score": 40}
        for key, ts in times.items():
            out[key + "_ms"] = round(min(ts), 3)
            out[key + "_ms_all"] = [round(t, 3) for t in ts]
        out.update(st)
        out["n_anchors"], out["n_members"] = ch.stats()["n_anchors"], ch.stats()["n_members"]
        out["mchains_per_s"] = round(st["n_chains"] / out["run_ms"] / 1e3, 2)
        out["run_over_chain"] = round(out["run_ms"] / out["chain_ms"], 3)
        out["top_chain_on_origin"], out["top_mapq"] = top_on_origin(ch.read()[0], mp.read(), rec)
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
    ap.add_argument("--trace", action="store_true", help="a warm-up and one run alone")
    a = ap.parse_args()
    if a.workload in ("short", "both"):
        bench("short", SB.make_data(a.mbases * 1_000_000, a.records, a.reads), a.records, a.reads, SB.CUTOFF_PPM, a)
    if a.workload in ("long", "both"):
        bench("long", CB.make_long(a.long_records, a.copies, a.long_reads), a.long_records, a.long_reads, 0, a)


if __name__ == "__main__":
    main()
