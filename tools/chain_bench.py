#!/usr/bin/env python3
"""Times chaining (needletail_amd.AnchorChains) on one GPU, in one process, on two workloads made on the device with torch:

  short   the seed bench's: a 100 Mbase random reference in 1 000 records, 1 M reads of 150 bp with 1 % substitutions, minimizers at
          (15, 10), anchors under occ_cutoff(200).  Many reads, a few dozen anchors each, runs of a few anchors.
  long    long reads on a repetitive reference: records of `--copies` diverged copies (3 % substitutions each) of a random unit of
          2 000 bp, reads of 5 000 bp with 5 % substitutions, no occ cutoff.  Every seed hits most copies of its unit, so a read's
          anchors on a record are one run of thousands of anchors on parallel diagonals: the long runs the random reference never has.

Every call of the library is synchronous, so a host clock around each call is the call's time: a warm-up first (the arrays grow
there), then `--repeat` rounds, the best and every single time reported.  One JSON line per workload: run_ms (AnchorChains.run on the
anchors the SeedIndex holds, zero-copy), read_ms (AnchorChains.read), match_ms beside them (the SeedIndex.match that made the anchors),
the stats (runs, the longest run, chains, members), anchors per second, the share of reads whose best chain lies on the record, strand
and diagonal they were cut from, and the device memory held.  --trace makes a warm-up and one run alone, for a kernel trace of its own.

  python tools/chain_bench.py [--workload short|long|both] [--repeat 5] [--trace] [--reads N] [--copies 20]"""
import argparse
import json
import os
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import needletail_amd as nt  # noqa: E402
import seed_index_bench as SB  # noqa: E402

K, W, PATH, PRE = SB.K, SB.W, SB.PATH, SB.PRE
UNIT, LONG_READ, LONG_SEED = 2000, 5000, 0x5EED52


def make_long(n_records, copies, n_reads):
    """(references, their offsets, bytes, reads, their offsets, bytes, where each read was cut) on the device: every record is `copies`
    copies of its own random unit, each base of each copy substituted with probability 3 %; reads are cut inside a record, 5 %."""
    gen = torch.Generator(device="cuda").manual_seed(LONG_SEED)
    acgt = torch.tensor(list(b"ACGT"), dtype=torch.uint8, device="cuda")
    rec_len = UNIT * copies
    units = torch.randint(0, 4, (n_records, 1, UNIT), generator=gen, device="cuda").expand(n_records, copies, UNIT)
    drift = torch.randint(0, 100, (n_records, copies, UNIT), generator=gen, device="cuda") < 3
    codes = torch.where(drift, torch.randint(0, 4, (n_records, copies, UNIT), generator=gen, device="cuda"), units).reshape(n_records, rec_len)
    refs = torch.full((SB.padded(n_records * (rec_len + 1)),), ord("\n"), dtype=torch.uint8, device="cuda")
    refs[: n_records * (rec_len + 1)].view(n_records, rec_len + 1)[:, :rec_len] = acgt[codes]
    r_off = torch.arange(n_records + 1, dtype=torch.int64, device="cuda") * (rec_len + 1)
    rec = torch.randint(0, n_records, (n_reads,), generator=gen, device="cuda")
    start = torch.randint(0, rec_len - LONG_READ + 1, (n_reads,), generator=gen, device="cuda")
    reads = torch.full((SB.padded(n_reads * (LONG_READ + 1)),), ord("\n"), dtype=torch.uint8, device="cuda")
    at = (rec * (rec_len + 1) + start)[:, None] + torch.arange(LONG_READ, device="cuda")[None, :]
    bases = refs[at]
    flip = torch.randint(0, 100, bases.shape, generator=gen, device="cuda") < 5
    reads[: n_reads * (LONG_READ + 1)].view(n_reads, LONG_READ + 1)[:, :LONG_READ] = torch.where(
        flip, acgt[torch.randint(0, 4, bases.shape, generator=gen, device="cuda")], bases)
    q_off = torch.arange(n_reads + 1, dtype=torch.int64, device="cuda") * (LONG_READ + 1)
    torch.cuda.synchronize()
    return refs, r_off, n_records * (rec_len + 1), reads, q_off, n_reads * (LONG_READ + 1), rec.cpu().numpy(), start.cpu().numpy()


def best_on_origin(result, rec, start):
    """The share of reads whose best chain (the first of the highest score) lies on the record they were cut from, forward, with both end
    anchors on the diagonal of the cut."""
    c_offsets, rows = result[0].astype(np.int64), result[1].astype(np.int64)
    good = 0
    for q in range(rec.size):
        lo, hi = c_offsets[q], c_offsets[q + 1]
        if hi > lo:
            score, _, ref_rev, r0, q0, r1, q1, _ = rows[lo + int(np.argmax(rows[lo:hi, 0]))]
            good += ref_rev == rec[q] << 1 and r0 - q0 == start[q] and r1 - q1 == start[q]
    return round(good / max(rec.size, 1), 5)


def bench(name, data, n_records, n_reads, cutoff_ppm, a):
    refs, r_off, r_bytes, reads, q_off, q_bytes, rec, start = data
    with nt.Context(0) as ctx, nt.MinimizerList(K, PATH, W, nt.HASH, ctx) as r_ml, nt.MinimizerList(K, PATH, W, nt.HASH, ctx) as q_ml, \
            nt.SeedIndex(ctx) as si, nt.AnchorChains(ctx) as ch:
        r_ml.run_device(refs, r_bytes, r_off, n_records, PRE)
        q_ml.run_device(reads, q_bytes, q_off, n_reads, PRE)
        si.build(r_ml)
        cutoff = si.occ_cutoff(cutoff_ppm) if cutoff_ppm else 0
        calls = {"match": lambda: si.match(q_ml, cutoff), "run": lambda: ch.run(si, K), "read": ch.read}
        for fn in calls.values():   # the warm-up
            fn()
        if a.trace:
            calls["run"]()
            print(json.dumps({"workload": name, "trace": True, **ch.stats()}), flush=True)
            return
        times = {key: [] for key in calls}
        for _ in range(a.repeat):
            for key, fn in calls.items():
                times[key].append(SB.timed(fn))
        st = ch.stats()
        out = {"workload": name, "k": K, "w": W, "records": n_records, "reads": n_reads, "max_occ": cutoff, "max_dist": 5000, "bw": 500, "h": 64,
               "min_score": 40, "min_cnt": 3}
        for key, ts in times.items():
            out[key + "_ms"] = round(min(ts), 3)
            out[key + "_ms_all"] = [round(t, 3) for t in ts]
        out.update(st)
        out["manchors_per_s"] = round(st["n_anchors"] / out["run_ms"] / 1e3, 2)
        t = time.perf_counter()
        out["best_chain_on_origin"] = best_on_origin(ch.read(), rec, start)
        out["host_check_s"] = round(time.perf_counter() - t, 2)
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
        bench("long", make_long(a.long_records, a.copies, a.long_reads), a.long_records, a.long_reads, 0, a)


if __name__ == "__main__":
    main()
