#!/usr/bin/env python3
"""Times seeding (needletail_amd.SeedIndex) on seeded synthetic data of a size a user would run, on one GPU, in one process: a
100 Mbase reference in 1 000 records, 1 M reads of 150 bp cut from it with 1 % substitutions, minimizers at (15, 10) in hash order on
the bit-canonical path, max_occ from occ_cutoff(200) - minimap2's -f 0.0002.  The data is made on the device with torch.

Every call of the library is synchronous, so a host clock around each call is the call's time: a warm-up of every call first (the
arrays grow there), then `--repeat` rounds, the best and every single time reported.  One JSON line:

  list_refs_ms, list_reads_ms   MinimizerList.run_device on the references and on the reads (what seeding consumes; not this library's)
  build_ms                      SeedIndex.build from the held reference list: verify, owners, radix sort, heads, scan, pack, largest occ
  spectrum_ms                   SeedIndex.spectrum(256)
  match_ms, match_all_ms        SeedIndex.match under the cutoff and with max_occ = 0: verify, lookup, scan, rows, fill, sort
  read_ms                       SeedIndex.read of the match under the cutoff (device to pageable host arrays)

with the entries, keys, largest occ, the cutoff, seeds, anchors, the share of reads with an anchor on the diagonal they were cut from,
and the device memory held.  --trace makes a warm-up and one build and match alone, for a kernel trace of their own.

  python tools/seed_index_bench.py [--mbases 100] [--records 1000] [--reads 1000000] [--repeat 5] [--trace]"""
import argparse
import json
import os
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import needletail_amd as nt  # noqa: E402

K, W, PATH, PRE = 15, 10, nt.PATH_BITS_CANONICAL, nt.PRE_NORMALIZE
READ_LEN, SEED, SUBSTITUTIONS_PPM, CUTOFF_PPM = 150, 0x5EED51, 10_000, 200


def padded(n):
    return (n + 15) // 16 * 16 + 64


def make_data(n_bases, n_records, n_reads):
    """(references, their offsets, reads, their offsets, where each read was cut) on the device: records of equal length, each with
    its break byte; reads cut inside a record, every base substituted with probability 1 %."""
    gen = torch.Generator(device="cuda").manual_seed(SEED)
    acgt = torch.tensor(list(b"ACGT"), dtype=torch.uint8, device="cuda")
    rec_len = n_bases // n_records
    refs = torch.full((padded(n_records * (rec_len + 1)),), ord("\n"), dtype=torch.uint8, device="cuda")
    body = refs[: n_records * (rec_len + 1)].view(n_records, rec_len + 1)
    body[:, :rec_len] = acgt[torch.randint(0, 4, (n_records, rec_len), generator=gen, device="cuda")]
    r_off = torch.arange(n_records + 1, dtype=torch.int64, device="cuda") * (rec_len + 1)
    rec = torch.randint(0, n_records, (n_reads,), generator=gen, device="cuda")
    start = torch.randint(0, rec_len - READ_LEN + 1, (n_reads,), generator=gen, device="cuda")
    reads = torch.full((padded(n_reads * (READ_LEN + 1)),), ord("\n"), dtype=torch.uint8, device="cuda")
    q_body = reads[: n_reads * (READ_LEN + 1)].view(n_reads, READ_LEN + 1)
    at = (rec * (rec_len + 1) + start)[:, None] + torch.arange(READ_LEN, device="cuda")[None, :]
    bases = refs[at]
    flip = torch.randint(0, 1_000_000, bases.shape, generator=gen, device="cuda") < SUBSTITUTIONS_PPM
    other = acgt[torch.randint(0, 4, bases.shape, generator=gen, device="cuda")]
    q_body[:, :READ_LEN] = torch.where(flip, other, bases)
    q_off = torch.arange(n_reads + 1, dtype=torch.int64, device="cuda") * (READ_LEN + 1)
    torch.cuda.synchronize()
    return refs, r_off, n_records * (rec_len + 1), reads, q_off, n_reads * (READ_LEN + 1), rec.cpu().numpy(), start.cpu().numpy()


def timed(fn):
    torch.cuda.synchronize()
    t = time.perf_counter()
    fn()
    return (time.perf_counter() - t) * 1e3


def on_diagonal(result, rec, start):
    """The share of reads with at least one forward anchor on their own record at rpos - qpos == the cut's start."""
    a_offsets, ref, rev, rpos, qpos, _ = result
    read = np.repeat(np.arange(rec.size), np.diff(a_offsets.astype(np.int64)))
    good = (ref == rec[read]) & (rev == 0) & (rpos.astype(np.int64) - qpos.astype(np.int64) == start[read])
    return round(np.unique(read[good]).size / max(rec.size, 1), 5)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--mbases", type=int, default=100)
    ap.add_argument("--records", type=int, default=1000)
    ap.add_argument("--reads", type=int, default=1_000_000)
    ap.add_argument("--repeat", type=int, default=5)
    ap.add_argument("--trace", action="store_true", help="a warm-up and one build and match alone")
    a = ap.parse_args()
    refs, r_off, r_bytes, reads, q_off, q_bytes, rec, start = make_data(a.mbases * 1_000_000, a.records, a.reads)
    with nt.Context(0) as ctx, nt.MinimizerList(K, PATH, W, nt.HASH, ctx) as r_ml, nt.MinimizerList(K, PATH, W, nt.HASH, ctx) as q_ml, \
            nt.SeedIndex(ctx) as si:
        calls = {
            "list_refs": lambda: r_ml.run_device(refs, r_bytes, r_off, a.records, PRE),
            "list_reads": lambda: q_ml.run_device(reads, q_bytes, q_off, a.reads, PRE),
            "build": lambda: si.build(r_ml),
            "spectrum": lambda: si.spectrum(256),
            "match_all": lambda: si.match(q_ml, 0),
        }
        for fn in calls.values():   # the warm-up
            fn()
        cutoff = si.occ_cutoff(CUTOFF_PPM)
        calls["match"] = lambda: si.match(q_ml, cutoff)
        calls["read"] = si.read
        calls["match"]()
        if a.trace:
            calls["build"]()
            calls["match"]()
            print(json.dumps({"trace": True, "cutoff": cutoff, **si.stats()}), flush=True)
            return
        times = {name: [] for name in calls}
        for _ in range(a.repeat):
            for name, fn in calls.items():
                times[name].append(timed(fn))
        calls["match_all"]()
        st_all = si.stats()
        calls["match"]()
        st, result = si.stats(), si.read()
        out = {"k": K, "w": W, "order": "hash", "mbases": a.mbases, "records": a.records, "reads": a.reads, "read_len": READ_LEN,
               "substitutions_ppm": SUBSTITUTIONS_PPM, "cutoff_ppm": CUTOFF_PPM, "max_occ": cutoff}
        for name, ts in times.items():
            out[name + "_ms"] = round(min(ts), 3)
            out[name + "_ms_all"] = [round(t, 3) for t in ts]
        out.update({key: st[key] for key in ("n_entries", "n_keys", "n_seeds", "n_anchors", "device_bytes")})
        out["largest_occ"] = st["max_occ"]
        out["n_anchors_all"] = st_all["n_anchors"]
        out["reads_on_their_diagonal"] = on_diagonal(result, rec, start)
        out["mseeds_per_s"] = round(st["n_seeds"] / out["match_ms"] / 1e3, 2)
        out["mentries_per_s_build"] = round(st["n_entries"] / out["build_ms"] / 1e3, 2)
        print(json.dumps(out), flush=True)


if __name__ == "__main__":
    main()
