"""Throughput of the device count table (include/needletail_amd_count.h), timed with device events on the table's stream.

  (a) config2: the config-2 batch (10M x 150 bp synthetic reads, k = 21, byte path after normalize): ~1.3 G nearly all-distinct keys in
      a 2^31-slot table (32 GiB);
  (b) genome: reads sampled error-free from a seeded random 1 Mb genome, ~1.5 Gbases (~1500x coverage): a repetitive key stream;
  (c) hotkey (--only hotkey): one record of 2^30 A at k = 21 (canonical bits path): 2^30 - 20 occurrences of one key, every lane
      adding to one table slot; one timed call after a 64 MiB warm-up, no repetition.  Then the same with T at k = 32 on the forward
      bits path: the all-ones key, counted in the side word.

For each: count (materialise + insert) in Gbases/s and inserted k-mers/s, extract (count, scan, scatter, sort) and spectrum in ms.
Prints one JSON line per workload.  --quick: one repetition, for a kernel-trace run (rocprofv3 --kernel-trace --stats -- python ...).

--k K runs (a) and (b) at that k instead of 21; k >= 33 selects the wide table (include/needletail_amd_wide_count.h, k = 33..63), whose
count is one fused kernel (read + insert) and whose extract sorts {hi, lo} pairs."""
import argparse
import json
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

import needletail_amd as nt  # noqa: E402
from _count_helpers import device_items  # noqa: E402
from needletail_amd import wide_counting  # noqa: E402


def wide_device_items(table, min_count=1):
    """(keys [n, 2], counts) of a wide table as device tensors."""
    import ctypes as C
    lib = wide_counting.lib()
    n = C.c_uint64(0)
    lib.ntk_wide_table_extract_device(table._h, min_count, None, None, 0, C.byref(n))
    keys = torch.empty(max(2 * n.value, 2), dtype=torch.int64, device="cuda")
    counts = torch.empty(max(n.value, 1), dtype=torch.int64, device="cuda")
    rc = lib.ntk_wide_table_extract_device(table._h, min_count, C.c_void_p(keys.data_ptr()), C.c_void_p(counts.data_ptr()), n.value,
                                           C.byref(n))
    assert rc == 0, rc
    return keys, counts


def genome_reads(dev: torch.Tensor, seed: int, genome_len: int, n_reads: int, L: int):
    g = torch.Generator(device="cuda")
    g.manual_seed(seed)
    acgt = torch.tensor(list(b"ACGT"), dtype=torch.uint8, device="cuda")
    genome = acgt[torch.randint(0, 4, (genome_len,), generator=g, device="cuda")]
    view = dev[: n_reads * (L + 1)].view(n_reads, L + 1)
    view[:, L] = ord("\n")
    off = torch.arange(L, device="cuda")
    for lo in range(0, n_reads, 1_000_000):
        hi = min(n_reads, lo + 1_000_000)
        starts = torch.randint(0, genome_len - L + 1, (hi - lo,), generator=g, device="cuda")
        view[lo:hi, :L] = genome[starts[:, None] + off]


def run(ctx, name, dev, nbytes, k, path, pre, capacity, reps):
    stream = torch.cuda.current_stream()
    ev = [torch.cuda.Event(enable_timing=True) for _ in range(6)]
    count_ms, extract_ms, spectrum_ms = [], [], []
    wide = k > 32
    table, items = (nt.WideKmerTable, wide_device_items) if wide else (nt.KmerTable, device_items)
    with table(k, path, capacity, ctx) as t:
        for r in range(reps + 1):   # the first repetition warms up
            t.reset()
            ev[0].record(stream)
            t.count_device(dev, nbytes, pre)
            ev[1].record(stream)
            ev[1].synchronize()
            ev[2].record(stream)
            keys, counts = items(t)
            ev[3].record(stream)
            ev[3].synchronize()
            del keys, counts
            ev[4].record(stream)
            t.spectrum(16384)
            ev[5].record(stream)
            ev[5].synchronize()
            if r:
                count_ms.append(ev[0].elapsed_time(ev[1]))
                extract_ms.append(ev[2].elapsed_time(ev[3]))
                spectrum_ms.append(ev[4].elapsed_time(ev[5]))
        st = t.stats()
    best = min(count_ms)
    return {"workload": name, "table": "wide" if wide else "narrow", "k": k, "bases": nbytes, "slots": st["slots"], "n_total": st["n_total"], "n_distinct": st["n_distinct"],
            "n_dropped": st["n_dropped"], "count_ms": round(best, 3), "count_ms_all": [round(x, 3) for x in count_ms],
            "gbases_per_s": round(nbytes / best / 1e6, 3), "inserted_kmers_per_s": round(st["n_total"] / best * 1e3, 1),
            "extract_ms": round(min(extract_ms), 3), "spectrum_ms": round(min(spectrum_ms), 3)}


def hotkey(ctx, dev, nbytes, base, k, path):
    stream = torch.cuda.current_stream()
    ev = [torch.cuda.Event(enable_timing=True) for _ in range(2)]
    dev.fill_(ord("\n"))
    dev[: nbytes - 1] = base
    torch.cuda.synchronize()
    with nt.KmerTable(k, path, 1024, ctx) as t:
        t.count_device(dev, (64 << 20) + 16, nt.PRE_NONE)   # warm-up: kernels loaded, the scratch of a whole chunk allocated
        ctx.synchronize()
        t.reset()
        ev[0].record(stream)
        t.count_device(dev, nbytes, nt.PRE_NONE)
        ev[1].record(stream)
        ev[1].synchronize()
        st = t.stats()
    ms = ev[0].elapsed_time(ev[1])
    return {"workload": "hotkey" if path != nt.PATH_BITS else "hotkey_side_word", "k": k, "bases": nbytes - 1,
            "n_total": st["n_total"], "n_distinct": st["n_distinct"], "n_dropped": st["n_dropped"], "count_ms": round(ms, 3),
            "inserted_kmers_per_s": round(st["n_total"] / ms * 1e3, 1), "s_per_2_32_occurrences": round((1 << 32) / st["n_total"] * ms / 1e3, 2)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--quick", action="store_true")
    ap.add_argument("--only", choices=["config2", "genome", "hotkey"], default=None)
    ap.add_argument("--k", type=int, default=21, help="k of workloads (a) and (b); k >= 33: the wide table")
    a = ap.parse_args()
    reps = 1 if a.quick else a.reps
    ctx = nt.Context(0, stream=torch.cuda.current_stream().cuda_stream)
    if a.only == "hotkey":
        nbytes = (1 << 30) + 1
        dev = torch.empty(nbytes + 1024, dtype=torch.uint8, device="cuda")
        print(json.dumps(hotkey(ctx, dev, nbytes, ord("A"), 21, nt.PATH_BITS_CANONICAL)), flush=True)
        print(json.dumps(hotkey(ctx, dev, nbytes, ord("T"), 32, nt.PATH_BITS)), flush=True)
        ctx.close()
        return
    L = 150
    n_reads = 10_000_000
    nbytes = n_reads * (L + 1)
    dev = torch.empty(nbytes + 1024, dtype=torch.uint8, device="cuda")
    if a.only in (None, "config2"):
        ctx.synth_reads_device(0x5EED0002, 0, n_reads, L, 1, dev)
        print(json.dumps(run(ctx, "config2", dev, nbytes, a.k, nt.PATH_BYTES_CANONICAL, nt.PRE_NORMALIZE, 1_400_000_000, reps)), flush=True)
    if a.only in (None, "genome"):
        genome_reads(dev, 0x6E0E, 1_000_000, n_reads, L)
        torch.cuda.synchronize()
        print(json.dumps(run(ctx, "genome", dev, nbytes, a.k, nt.PATH_BYTES_CANONICAL, nt.PRE_NORMALIZE, 2_000_000, reps)), flush=True)
    ctx.close()


if __name__ == "__main__":
    main()
