"""What trimming costs (include/needletail_amd_trim.h): ReadTrimmer.run_device and compact_device, each on the host clock around its
synchronising end, one warm-up call and then --reps repetitions (default 5), on the workloads of tools/abundance_bench.py at
min_count = 3:

  config2:   the config-2 batch (10 M x 150 bp synthetic reads, byte path after normalize), k = 21, table from the same batch;
  config3:   100 000 x 10 kb, k = 31, bit-packed canonical path after strip_returns, table from the same batch;
  genome:    10 M x 150 bp reads of a seeded random 1 Mb genome, k = 21, table from the same batch;
  single70m: one record of 75.5 M bases between two short ones, against a table of its 2 000-base genome (min_count 2).

Prints one JSON line per workload.  Three more modes:

  --trace    ReadAbundance.run_device and ReadTrimmer.run_device once each (after a warm-up of each) on the first three workloads and
             the same table, for `rocprofv3 --kernel-trace --stats -- python tools/trim_bench.py --trace`: the gate is the total of
             rt_solid_kernel + rt_interval_kernel against the total of the ra_* kernels in that one trace.
  --copy     the copy gate: LONGEST mode on the genome reads (the config-2 batch's size; most reads survive), sequence and a parallel
             stream.  compact_device and a hipMemcpyAsync device-to-device of the same number of output bytes alternate in one
             process, both between device events on the stream.  compact_device is also timed as a size query (the scan, the read
             of its total and the return, no copy): the copy kernels' time is the whole call minus the query.
  --host-route  what the same result costs without this library, on the first --sample reads of the genome workload (PREFIX mode):
             counts of every window through materialize + lookup to the host (8 B per base), intervals on the host (numpy),
             ntk_batch_append re-pack of the kept parts, upload; next to run_device + compact_device on the same reads."""
import argparse
import ctypes as C
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
from abundance_bench import offsets_of_equal_records  # noqa: E402
from count_bench import genome_reads  # noqa: E402

MIN_COUNT = 3


def workloads(ctx, want, contigs):
    """(name, dev, nbytes, d_off, n_records, k, path, pre, min_count, table_bytes), one at a time."""
    if "config2" in want:
        L, n = 150, 10_000_000
        dev = torch.empty(n * (L + 1) + 1024, dtype=torch.uint8, device="cuda")
        ctx.synth_reads_device(0x5EED0002, 0, n, L, 1, dev)
        yield "config2", dev, n * (L + 1), offsets_of_equal_records(n, L), n, 21, nt.PATH_BYTES_CANONICAL, nt.PRE_NORMALIZE, MIN_COUNT, None
    if "config3" in want:
        L, n = 10_000, contigs
        dev = torch.empty(n * (L + 1) + 2048, dtype=torch.uint8, device="cuda")
        ctx.synth_reads_device(0x5EED0003, 0, n, L, 1, dev)
        yield (f"config3 shape, {n} x 10 kb", dev, n * (L + 1), offsets_of_equal_records(n, L), n, 31, nt.PATH_BITS_CANONICAL,
               nt.PRE_STRIP_RETURNS, MIN_COUNT, None)
    if "genome" in want:
        L, n = 150, 10_000_000
        dev = torch.empty(n * (L + 1) + 1024, dtype=torch.uint8, device="cuda")
        genome_reads(dev, 0x6E0E, 1_000_000, n, L)
        yield "genome", dev, n * (L + 1), offsets_of_equal_records(n, L), n, 21, nt.PATH_BYTES_CANONICAL, nt.PRE_NORMALIZE, MIN_COUNT, None
    if "single70m" in want:
        rng = np.random.default_rng(0x70)
        genome = np.frombuffer(b"ACGT", dtype=np.uint8)[rng.integers(0, 4, 2000)]
        reads = [np.tile(genome, 2)[s:s + n] for s, n in zip(rng.integers(0, 2000, 600) ** 2 // 2000, rng.integers(40, 200, 600))]
        head = b"".join(r.tobytes() + b"\n" for r in reads)
        lens = [len(r) for r in reads] + [100, 500_000 * 151, 100]
        nbytes = sum(lens) + len(lens)
        dev = torch.full((nbytes + 1024,), ord("\n"), dtype=torch.uint8, device="cuda")
        dev[:len(head)] = torch.from_numpy(np.frombuffer(head, dtype=np.uint8).copy()).cuda()
        g, at = torch.from_numpy(genome.copy()).cuda(), len(head)
        for n in lens[len(reads):]:
            dev[at:at + n] = g.repeat(n // 2000 + 1)[:n]
            at += n + 1
        d_off = torch.from_numpy(np.concatenate([[0], np.cumsum(np.array(lens) + 1)]).astype(np.int64)).cuda()
        yield "single70m", dev, nbytes, d_off, len(lens), 21, nt.PATH_BYTES_CANONICAL, nt.PRE_NORMALIZE, 2, len(head)


def table_for(ctx, dev, counted, k, path, pre):
    with nt.KmerSketch(k, path, ctx) as sk:
        sk.add_device(dev, counted, pre)
        t = sk.table()
    t.count_device(dev, counted, pre)
    assert t.stats()["n_dropped"] == 0
    return t


def host_ms(call, reps):
    ms, out = [], None
    for r in range(reps + 1):   # the first call warms up (and allocates the scratch)
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        out = call()
        dt = (time.perf_counter() - t0) * 1e3
        if r:
            ms.append(dt)
    return out, ms


def spread(ms):
    return {"best_ms": round(min(ms), 3), "all_ms": [round(v, 3) for v in ms], "spread": round((max(ms) - min(ms)) / min(ms), 4)}


def bench(ctx, w, reps):
    name, dev, nbytes, d_off, n, k, path, pre, mc, table_bytes = w
    torch.cuda.synchronize()
    out = {"workload": name, "k": k, "bases": nbytes, "n_records": n, "min_count": mc}
    with table_for(ctx, dev, table_bytes or nbytes, k, path, pre) as t, nt.ReadTrimmer(t) as rt:
        for mode in ("prefix", "longest"):
            rows, ms = host_ms(lambda: rt.run_device(dev, nbytes, d_off, n, pre, min_count=mc, mode=mode), reps)
            got, cms = host_ms(lambda: rt.compact_device(dev, nbytes, d_off, n, rows), reps)
            out[mode] = {"run_device": spread(ms), "gbases_per_s": round(nbytes / min(ms) / 1e6, 2), "compact_device": spread(cms),
                         "records_out": len(got[3]), "bytes_out": got[1], "n_kmers": int(rows[:, 2].sum()), "n_solid": int(rows[:, 3].sum()),
                         "first_rows": rows[: min(n, 3)].cpu().numpy().view(np.uint64).tolist()}
            del got, rows
            torch.cuda.empty_cache()
    return out


def trace(ctx, w):
    name, dev, nbytes, d_off, n, k, path, pre, mc, table_bytes = w
    with table_for(ctx, dev, table_bytes or nbytes, k, path, pre) as t, nt.ReadAbundance(t) as ra, nt.ReadTrimmer(t) as rt:
        for _ in range(2):   # a warm-up of each, then the pair that is compared (both are in the trace: halve the totals)
            a = ra.run_device(dev, nbytes, d_off, n, pre, min_count=mc)
            r = rt.run_device(dev, nbytes, d_off, n, pre, min_count=mc, mode="longest")
        assert torch.equal(a[:, 0], r[:, 2]) and torch.equal(a[:, 1], r[:, 3])
    return {"workload": name, "traced": "2 x (ReadAbundance.run_device, ReadTrimmer.run_device)", "n_kmers": int(r[:, 2].sum())}


def copy_gate(ctx, w, reps):
    name, dev, nbytes, d_off, n, k, path, pre, mc, table_bytes = w
    hip = C.CDLL("libamdhip64.so")
    hip.hipMemcpyAsync.argtypes = [C.c_void_p, C.c_void_p, C.c_size_t, C.c_int, C.c_void_p]
    stream = torch.cuda.current_stream()
    aux = torch.randint(33, 127, (dev.numel(),), dtype=torch.uint8, device="cuda")
    with table_for(ctx, dev, nbytes, k, path, pre) as t, nt.ReadTrimmer(t) as rt:
        rows = rt.run_device(dev, nbytes, d_off, n, pre, min_count=mc, mode="longest")
        out = rt.compact_device(dev, nbytes, d_off, n, rows, aux)   # warms up, and gives the output's size
        nb, n_out = out[1], len(out[3])
        out_seq, out_aux, out_off, out_src = out[0], out[4], torch.empty(n_out + 1, dtype=torch.int64, device="cuda"), torch.empty_like(out[3])
        dst, dst2 = torch.empty_like(out_seq), torch.empty_like(out_seq)
        cap = (nb + 15) // 16 * 16
        lib, nbq, nrq = nt.trimming.lib(), C.c_uint64(0), C.c_uint64(0)
        vp = lambda x: None if x is None else C.c_void_p(x.data_ptr())   # noqa: E731

        def compact(seq_out, aux_out, cap_bytes, off_out, src_out, cap_records):
            return lib.ntk_read_trim_compact_device(rt._h, vp(dev), vp(aux), nbytes, vp(d_off), n, vp(rows), vp(seq_out), vp(aux_out), cap_bytes,
                                                    vp(off_out), vp(src_out), cap_records, C.byref(nbq), C.byref(nrq))

        ev = [torch.cuda.Event(enable_timing=True) for _ in range(6)]
        full, query, memcpy = [], [], []
        for r in range(reps + 1):
            ev[0].record(stream)
            rc = compact(out_seq, out_aux, cap, out_off, out_src, n_out)
            ev[1].record(stream)
            assert rc == 0 and nbq.value == nb and nrq.value == n_out
            ev[2].record(stream)
            rc = compact(None, None, 0, None, None, 0)
            ev[3].record(stream)
            assert rc == 5 and nbq.value == nb
            ev[4].record(stream)
            for d, s_ in ((dst, out_seq), (dst2, out_aux)):
                assert hip.hipMemcpyAsync(vp(d), vp(s_), nb, 3, C.c_void_p(stream.cuda_stream)) == 0   # hipMemcpyDeviceToDevice
            ev[5].record(stream)
            torch.cuda.synchronize()
            if r:
                full.append(ev[0].elapsed_time(ev[1]))
                query.append(ev[2].elapsed_time(ev[3]))
                memcpy.append(ev[4].elapsed_time(ev[5]))
        assert torch.equal(dst[:nb], out_seq[:nb]) and torch.equal(dst2[:nb], out_aux[:nb])
    # the size query runs the scan, reads its total and returns: the whole call minus the query is the copy kernels' time
    copy = min(full) - min(query)
    return {"workload": name + " (copy gate)", "records_out": n_out, "bytes_out_per_stream": nb, "streams": 2,
            "compact_device": spread(full), "size_query": spread(query), "memcpy_d2d_same_bytes": spread(memcpy),
            "copy_ms_full_minus_query": round(copy, 3), "ratio_to_memcpy": round(copy / min(memcpy), 3)}


def host_route(ctx, w, sample, reps):
    """PREFIX mode on the first `sample` reads, the table from the whole batch."""
    name, dev, nbytes, d_off, n, k, path, pre, mc, table_bytes = w
    L = 150
    sub = sample * (L + 1)
    d_sub_off = offsets_of_equal_records(sample, L)
    with table_for(ctx, dev, nbytes, k, path, pre) as t, nt.ReadTrimmer(t) as rt:
        def device_path():
            rows = rt.run_device(dev, sub, d_sub_off, sample, pre, min_count=mc, mode="prefix")
            return rt.compact_device(dev, sub, d_sub_off, sample, rows)

        def host_path():
            vals = torch.empty(sub, dtype=torch.int64, device="cuda")
            v16, r16 = (torch.empty(sub // 16 + 1, dtype=torch.int16, device="cuda") for _ in range(2))
            counts = torch.empty(sub, dtype=torch.int64, device="cuda")
            ctx.materialize_device(dev, sub, k, path, pre, vals, v16, r16)
            rc = nt.counting.lib().ntk_kmer_table_lookup_device(t._h, C.c_void_p(vals.data_ptr()), sub, C.c_void_p(counts.data_ptr()))
            assert rc == 0
            c = counts.cpu().numpy().reshape(sample, L + 1)          # 8 B per base over the bus
            valid = np.unpackbits(v16.cpu().numpy().view(np.uint8).reshape(-1, 2)[:, ::-1].reshape(-1))[:sub].reshape(sample, L + 1)
            seq = dev[:sub].cpu().numpy().reshape(sample, L + 1)
            solid = (valid[:, k - 1:L] == 1) & (c[:, k - 1:L] >= mc)
            lead = np.where(solid.all(axis=1), L - k + 1, np.argmin(solid, axis=1))
            length = np.where(lead > 0, lead + k - 1, 0)
            b = nt.Batch(ctx, int(length.sum()) + sample, sample)
            for i in np.nonzero(length)[0]:
                b.append(seq[i, :length[i]].tobytes(), pre)
            packed, _ = b.buffers()
            up = torch.from_numpy(np.array(packed, copy=True)).cuda()
            torch.cuda.synchronize()
            b.release()
            return up

        got, dms = host_ms(device_path, reps)
        up, hms = host_ms(host_path, 1)
        assert got[1] == up.numel() and torch.equal(got[0][:got[1]], up)
    return {"workload": f"{name}, first {sample} reads, PREFIX", "bytes_out": got[1], "records_out": len(got[3]),
            "device_path": spread(dms), "host_route": spread(hms), "host_over_device": round(min(hms) / min(dms), 1)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--quick", action="store_true")
    ap.add_argument("--only", nargs="+", choices=["config2", "config3", "genome", "single70m"], default=None)
    ap.add_argument("--contigs", type=int, default=100_000)
    ap.add_argument("--trace", action="store_true")
    ap.add_argument("--copy", action="store_true")
    ap.add_argument("--host-route", action="store_true")
    ap.add_argument("--sample", type=int, default=1_000_000)
    a = ap.parse_args()
    reps = 1 if a.quick else a.reps
    ctx = nt.Context(0, stream=torch.cuda.current_stream().cuda_stream)
    if a.trace:
        for w in workloads(ctx, a.only or ["config2", "config3", "genome"], a.contigs):
            print(json.dumps(trace(ctx, w)), flush=True)
    elif a.copy or a.host_route:
        for w in workloads(ctx, ["genome"], a.contigs):
            print(json.dumps(copy_gate(ctx, w, reps) if a.copy else host_route(ctx, w, a.sample, reps)), flush=True)
    else:
        for w in workloads(ctx, a.only or ["config2", "config3", "genome", "single70m"], a.contigs):
            print(json.dumps(bench(ctx, w, reps)), flush=True)
            del w
            torch.cuda.empty_cache()
    ctx.close()


if __name__ == "__main__":
    main()
