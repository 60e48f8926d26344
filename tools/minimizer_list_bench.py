#!/usr/bin/env python3
"""Times the minimizer-list call (needletail_amd.MinimizerList.run_device) on the config-2 batch - 10 M reads of 150 bp, made on the
device (ntk_synth_reads_device) - against the work the core already does on the same bases, on one GPU, in one process, the routes
alternated, best of `--repeat` after a warm-up; one JSON line per (k, w) and order.

  list         MinimizerList.run_device on the whole batch: materialise chunk by chunk, select, compaction, record ranges.  The
               result stays on the device; nothing is read back inside the timed region
  two_pass     the core's two-pass reduce route (ntk_minimizers_reduce_device with the fused and the generic kernels switched off)
               for the same (k, w): materialise-like scan plus a window pass, folded into counters - the comparable work
  materialize  ntk_materialize_device alone over the same chunks (64 Mi bases at a time into one scratch)

Reported besides the times: the entries, their density against the 2 / (w + 1) of random keys, the windows, device memory held.  The
list's LEX digest is checked against the two-pass route's counters before anything is timed.  The split of run_device into materialise,
select and compaction is not timed from here (the call is one synchronous C call): --trace runs the list alone, a warm-up and one call,
for a kernel trace of its own, which names the kernels.

  python tools/minimizer_list_bench.py [--reads 10000000] [--repeat 5] [--config 21,11] [--trace 21,11,lex]"""
import argparse
import json
import os
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import needletail_amd as nt  # noqa: E402
from needletail_amd import _lib as NL  # noqa: E402

CONFIGS = ((21, 11), (15, 10), (31, 19))
ORDERS = {"lex": nt.LEX, "hash": nt.HASH}
PATH, PRE = nt.PATH_BYTES_CANONICAL, nt.PRE_NORMALIZE
READ_LEN, SEED, N_PER_1024 = 150, 0x5EED0002, 2
CHUNK = 64 << 20


def make_batch(ctx, n_reads: int):
    n_bytes = n_reads * (READ_LEN + 1)
    dev = torch.full(((n_bytes + 15) // 16 * 16 + 64,), ord("\n"), dtype=torch.uint8, device="cuda")
    ctx.synth_reads_device(SEED, 0, n_reads, READ_LEN, N_PER_1024, dev)
    off = torch.arange(n_reads + 1, dtype=torch.int64, device="cuda") * (READ_LEN + 1)
    ctx.synchronize()
    torch.cuda.synchronize()
    return dev, n_bytes, off


def timed(fn):
    torch.cuda.synchronize()
    t = time.perf_counter()
    fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t) * 1e3


def device_digest(ml, k):
    """(n_total, n_fwd, sum, xor) of the held list, folded on the device from the arrays result_device gives."""
    class View:
        def __init__(self, address, n, typestr):
            self.__cuda_array_interface__ = {"shape": (n,), "typestr": typestr, "data": (address, False), "version": 2}
    _, _, d_val, d_info, n = ml.device_arrays()
    if n == 0:
        return 0, 0, 0, 0
    values, info = torch.as_tensor(View(d_val, n, "<i8"), device="cuda"), torch.as_tensor(View(d_info, n, "<i4"), device="cuda")
    span = (info >> 1).to(torch.int64)
    odd = values[(span & 1) == 1]
    x = 0
    for bit in range(64):   # torch has no xor reduction: bit by bit
        x |= (int(((odd >> bit) & 1).sum().item()) & 1) << bit
    total = int(span.sum().item())
    fwd = int(span[(info & 1) == 0].sum().item())
    return total, fwd, int((span * values).sum().item()) & ((1 << 64) - 1), x


def bench(ctx, dev, n_bytes, off, n_reads, k, w, order, repeat):
    out = {"k": k, "w": w, "order": order, "n_reads": n_reads, "read_len": READ_LEN, "n_bytes": n_bytes}
    scratch_n = min(n_bytes, CHUNK)
    values = torch.empty((scratch_n + 15) // 16 * 16, dtype=torch.int64, device="cuda")
    valid, rc = (torch.empty((scratch_n + 15) // 16, dtype=torch.int16, device="cuda") for _ in range(2))

    def materialize():
        for start in range(0, n_bytes, CHUNK):
            ctx.materialize_device(dev[start:], min(CHUNK, n_bytes - start), k, PATH, PRE, values, valid, rc)

    def two_pass():
        ctx.accum_reset()
        ctx.reduce_device(dev, n_bytes, k, PATH, PRE, w=w)

    with nt.MinimizerList(k, PATH, w, ORDERS[order], ctx) as ml:
        run = lambda: ml.run_device(dev, n_bytes, off, n_reads, PRE)   # noqa: E731
        ctx.set_option(NL.OPT_MINIMIZER_ROUTE, NL.ROUTE_TWO_PASS)
        try:
            run()
            two_pass()
            core = ctx.accum_read()
            materialize()
            st = ml.stats()
            assert st["n_windows"] == core["n_total"], (st["n_windows"], core["n_total"])
            if order == "lex":
                total, fwd, s, x = device_digest(ml, k)
                assert (total, fwd, s, x) == (core["n_total"], core["n_fwd"], core["sum"], core["xor"]), "the list's digest is not the core's"
            times = {"list": [], "two_pass": [], "materialize": []}
            for _ in range(repeat):
                times["list"].append(timed(run))
                times["two_pass"].append(timed(two_pass))
                times["materialize"].append(timed(materialize))
        finally:
            ctx.set_option(NL.OPT_MINIMIZER_ROUTE, 0)
        for route, ts in times.items():
            out[route + "_ms"] = round(min(ts), 3)
            out[route + "_ms_all"] = [round(t, 3) for t in ts]
        out.update({key: st[key] for key in ("n_entries", "n_windows", "n_chunks", "device_bytes")})
        out["density"] = round(st["n_entries"] / max(st["n_windows"], 1), 5)
        out["density_random"] = round(2 / (w + 1), 5)
        out["gbases_per_s"] = round(n_bytes / out["list_ms"] / 1e6, 2)
        out["list_over_two_pass"] = round(out["list_ms"] / out["two_pass_ms"], 3)
        out["list_over_materialize"] = round(out["list_ms"] / out["materialize_ms"], 3)
    return out


def trace(ctx, dev, n_bytes, off, n_reads, k, w, order):
    with nt.MinimizerList(k, PATH, w, ORDERS[order], ctx) as ml:
        for _ in range(2):
            ml.run_device(dev, n_bytes, off, n_reads, PRE)
        print(json.dumps({"trace": f"{k},{w},{order}", **ml.stats()}), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reads", type=int, default=10_000_000)
    ap.add_argument("--repeat", type=int, default=5)
    ap.add_argument("--config", default=None, help="K,W: that configuration alone")
    ap.add_argument("--trace", default=None, help="K,W,ORDER, e.g. 21,11,lex")
    a = ap.parse_args()
    with nt.Context(0) as ctx:
        dev, n_bytes, off = make_batch(ctx, a.reads)
        if a.trace:
            k, w, order = a.trace.split(",")
            trace(ctx, dev, n_bytes, off, a.reads, int(k), int(w), order)
            return
        configs = [tuple(int(v) for v in a.config.split(","))] if a.config else CONFIGS
        for k, w in configs:
            for order in ORDERS:
                print(json.dumps(bench(ctx, dev, n_bytes, off, a.reads, k, w, order, a.repeat)), flush=True)


if __name__ == "__main__":
    main()
