"""Quality masking on byte-path input that was not normalised and at k > 32, at config-2 size (10 M x 150 bp, 1.51 GB, Phred+33 qualities of
good reads: 3 % below Q20), cutoff 53: kernel time of
  * k = 21, PRE_NONE with the quality stream next to PRE_NORMALIZE with it, alternating in the same loop (the speculative packed-value scan
    against the scan it speculates on);
  * k = 21, PRE_NONE with the quality stream when one unmasked lower-case base sends the launch to the byte-walking kernel (the redo);
  * k = 64, PRE_NONE, with and without the quality stream;
  * NTK_ROUTE_NO_SPECULATION (the byte-walking kernel alone) for both k.
Times are the hipEvent spans the library records (enable_timing), after 400 launches of preheat per configuration.
Run on the GPU box: python tools/quality_raw_bench.py [--reads N] [--cutoff C] [--steps S]"""
import argparse
import json
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import needletail_amd as nt  # noqa: E402
from needletail_amd import _lib as NL  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--reads", type=int, default=10_000_000)
ap.add_argument("--cutoff", type=int, default=53)   # Phred 20
ap.add_argument("--steps", type=int, default=20)
ap.add_argument("--preheat", type=int, default=400)
args = ap.parse_args()
L = 150
n = args.reads * (L + 1)
ctx = nt.Context(0, stream=torch.cuda.current_stream().cuda_stream)
seq = torch.empty(n + 2048, dtype=torch.uint8, device="cuda")
ctx.synth_reads_device(0x5EED0002, 0, args.reads, L, 1, seq)
g = torch.Generator(device="cuda"); g.manual_seed(53)
qual = torch.randint(53, 75, (n + 2048,), dtype=torch.uint8, device="cuda", generator=g)
low = torch.rand(n + 2048, device="cuda", generator=g) < 0.03
qual[low] = torch.randint(33, 53, (int(low.sum()),), dtype=torch.uint8, device="cuda", generator=g)
del low
# one lower-case base under a good quality, half way through the batch
seq_lc = seq.clone()
mid = n // 2
pos = mid + int(torch.nonzero((seq[mid: mid + 4096] == ord("A")) & (qual[mid: mid + 4096] >= args.cutoff))[0])
seq_lc[pos] = ord("a")
P = nt.PATH_BYTES_CANONICAL
Q = {"d_qual": qual, "quality_cutoff": args.cutoff}


def launch(cfg):
    s, k, pre, kw, route = cfg
    ctx.set_option(NL.OPT_MINIMIZER_ROUTE, route)
    ctx.reduce_device(s, n, k, P, pre, reset=True, **kw)


def timed(cfgs):
    """Preheat each configuration, then `steps` rounds of one launch each, round-robin; ms per launch and the result of each."""
    for cfg in cfgs:
        for _ in range(args.preheat):
            launch(cfg)
    torch.cuda.synchronize()
    tot = [0.0] * len(cfgs)
    ctx.scan_time_ms()
    for _ in range(args.steps):
        for i, cfg in enumerate(cfgs):
            ctx.enable_timing(True)
            launch(cfg)
            ms, launches = ctx.scan_time_ms()
            ctx.enable_timing(False)
            tot[i] += ms / launches
    out = []
    for i, cfg in enumerate(cfgs):
        with_redo = torch.zeros(NL.ACC_WORDS, dtype=torch.int64, device="cuda")
        ctx.accum_bind_device(with_redo)
        launch(cfg)
        ctx.synchronize()
        ctx.accum_bind_device(None)
        launch(cfg)
        st = ctx.accum_read()
        out.append({"kernel_ms": round(tot[i] / args.steps, 4), "gbases_s": round(args.reads * L / (tot[i] / args.steps) / 1e6, 1),
                    "n_total": int(st["n_total"]), "redone": int(with_redo[NL.ACC_REDONE])})
    ctx.set_option(NL.OPT_MINIMIZER_ROUTE, 0)
    return out


res = {}
a, b = timed([(seq, 21, nt.PRE_NORMALIZE, Q, 0), (seq, 21, nt.PRE_NONE, Q, 0)])
res["k21_normalize_quality"], res["k21_none_quality"] = a, b
res["k21_none_quality_over_normalize"] = round(b["kernel_ms"] / a["kernel_ms"], 4)
res["k21_none_quality_redo"], = timed([(seq_lc, 21, nt.PRE_NONE, Q, 0)])
a, b = timed([(seq, 64, nt.PRE_NONE, {}, 0), (seq, 64, nt.PRE_NONE, Q, 0)])
res["k64_none"], res["k64_none_quality"] = a, b
a, b = timed([(seq, 21, nt.PRE_NONE, Q, NL.ROUTE_NO_SPECULATION), (seq, 64, nt.PRE_NONE, Q, NL.ROUTE_NO_SPECULATION)])
res["k21_none_quality_no_speculation"], res["k64_none_quality_no_speculation"] = a, b
assert res["k21_none_quality"]["n_total"] == res["k21_normalize_quality"]["n_total"] == res["k21_none_quality_no_speculation"]["n_total"]
assert res["k64_none_quality"]["n_total"] == res["k64_none_quality_no_speculation"]["n_total"]
ctx.close()
print(json.dumps({"workload": f"{args.reads} x {L} bp, cutoff {args.cutoff}, 3 % of qualities below Q20", **res}))
