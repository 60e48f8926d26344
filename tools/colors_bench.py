"""What screening reads against several references costs (include/needletail_amd_colors.h), on the host clock (both calls end
synchronised): one process, a warm-up, best of --reps, the two routes alternating inside the process.

Workload: k = 21; C = 8 references of --ref-len bases (default 2 Mb) derived from one random genome by 1 % substitutions each, so most
k-mers are shared by several colours and some are private; --reads (default 2 M) reads of 150 bp with 1 % errors, sampled from the
eight, resident on the device.

  (a) one pass:     one KmerColors.run_device with the single matrix, against an index of the eight references;
  (b) eight passes: the route without the index for the hits columns alone - eight ReadAbundance.run_device calls on eight count
                    tables, rows left on the device.
  (c) colours:      the one-pass call at n_colors = 1, 8 and 64 (the eight references spread over the colours), to show what the
                    colour loops cost.

Prints one JSON line per measurement and a last line with the ratio; exits 1 if the one pass is not faster than the eight (the gate).
--quick: one repetition, for a kernel-trace run (rocprofv3 --kernel-trace --stats -- python tools/colors_bench.py --quick), whose
per-kernel totals put the core's materialise kernel beside kc_*."""
import argparse
import json
import os
import sys
import time

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import needletail_amd as nt  # noqa: E402

K, PATH, PRE, READ_LEN = 21, nt.PATH_BYTES_CANONICAL, nt.PRE_NORMALIZE, 150


def substituted(seq, rate, gen):
    """`seq` (uint8 codes 0..3 on the device) with a share `rate` of its bases replaced by one of the three others."""
    hit = torch.rand(seq.shape, device=seq.device, generator=gen) < rate
    shift = torch.randint(1, 4, seq.shape, device=seq.device, generator=gen, dtype=torch.uint8)
    return torch.where(hit, (seq + shift) & 3, seq)


def workload(n_refs, ref_len, n_reads, seed=0xC0105):
    """(references as device batches [(tensor, n_bytes)], the reads' batch, its n_bytes, its offsets)."""
    gen = torch.Generator(device="cuda").manual_seed(seed)
    letters = torch.tensor(list(b"ACGT"), dtype=torch.uint8, device="cuda")
    genome = torch.randint(0, 4, (ref_len,), device="cuda", generator=gen, dtype=torch.uint8)
    refs = torch.stack([substituted(genome, 0.01, gen) for _ in range(n_refs)])
    which = torch.randint(0, n_refs, (n_reads,), device="cuda", generator=gen)
    start = torch.randint(0, ref_len - READ_LEN + 1, (n_reads,), device="cuda", generator=gen)
    n_bytes = n_reads * (READ_LEN + 1)
    batch = torch.full((n_bytes + 1024,), ord("\n"), dtype=torch.uint8, device="cuda")
    rows = batch[:n_bytes].view(n_reads, READ_LEN + 1)
    step = 1 << 18   # the gather's index tensor in pieces
    for lo in range(0, n_reads, step):
        hi = min(lo + step, n_reads)
        at = start[lo:hi, None] + torch.arange(READ_LEN, device="cuda")[None, :]
        codes = substituted(refs[which[lo:hi, None], at], 0.01, gen)
        rows[lo:hi, :READ_LEN] = letters[codes.long()]
    ref_batches = []
    for c in range(n_refs):
        t = torch.full((ref_len + 1 + 1024,), ord("\n"), dtype=torch.uint8, device="cuda")
        t[:ref_len] = letters[refs[c].long()]
        ref_batches.append((t, ref_len + 1))
    offsets = torch.arange(n_reads + 1, dtype=torch.int64, device="cuda") * (READ_LEN + 1)
    torch.cuda.synchronize()
    return ref_batches, batch, n_bytes, offsets


def timed(fn, reps):
    """Milliseconds of each of `reps` calls after one warm-up (which allocates the scratch)."""
    out = []
    for r in range(reps + 1):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        fn()
        if r:
            out.append((time.perf_counter() - t0) * 1e3)
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--quick", action="store_true")
    ap.add_argument("--reads", type=int, default=2_000_000)
    ap.add_argument("--ref-len", type=int, default=2_000_000)
    ap.add_argument("--colors", type=int, nargs="+", default=[1, 8, 64])
    a = ap.parse_args()
    reps, n_refs = (1 if a.quick else a.reps), 8
    ctx = nt.Context(0, stream=torch.cuda.current_stream().cuda_stream)
    ref_batches, batch, n_bytes, offsets = workload(n_refs, a.ref_len, a.reads)
    tables, sets = [], []
    for dev, nb in ref_batches:
        t = nt.KmerTable(K, PATH, nb, ctx)
        t.count_device(dev, nb, PRE)
        assert t.stats()["n_dropped"] == 0
        tables.append(t)
        sets.append(nt.KmerSet.from_table(t))
    abund = [nt.ReadAbundance(t) for t in tables]
    kc = nt.KmerColors.from_sets(sets)
    st = kc.stats()
    assert st["n_dropped"] == 0
    shared = st["n_keys"] and sum(st["per_color"]) / st["n_keys"]

    one_pass = lambda: kc.run_device(batch, n_bytes, offsets, a.reads, PRE, single=True)                      # noqa: E731
    eight = lambda: [ra.run_device(batch, n_bytes, offsets, a.reads, PRE) for ra in abund]                      # noqa: E731
    # what came back, as a plausibility check of the run itself (the tests hold the answers to the model)
    rows, hits, _ = one_pass()
    columns = eight()
    for c in range(n_refs):
        assert torch.equal(hits[:, c], columns[c][:, 1]) and torch.equal(rows[:, 0], columns[c][:, 0]), c
    del columns
    a_ms, b_ms = [], []
    for _ in range(reps):   # alternating
        a_ms += timed(one_pass, 1)
        b_ms += timed(eight, 1)
    base = {"k": K, "n_reads": a.reads, "read_len": READ_LEN, "bases": n_bytes, "ref_len": a.ref_len, "n_keys": st["n_keys"],
            "colours_per_key": round(shared, 3), "slots": st["slots"]}
    print(json.dumps({"route": "one pass, n_colors = 8, with single", **base, "ms": round(min(a_ms), 3),
                      "all_ms": [round(v, 3) for v in a_ms], "gbases_per_s": round(n_bytes / min(a_ms) / 1e6, 2),
                      "assigned": int((rows[:, 3] >= 0).sum()), "n_hit": int(rows[:, 1].sum())}), flush=True)
    print(json.dumps({"route": "eight ReadAbundance passes", **base, "ms": round(min(b_ms), 3), "all_ms": [round(v, 3) for v in b_ms],
                      "gbases_per_s": round(n_bytes / min(b_ms) / 1e6, 2)}), flush=True)
    for ra in abund:
        ra.close()
    for n_colors in a.colors:
        with nt.KmerColors(K, PATH, n_colors, sum(len(s) for s in sets), ctx) as other:
            for i, s in enumerate(sets):   # reference i under colours i, i + 8, ... (all of them under colour 0 when there is one)
                for color in sorted({c for c in range(i % n_colors, n_colors, n_refs)}):
                    other.add(s, color)
            for single in (True, False):
                ms = timed(lambda: other.run_device(batch, n_bytes, offsets, a.reads, PRE, single=single), reps)
                print(json.dumps({"route": f"one pass, n_colors = {n_colors}, {'with' if single else 'without'} single", "ms": round(min(ms), 3),
                                  "all_ms": [round(v, 3) for v in ms]}), flush=True)
    ok = min(a_ms) < min(b_ms)
    print(json.dumps({"gate": "one pass faster than eight passes", "one_pass_ms": round(min(a_ms), 3), "eight_passes_ms": round(min(b_ms), 3),
                      "ratio": round(min(b_ms) / min(a_ms), 2), "holds": ok}), flush=True)
    kc.close()
    for t in tables:
        t.close()
    ctx.close()
    return 0 if ok else 1


if __name__ == "__main__":
    sys.exit(main())
