#!/usr/bin/env python3
"""Time-budgeted structured differential fuzz of sixteen libraries in thirteen stages: the twelve k-mer libraries (count table, wide count table, HyperLogLog sketch, read
abundance, read trimmer and its batch writer, MinHash, per-record MinHash with the sketch set, k-mer set algebra narrow and wide, the
de Bruijn graph, the coloured index, the minimizer lists) and the read-mapping pipeline (seed index, chains, mappings, alignments: one
stage, `map_reads`, through ReadMapper) against the host models of tests/ - the generator and the checkers are tests/_lib_fuzz.py, whose
fixed slices run in the suite (tests/test_gpu_lib_fuzz.py).  Needs a gfx950 device, but for --dump.  --stage takes any of
`_lib_fuzz.STAGES`: count, count_wide, minhash, minhash_wide, abundance, trim, record_minhash, kmer_sets, kmer_sets_wide, dbg, colors,
minimizer_list, map_reads.

    python tools/lib_fuzz.py --seconds 180 --seed 1 > profiles/lib_fuzz/<name>.log
    python tools/lib_fuzz.py --seed 1 --stage trim --replay-it 17            # the device work of that case alone
    python tools/lib_fuzz.py --seed 1 --stage trim --replay-it 17 --dump case.npz   # its input, without a GPU
    python tools/lib_fuzz.py --seed 1 --stage colors --replay-it 5 --dump case.npz  # (a newer stage's dump also holds what it drew first)
    python tools/lib_fuzz.py --seed 1 --stage map_reads --replay-it 5 --dump case.npz   # reads, references, every drawn parameter in `extra`

Iteration N runs case N of every chosen stage; each (seed, stage, N) has a random stream of its own, so a replay draws exactly what
the run drew.  A mismatch prints "MISMATCH seed S it N stage X (k, path, pre, kinds ...)" and the settings the checker drew."""
import argparse
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

import _lib_fuzz as F  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--seconds", type=float, default=120)
    ap.add_argument("--seed", type=int, default=1)
    ap.add_argument("--stage", default="all", choices=("all",) + F.STAGES)
    ap.add_argument("--replay-it", type=int, default=0, help="do the device work of iteration N only")
    ap.add_argument("--dump", default="", help="with --replay-it and one --stage: write that case to this .npz and stop (needs no GPU)")
    args = ap.parse_args()
    stages = F.STAGES if args.stage == "all" else (args.stage,)
    if args.dump:
        if not args.replay_it or len(stages) != 1:
            ap.error("--dump needs --replay-it N and one --stage")
        _, case = F.draw_case(args.seed, stages[0], args.replay_it)
        F.dump(case, args.dump)
        print("dumped seed", args.seed, "it", args.replay_it, "stage", stages[0], case.tag(), "kinds", sorted(set(case.kinds)))
        return 0
    import torch
    import needletail_amd as nt
    ctx = nt.Context(0, stream=torch.cuda.current_stream().cuda_stream)
    sess = F.Session(ctx)
    counts = {s: 0 for s in stages}
    n_bytes, it = 0, args.replay_it - 1 if args.replay_it else 0
    t0 = time.time()
    t_end = t0 + args.seconds
    try:
        while time.time() < t_end or args.replay_it:
            it += 1
            for stage in stages:
                try:
                    case = F.run_case(sess, args.seed, stage, it)
                except F.Mismatch as e:
                    print(e)
                    return 1
                counts[stage] += 1
                n_bytes += len(case.buf())
            if args.replay_it:
                break
    finally:
        sess.close()
    print(f"lib_fuzz: seed {args.seed}, {time.time() - t0:.0f} s, {it if not args.replay_it else 1} iterations, {n_bytes / 1e6:.1f} MB, "
          f"all equal to the models: {counts}")
    return 0


if __name__ == "__main__":
    sys.exit(main())
