"""What one case of the `map_reads` stage of tests/_lib_fuzz.py contributes to the conditions of its slice, from `pipeline_want` and the
four host models alone (no GPU), and the conditions themselves.  tests/test_lib_fuzz_inputs.py asserts them over the fixed slice; the
seed search that chose the slice used the same functions."""
import numpy as np

import _align_model as AL
import _chain_model as CH
import _lib_fuzz as F
import _mapping_model as MP
import _seed_index_model as SI

# Planted wrong rules that no pipeline-born input can reach: (model, rule, why, the test that owns it).  The slice test asserts that each
# changes no case, so that this list cannot hide a catch.
EXCUSED = (
    ("align", "trust_anchors", "an anchor is a k-mer match of two minimizers, so no anchor column holds unequal bases or an N",
     "tests/test_gpu_align.py::test_ties_and_bases"),
)


def walk_cigars(case, p) -> int:
    """Every CIGAR of the run walked over its two intervals, independently of the alignment model: = on equal bases (case folded, U as
    T), X on unequal ones or a non-base, the walk ends on the mapping's ends.  Returns the number of columns that hold an N, a
    lower-case letter, a U or a junk byte."""
    rows, special = p.marks.rows, 0
    fold = np.arange(256, dtype=np.uint8)
    for a, b in zip(b"acgtUu", b"ACGTTT"):
        fold[a] = b
    comp = F.COMP[fold]
    for s, c in enumerate(p.marks.out.tolist()):
        if p.aln.rows[s, 0] != AL.ALIGNED:
            continue
        read = AL.read_of(p.inp.chains, c)
        raw = np.frombuffer(case.records[read], dtype=np.uint8)
        qs, qe, rs, re, ref_rev = (int(x) for x in rows[c, :5])
        ref_raw = np.frombuffer(case.ref_records[ref_rev >> 1], dtype=np.uint8)
        ref = fold[ref_raw]
        qry = comp[raw][::-1] if ref_rev & 1 else fold[raw]
        plain = np.isin(raw, np.frombuffer(b"ACGT", dtype=np.uint8))
        plain = plain[::-1] if ref_rev & 1 else plain
        ref_plain = np.isin(ref_raw, np.frombuffer(b"ACGT", dtype=np.uint8))
        r, q = rs, (raw.size - qe if ref_rev & 1 else qs)
        q_end = raw.size - qs if ref_rev & 1 else qe
        special += int((~plain[q:q_end]).sum()) + int((~ref_plain[rs:re]).sum())
        base = np.frombuffer(b"ACGT", dtype=np.uint8)
        for word in p.aln.cigar[int(p.aln.g_offsets[s]): int(p.aln.g_offsets[s + 1])].tolist():
            op, n = word & 15, word >> 4
            if op in (AL.OP_EQ, AL.OP_X):
                same = (ref[r: r + n] == qry[q: q + n]) & np.isin(ref[r: r + n], base)
                assert same.size == n and (same.all() if op == AL.OP_EQ else not same.any()), (s, c, r, q, op, n)
            r, q = r + n * (op != AL.OP_I), q + n * (op != AL.OP_D)
        assert (r, q) == (re, q_end), (s, c, r, q, re, q_end)
    return special


def origins_hold(case, p):
    """(checked, held) over the reads cut from a region nothing was planted in, substitutions only: where the read's rank-0 chain has at
    least three members (a chance match of one k-mer elsewhere can tie a one-seed chain at score k, and then the chain index decides),
    it lies on the origin's reference, strand and diagonal at both of its ends."""
    checked = held = 0
    rows = p.marks.rows
    for read, origin in enumerate(case.origins):
        lo, hi = int(p.chains.c_offsets[read]), int(p.chains.c_offsets[read + 1])
        if origin is None or case.kinds[read] == "dup" or lo == hi:
            continue
        c = int(p.marks.order[lo])
        qs, qe, rs, re, ref_rev, _, cnt = (int(x) for x in rows[c, :7])
        if cnt < 3:
            continue
        r, s, rev = origin
        L = len(case.records[read])
        checked += 1
        held += (ref_rev >> 1, ref_rev & 1) == (r, int(rev)) and rs - (L - qe if rev else qs) == s and re - (L - qs if rev else qe) == s
    return checked, held


def mutants_caught(case, p, skip=()) -> dict:
    """(model, rule) -> whether the planted wrong rule changes that stage's expected result on the true input of that stage (for the
    alignments: on the reported selection or on the thinned chains).  skip: rules not computed."""
    out = {}
    same = lambda a, b: all(np.asarray(x).shape == np.asarray(y).shape and np.array_equal(x, y) for x, y in zip(a, b))   # noqa: E731
    for rule in SI.MUTANTS:
        if ("seeds", rule) not in skip:
            out["seeds", rule] = not same(SI.match(p.index, p.read_list, case.extra["max_occ"], mutant=rule)[1], p.seeds)
    for rule in CH.MUTANTS:
        if ("chains", rule) not in skip:
            out["chains", rule] = not same(CH.chain(p.anchors, p.cp, mutant=rule), p.chains)
    for rule in MP.MUTANTS:
        if ("mappings", rule) not in skip:
            out["mappings", rule] = not same(MP.run(p.mch, p.mp, mutant=rule), p.marks)
    t_inp, _, t_want, _ = F.thinned_want(case)
    for rule in AL.MUTANTS:
        if ("align", rule) not in skip:
            out["align", rule] = not same(AL.run(p.inp, p.ap, mutant=rule)[0], p.aln) or not same(AL.run(t_inp, p.ap, mutant=rule)[0], t_want)
    return out


def case_report(case, skip=()) -> dict:
    p = F.pipeline_want(case)
    e, k = case.extra, case.k
    r = {}
    # seeds
    lo, hi = int(p.read_list[0][0]), int(p.read_list[0][-1])
    _, occ, hit = SI.classify(p.index, p.read_list[2][lo:hi], e["max_occ"])
    r["occ_at"] = int(((occ == e["max_occ"]) & hit).sum()) if e["max_occ"] else 0
    r["occ_above"] = int((occ == e["max_occ"] + 1).sum()) if e["max_occ"] else 0
    a_off, ref, rev = p.seeds[0].astype(np.int64), p.seeds[1], p.seeds[2]
    r["no_anchor"] = int((np.diff(a_off) == 0).sum())
    r["strands"], r["refs"] = set(rev.tolist()), set(ref.tolist())
    # chains
    runs = CH.run_lengths(p.anchors, p.cp.max_dist)
    r["long_run"] = int(sum(n > 128 for n in runs))
    off, ref_rev, rpos = (a.astype(np.int64) for a in p.anchors[:3])
    inner = np.ones(max(rpos.size - 1, 0), dtype=bool)
    inner[off[1:-1][(off[1:-1] > 0) & (off[1:-1] < rpos.size)] - 1] = False
    same_rr = ref_rev[1:] == ref_rev[:-1]
    r["split_dist"] = int((inner & same_rr & (np.diff(rpos) > p.cp.max_dist)).sum())
    r["split_ref"] = int((inner & ~same_rr).sum())
    trace = []
    CH.chain(p.anchors, p.cp, trace=trace)
    r["drop_score"] = sum(1 for t in trace if t[4] < p.cp.min_score)
    r["drop_cnt"] = sum(1 for t in trace if t[4] >= p.cp.min_score and len(t[2]) < p.cp.min_cnt)
    r["f_tie"] = bool(not np.array_equal(np.asarray(CH.recurrence(p.anchors, p.cp, "tie_smallest")[1]), p.chains.p))
    # mappings
    rr, rows = p.marks.read_rows, p.marks.rows
    eligible = np.zeros(rr.shape[0], dtype=np.int64)
    for q in range(rr.shape[0]):
        for c in range(int(p.chains.c_offsets[q]), int(p.chains.c_offsets[q + 1])):
            pc = int(rows[c, MP.W["parent"]])
            eligible[q] += pc != c and int(rows[c, MP.W["score"]]) * 1000 >= p.mp.pri_ratio_pm * int(rows[pc, MP.W["score"]])
    # a kept secondary whose score is exactly pri_ratio of its parent's: the >= of mp_eligible decides it
    r["eligible_eq"] = sum(1 for c in range(rows.shape[0]) if rows[c, MP.W["flags"]] & MP.SECONDARY and
                           int(rows[c, MP.W["score"]]) * 1000 == p.mp.pri_ratio_pm * int(rows[int(rows[c, MP.W["parent"]]), MP.W["score"]]))
    r["sec_kept"] = int((rr[:, 2] > 0).sum()) if rr.size else 0
    r["sec_cut"] = int(((eligible > rr[:, 2]) & (p.mp.best_n > 0)).sum()) if rr.size else 0
    chimera = [i for i, kind in enumerate(case.kinds) if kind == "chimera"]
    r["chimera_two"] = int(sum(rr[i, 1] >= 2 for i in chimera)) if rr.size else 0
    r["many_chains"] = int((rr[:, 0] > MP.LDS_CHAINS).sum()) if rr.size else 0
    pri = (rows[:, MP.W["flags"]] & MP.PRIMARY) != 0
    r["mapq0"], r["mapq_pos"] = int((pri & (rows[:, MP.W["mapq"]] == 0)).sum()), int((pri & (rows[:, MP.W["mapq"]] > 0)).sum())
    # alignments
    sel = p.marks.out
    r["aln_strands"] = set((p.chains.chain_rows[sel, 2] & 1).tolist()) if sel.size else set()
    flags = set(p.aln.rows[:, 0].tolist())
    r["both_flags"] = {AL.ALIGNED, AL.TOO_LONG} <= flags
    segs = [(g, s) for g in p.aligned if not g.too_long for s in g.segments]
    pure = overlap = 0
    for c, g in zip(sel.tolist(), p.aligned):
        if g.too_long:
            continue
        for (dr, dq), s in zip(AL.steps(p.inp.chains, c), g.segments):
            m0 = min(dr, dq, k)
            pure += s is None and (dr - m0 > 0 or dq - m0 > 0)
            overlap += min(dr, dq) < k
    r["pure_gap"], r["overlap"] = int(pure), int(overlap)
    dp = [s for _, s in segs if s is not None]
    r["band_edge"] = sum(1 for s in dp if s.in_band and (s.touches_lo or s.touches_hi) and p.ap.band_pad > 0 and max(s.n, s.m) > p.ap.band_pad)
    r["special"] = walk_cigars(case, p)
    _, sizes, _, t_chains = F.thinned_want(case)
    thin_dp = [s for g in t_chains if not g.too_long for s in g.segments if s is not None]
    r["band_edge"] += sum(1 for s in thin_dp if s.in_band and (s.touches_lo or s.touches_hi) and p.ap.band_pad > 0 and max(s.n, s.m) > p.ap.band_pad)
    made = [(s.n, s.m) for g in t_chains if not g.too_long for s in g.segments if s is not None]
    r["thin"] = {x for n, m in made for x in F.thin_classes(n, m)}
    r["origins"] = origins_hold(case, p)
    r["mutants"] = mutants_caught(case, p, skip)
    r["reads"], r["anchors"], r["n_chains"], r["reported"] = len(case.records), int(rpos.size), int(rows.shape[0]), int(sel.size)
    return r


THIN_WANT = {(axis, size) for axis in "nm" for size in F.THIN_SIZES} | {"cross"}


def slice_report(reports) -> dict:
    reports = list(reports)
    total = lambda name: sum(int(r[name]) for r in reports)   # noqa: E731
    union = lambda name: set().union(*(r[name] for r in reports))   # noqa: E731
    out = {name: total(name) for name in ("occ_at", "occ_above", "no_anchor", "long_run", "split_dist", "split_ref", "drop_score", "drop_cnt", "f_tie",
                                          "sec_kept", "sec_cut", "eligible_eq", "chimera_two", "many_chains", "mapq0", "mapq_pos", "both_flags", "pure_gap",
                                          "overlap", "band_edge", "special")}
    out.update(strands=union("strands"), refs=union("refs"), aln_strands=union("aln_strands"), thin=union("thin"),
               origins=(sum(r["origins"][0] for r in reports), sum(r["origins"][1] for r in reports)),
               mutants={key: sum(r["mutants"].get(key, 0) for r in reports) for key in all_mutants()})
    return out


def all_mutants():
    return [(model, rule) for model, rules in (("seeds", SI.MUTANTS), ("chains", CH.MUTANTS), ("mappings", MP.MUTANTS), ("align", AL.MUTANTS))
            for rule in rules]


def conditions(r) -> list:
    """The conditions of the slice that do not hold (none: the slice means something)."""
    miss = [name for name in ("occ_at", "occ_above", "no_anchor", "long_run", "split_dist", "split_ref", "drop_score", "drop_cnt", "f_tie", "sec_kept",
                              "sec_cut", "eligible_eq", "chimera_two", "many_chains", "mapq0", "mapq_pos", "both_flags", "pure_gap", "overlap", "band_edge", "special")
            if r[name] < 1]
    if r["strands"] != {0, 1} or len(r["refs"]) < 2 or r["aln_strands"] != {0, 1}:
        miss.append("anchors and alignments on both strands, anchors on more than one reference")
    if not r["thin"] >= THIN_WANT:
        miss.append(f"thinned sizes {sorted(map(str, THIN_WANT - r['thin']))}")
    if r["origins"][0] < 3 or r["origins"][0] != r["origins"][1]:
        miss.append(f"origins {r['origins']}")
    excused = {(m, rule) for m, rule, _, _ in EXCUSED}
    miss += [f"mutant {key}" for key, n in r["mutants"].items() if (n < 1) != (key in excused)]
    return miss
