"""The host model of the alignment library (include_pending/needletail_amd/align.h): the rule in plain Python integers, written from the
header's text, and the device memory the header states.  An input is the two batches (bytes and record starts), the chains of the reads
(c_offsets, chain_rows, m_offsets, members, rpos, qpos, the shape AnchorChains and SeedIndex hand out) and the selection.

`fill` is the rule cell by cell and the definition; `fill_fast` sweeps anti-diagonals with numpy so that a 4095 x 4095 part takes a
second, and tests/test_align_model.py holds it to `fill`.  The traceback walks the three matrices, borders included, and reports every
cell it visits.  The `mutant` arguments restate six wrong libraries (tests/test_align_model.py shows that the GPU cases tell each of them
from the right one)."""
import collections

import numpy as np

OK, ERR_BAD_ARG, ERR_CAPACITY, ERR_UNSUPPORTED = 0, 2, 5, 6
THREADS = 256             # ALN_THREADS of csrc/ntk_align_rule.hpp
BLOCKS_PER_CU = 8         # ALN_BLOCKS_PER_CU
SEG_MAX = 4095            # ALN_SEG_MAX
SPAN_MAX = 1 << 28        # ALN_SPAN_MAX
CTR_WORDS = 7             # kCtrWords of csrc/ntk_align.hip
NEG = -(1 << 40)          # minus infinity; the library's is -2^29, and no result depends on which
STATS = ("n_sel", "n_aligned", "n_too_long", "n_segments", "n_dp_segments", "dp_cells", "n_cigar", "n_groups", "device_bytes")
FIELDS = ("rows", "scores", "g_offsets", "cigar")
ROW = ("flags", "n_cigar", "n_eq", "n_x", "n_ins", "n_del", "n_gaps", "zero")
ALIGNED, TOO_LONG = 1, 2
OP_I, OP_D, OP_EQ, OP_X = 1, 2, 7, 8
OPS = {OP_I: "I", OP_D: "D", OP_EQ: "=", OP_X: "X"}
MUTANTS = ("extend_first", "ins_first", "band_narrow", "no_complement", "trust_anchors", "no_merge")
U64, U32, U8 = np.uint64, np.uint32, np.uint8

Params = collections.namedtuple("Params", "k a b q e band_pad max_seg work_mib", defaults=(2, 4, 4, 2, 64, 2048, 0))
Result = collections.namedtuple("Result", FIELDS)
Batch = collections.namedtuple("Batch", "data offsets")
Chains = collections.namedtuple("Chains", "c_offsets chain_rows m_offsets members rpos qpos")
Input = collections.namedtuple("Input", "refs reads chains sel")

CODE = np.full(256, 4, dtype=np.int64)
for _i, _pair in enumerate((b"Aa", b"Cc", b"Gg", b"TtUu")):
    for _c in _pair:
        CODE[_c] = _i


def pack(records, brk=b"\n"):
    """A batch: the records back to back, each followed by one break byte, and their starts."""
    data = b"".join(bytes(r) + brk for r in records)
    return Batch(np.frombuffer(data, dtype=U8).copy(), np.cumsum([0] + [len(r) + 1 for r in records]).astype(U64))


def chains_of(reads):
    """The chains of a batch of reads, each a list of chains (score, ref_rev, [(rpos, qpos), ...]); every chain's anchors are its own."""
    flat = [c for r in reads for c in r]
    anchors = [a for _, _, m in flat for a in m]
    return Chains(np.cumsum([0] + [len(r) for r in reads]).astype(U64),
                  np.asarray([[score, len(m), ref_rev, 0, 0, 0, 0, 0] for score, ref_rev, m in flat], dtype=U32).reshape(-1, 8),
                  np.cumsum([0] + [len(m) for _, _, m in flat]).astype(U64), np.arange(len(anchors), dtype=U32),
                  np.asarray([a[0] for a in anchors], dtype=U32), np.asarray([a[1] for a in anchors], dtype=U32))


def cigar_string(words):
    return "".join("%d%s" % (int(w) >> 4, OPS[int(w) & 15]) for w in words)


def record_len(batch, r):
    return max(int(batch.offsets[r + 1]) - int(batch.offsets[r]), 1) - 1


def check_params(p):
    """What run_device refuses before any device call."""
    ok = (1 <= p.k <= 255 and 1 <= p.a <= 255 and 1 <= p.b <= 255 and 0 <= p.q <= 255 and 1 <= p.e <= 255 and 0 <= p.band_pad <= 4095 and
          1 <= p.max_seg <= 4095 and (p.work_mib == 0 or 16 <= p.work_mib <= 4096))
    return OK if ok else ERR_BAD_ARG


def work_bytes(p):
    return (p.work_mib or 256) << 20


def members_of(ch, c):
    return ch.members[int(ch.m_offsets[c]): int(ch.m_offsets[c + 1])].tolist()


def steps(ch, c):
    """(dr, dq) of the consecutive members of chain c, dq taken strand-wise."""
    m, rev = members_of(ch, c), int(ch.chain_rows[c, 2]) & 1
    return [(int(ch.rpos[i]) - int(ch.rpos[j]), int(ch.qpos[j]) - int(ch.qpos[i]) if rev else int(ch.qpos[i]) - int(ch.qpos[j]))
            for j, i in zip(m, m[1:])]


def read_of(ch, c):
    """The read of chain c."""
    return int(np.searchsorted(ch.c_offsets, c, side="right")) - 1


def verify(inp, p):
    """The status of the verification of the arrays."""
    refs, reads, ch, sel = inp
    n_refs, n_reads, n_chains, n_members, n_anchors = refs.offsets.size - 1, reads.offsets.size - 1, ch.chain_rows.shape[0], ch.members.size, ch.rpos.size
    assert ch.c_offsets.size == n_reads + 1 and ch.m_offsets.size == n_chains + 1
    for off, top in ((refs.offsets, refs.data.size), (reads.offsets, reads.data.size), (ch.c_offsets, n_chains)):
        o = off.tolist()
        if any(x > y for x, y in zip(o, o[1:])) or o[-1] > top:
            return ERR_BAD_ARG
    unsupported = False
    mo = ch.m_offsets.tolist()
    for c in sel.tolist():
        if c >= n_chains or not int(ch.c_offsets[0]) <= c < int(ch.c_offsets[-1]):
            return ERR_BAD_ARG
        if not mo[c] <= mo[c + 1] <= n_members or mo[c] == mo[c + 1] or not 1 <= int(ch.chain_rows[c, 0]) < 1 << 31:
            return ERR_BAD_ARG
        m = members_of(ch, c)
        if any(i >= n_anchors for i in m) or any(dr < 1 or dq < 1 for dr, dq in steps(ch, c)):
            return ERR_BAD_ARG
        ref = int(ch.chain_rows[c, 2]) >> 1
        if ref >= n_refs:
            return ERR_BAD_ARG
        rs, re = int(ch.rpos[m[0]]), int(ch.rpos[m[-1]]) + p.k
        q = (int(ch.qpos[m[0]]), int(ch.qpos[m[-1]]))
        qs, qe = min(q), max(q) + p.k
        if re > record_len(refs, ref) or qe > record_len(reads, read_of(ch, c)):
            return ERR_BAD_ARG
        if re - rs >= SPAN_MAX or qe - qs >= SPAN_MAX:
            unsupported = True
    return ERR_UNSUPPORTED if unsupported else OK


# ---- one between part ---------------------------------------------------------------------------------------------------------------------

def band(n, m, band_pad, mutant=None):
    pad = band_pad - 1 if mutant == "band_narrow" and band_pad else band_pad
    return min(0, m - n) - pad, max(0, m - n) + pad


def fill(ref, qry, p, mutant=None):
    """H, E and F of the between part of the code lists ref against qry, (n + 1) x (m + 1) each, cell by cell as the rule states them."""
    n, m = len(ref), len(qry)
    lo, hi = band(n, m, p.band_pad, mutant)
    H = [[NEG] * (m + 1) for _ in range(n + 1)]
    E = [[NEG] * (m + 1) for _ in range(n + 1)]
    F = [[NEG] * (m + 1) for _ in range(n + 1)]
    H[0][0] = 0
    for i in range(n + 1):
        for j in range(m + 1):
            if (i == 0 and j == 0) or not lo <= j - i <= hi:
                continue
            best = NEG
            if i > 0:
                E[i][j] = max(E[i - 1][j], H[i - 1][j] - p.q) - p.e
                best = max(best, E[i][j])
            if j > 0:
                F[i][j] = max(F[i][j - 1], H[i][j - 1] - p.q) - p.e
                best = max(best, F[i][j])
            if i > 0 and j > 0:
                s = p.a if ref[i - 1] == qry[j - 1] and ref[i - 1] < 4 else -p.b
                best = max(best, H[i - 1][j - 1] + s)
            H[i][j] = max(best, NEG)
    return H, E, F


def fill_fast(ref, qry, p, mutant=None):
    """fill() with numpy, one anti-diagonal at a time."""
    n, m = len(ref), len(qry)
    lo, hi = band(n, m, p.band_pad, mutant)
    r, q = np.asarray(ref, dtype=np.int64), np.asarray(qry, dtype=np.int64)
    H, E, F = (np.full((n + 1, m + 1), NEG, dtype=np.int64) for _ in range(3))
    H[0, 0] = 0
    for j in range(1, min(m, hi) + 1):
        F[0, j] = H[0, j] = -(p.q + j * p.e)
    for i in range(1, min(n, -lo) + 1):
        E[i, 0] = H[i, 0] = -(p.q + i * p.e)
    for d in range(2, n + m + 1):
        # cells (i, d - i) with 1 <= i <= n, 1 <= d - i <= m and lo <= d - 2 i <= hi
        i = np.arange(max(1, d - m, -((hi - d) // 2)), min(n, d - 1, (d - lo) // 2) + 1)
        if not i.size:
            continue
        j = d - i
        e = np.maximum(E[i - 1, j], H[i - 1, j] - p.q) - p.e
        f = np.maximum(F[i, j - 1], H[i, j - 1] - p.q) - p.e
        s = np.where((r[i - 1] == q[j - 1]) & (r[i - 1] < 4), p.a, -p.b)
        E[i, j], F[i, j] = e, f
        H[i, j] = np.maximum(np.maximum(H[i - 1, j - 1] + s, e), f)
    return H, E, F


def trace(H, E, F, ref, qry, p, mutant=None):
    """The traceback from (n, m): the ops from the first column to the last, one per column, and the cells visited."""
    i, j, state, ops, cells = len(ref), len(qry), "H", [], []
    while i > 0 or j > 0:
        cells.append((i, j))
        h = int(H[i][j])
        if state == "H":
            s = (p.a if ref[i - 1] == qry[j - 1] and ref[i - 1] < 4 else -p.b) if i > 0 and j > 0 else None
            if s is not None and h == int(H[i - 1][j - 1]) + s:
                ops.append(OP_EQ if s == p.a else OP_X)
                i, j = i - 1, j - 1
            elif mutant == "ins_first" and j > 0 and h == int(F[i][j]):
                state = "F"
            elif i > 0 and h == int(E[i][j]):
                state = "E"
            else:
                assert j > 0 and h == int(F[i][j])
                state = "F"
        elif state == "E":
            ops.append(OP_D)
            opened, extended = int(E[i][j]) == int(H[i - 1][j]) - p.q - p.e, int(E[i][j]) == int(E[i - 1][j]) - p.e
            assert opened or extended
            if opened and not (mutant == "extend_first" and extended):
                state = "H"
            i -= 1
        else:
            ops.append(OP_I)
            opened, extended = int(F[i][j]) == int(H[i][j - 1]) - p.q - p.e, int(F[i][j]) == int(F[i][j - 1]) - p.e
            assert opened or extended
            if opened and not (mutant == "extend_first" and extended):
                state = "H"
            j -= 1
    return ops[::-1], cells


def runs_of(ops):
    """[(op, len)] of a list of ops, adjacent equal ops merged."""
    out = []
    for op in ops:
        if out and out[-1][0] == op:
            out[-1][1] += 1
        else:
            out.append([op, 1])
    return [(op, n) for op, n in out]


Segment = collections.namedtuple("Segment", "n m runs score cells touches_lo touches_hi in_band")


def segment(ref, qry, p, mutant=None, fast=None):
    """A between part with n, m >= 1: its runs, H[n][m], its cells in band with i, j >= 1, and whether the path touches the lowest and
    the highest diagonal of the band and stays inside it.  fast: fill_fast, by default where the part is large enough to gain by it."""
    n, m = len(ref), len(qry)
    fast = n * m > 2048 if fast is None else fast
    H, E, F = (fill_fast if fast else fill)(ref, qry, p, mutant)
    ops, cells = trace(H, E, F, ref, qry, p, mutant)
    lo, hi = band(n, m, p.band_pad, mutant)
    n_cells = sum(max(0, min(m, i + hi) - max(1, i + lo) + 1) for i in range(1, n + 1))
    diag = [j - i for i, j in cells] + [0]
    return Segment(n, m, runs_of(ops), int(H[n][m]), n_cells, min(diag) == lo, max(diag) == hi, all(lo <= d <= hi for d in diag))


def score_of(runs, p):
    """The score of a list of runs, as the result states it."""
    count = lambda op: sum(n for o, n in runs if o == op)   # noqa: E731
    gaps = sum(1 for o, _ in runs if o in (OP_I, OP_D))
    return p.a * count(OP_EQ) - p.b * count(OP_X) - p.q * gaps - p.e * (count(OP_I) + count(OP_D))


# ---- a chain ------------------------------------------------------------------------------------------------------------------------------

def sequences_of(inp, c, mutant=None, cache=None):
    """The codes of chain c's reference record and of its query: the read, or on the reverse strand its reverse complement.  cache: a
    dict of one run, so that a record many chains lie on is decoded once."""
    refs, reads, ch, _ = inp
    ref, rev, q = int(ch.chain_rows[c, 2]) >> 1, int(ch.chain_rows[c, 2]) & 1, read_of(ch, c)
    cache = {} if cache is None else cache
    if ("ref", ref) not in cache:
        cache["ref", ref] = CODE[refs.data[int(refs.offsets[ref]): int(refs.offsets[ref]) + record_len(refs, ref)]].tolist()
    if ("read", q, rev) not in cache:
        s = CODE[reads.data[int(reads.offsets[q]): int(reads.offsets[q]) + record_len(reads, q)]]
        if rev:
            s = s[::-1] if mutant == "no_complement" else np.where(s < 4, 3 - s, 4)[::-1]
        cache["read", q, rev] = s.tolist()
    return cache["ref", ref], cache["read", q, rev]


def parts_of(inp, c, p):
    """The pieces of chain c in reference-forward coordinates: ("diag", r, q, columns) and ("between", r, q, n, m)."""
    ch = inp.chains
    m, rev = members_of(ch, c), int(ch.chain_rows[c, 2]) & 1
    q_len = record_len(inp.reads, read_of(ch, c))
    at = [(int(ch.rpos[i]), q_len - int(ch.qpos[i]) - p.k if rev else int(ch.qpos[i])) for i in m]
    out = []
    for (r0, q0), (r1, q1) in zip(at, at[1:]):
        m0 = min(r1 - r0, q1 - q0, p.k)
        out += [("diag", r0, q0, m0), ("between", r0 + m0, q0 + m0, r1 - r0 - m0, q1 - q0 - m0)]
    return out + [("diag", at[-1][0], at[-1][1], p.k)]


Chain = collections.namedtuple("Chain", "too_long runs segments")


def chain(inp, c, p, mutant=None, cache=None):
    """Chain c aligned: its canonical runs and its between parts (a Segment for one with DP, None for one without)."""
    parts = parts_of(inp, c, p)
    if any(part[0] == "between" and max(part[3], part[4]) > p.max_seg for part in parts):
        return Chain(True, [], [])
    ref, qry = sequences_of(inp, c, mutant, cache)
    ops, pieces, segments = [], [], []
    for part in parts:
        if part[0] == "diag":
            _, r, q, cols = part
            new = [(OP_EQ if mutant == "trust_anchors" or (ref[r + x] == qry[q + x] and ref[r + x] < 4) else OP_X, 1) for x in range(cols)]
        else:
            _, r, q, n, m = part
            if n and m:
                segments.append(segment(ref[r: r + n], qry[q: q + m], p, mutant))
                new = segments[-1].runs
            else:
                segments.append(None)
                new = [(OP_D, n)] * (n > 0) + [(OP_I, m)] * (m > 0)
        pieces.append(runs_merged(new))
        ops += new
    runs = [r for piece in pieces for r in piece] if mutant == "no_merge" else runs_merged(ops)
    return Chain(False, runs, segments)


def runs_merged(runs):
    out = []
    for op, n in runs:
        if out and out[-1][0] == op:
            out[-1] = (op, out[-1][1] + n)
        elif n:
            out.append((op, n))
    return out


def run(inp, p, mutant=None):
    """The whole result of run_device, and the stats without device_bytes; .chains holds every entry's Chain."""
    assert verify(inp, p) == OK and check_params(p) == OK
    rows, scores, g_offsets, cigar, chains, cache = [], [], [0], [], [], {}
    for c in inp.sel.tolist():
        got = chain(inp, c, p, mutant, cache)
        chains.append(got)
        count = lambda op: sum(n for o, n in got.runs if o == op)   # noqa: E731
        rows.append([TOO_LONG, 0, 0, 0, 0, 0, 0, 0] if got.too_long else
                    [ALIGNED, len(got.runs), count(OP_EQ), count(OP_X), count(OP_I), count(OP_D), sum(1 for o, _ in got.runs if o in (OP_I, OP_D)), 0])
        scores.append(0 if got.too_long else score_of(got.runs, p))
        cigar += [n << 4 | op for op, n in got.runs]
        g_offsets.append(len(cigar))
    result = Result(np.asarray(rows, dtype=U32).reshape(-1, 8), np.asarray(scores, dtype=np.int64), np.asarray(g_offsets, dtype=U64),
                    np.asarray(cigar, dtype=U32))
    return result, chains


def segment_bytes(inp, p, chains):
    """Per segment of every selected chain, in order: (direction bytes, run bound), both 0 for a part without DP or a chain too long."""
    out = []
    for c, got in zip(inp.sel.tolist(), chains):
        n_seg = int(inp.chains.m_offsets[c + 1]) - int(inp.chains.m_offsets[c]) - 1
        for t in range(n_seg):
            seg = None if got.too_long else got.segments[t]
            if seg is None:
                out.append((0, 0))
            else:
                lo, hi = band(seg.n, seg.m, p.band_pad)
                out.append((seg.n * min(hi - lo + 1, seg.m), seg.n + seg.m))
    return out


def groups(sizes, limit):
    """The consecutive groups of segments whose direction bytes fit `limit`: [(first, end, bytes)]."""
    out, lo = [], 0
    while lo < len(sizes):
        hi, total = lo, 0
        while hi < len(sizes) and total + sizes[hi] <= limit:
            total, hi = total + sizes[hi], hi + 1
        assert hi > lo
        out.append((lo, hi, total))
        lo = hi
    return out


def stats(inp, p, result, chains):
    """The stats without device_bytes."""
    live = [g for g in chains if not g.too_long]
    dp = [s for g in live for s in g.segments if s is not None]
    sizes = [b for b, _ in segment_bytes(inp, p, chains)]
    return {"n_sel": inp.sel.size, "n_aligned": len(live), "n_too_long": len(chains) - len(live), "n_segments": sum(len(g.segments) for g in live),
            "n_dp_segments": len(dp), "dp_cells": sum(s.cells for s in dp), "n_cigar": result.cigar.size,
            "n_groups": len(groups(sizes, work_bytes(p))) if dp else 0}


def held(inp, p, result, chains):
    """The sizes device_bytes takes, of one run."""
    seg = segment_bytes(inp, p, chains)
    has_dp = any(b for b, _ in seg)
    return dict(n_sel=inp.sel.size, n_seg=len(seg), n_runs=sum(r for _, r in seg), n_cigar=result.cigar.size,
                dir_bytes=max(g[2] for g in groups([b for b, _ in seg], work_bytes(p))) if has_dp else 0)


EMPTY_STATS = dict.fromkeys(STATS[:-1], 0)


def device_bytes(n_sel=None, n_seg=0, n_runs=0, n_cigar=0, dir_bytes=0):
    """stats.device_bytes of a handle since its last trim, term by term as the header states them; every argument is the largest of the
    runs since then (every array grows to exactly the largest size needed so far).  The counter words; then, with any run: the result,
    32 + 8 + 8 B per selected chain and 8 more (the rows, scores and g_offsets) and 4 B per CIGAR word; the work arrays, 8 B per selected
    chain and 8 more (its first segment), 32 B per segment and 28 more, 4 B per run bound, the direction bytes of the largest group.
    rocPRIM's temporary storage is held inside a call only: no term."""
    if n_sel is None:
        return 0
    return 8 * CTR_WORDS + 48 * n_sel + 8 + 4 * n_cigar + 8 * n_sel + 8 + 32 * n_seg + 28 + 4 * n_runs + dir_bytes
