"""The host model of the chain library (include_pending/needletail_amd/chain.h): the rule in plain Python, written from the header's
text, and the device memory the header states.  The anchors of a batch are (offsets, ref_rev, rpos, qpos) as numpy arrays, the shape
SeedIndex hands out on the device.

The recurrence and the backtrack know nothing of runs: runs are counted for the stats alone.  tests/test_chain_model.py holds the model
to the issue's fixtures and to an explicit enumeration of predecessor paths; the GPU tests hold the library to it.  The `mutant`
arguments restate eight wrong libraries (tests/test_chain_inputs.py shows that the GPU cases tell each of them from the right one)."""
import collections

import numpy as np

OK, ERR_BAD_ARG, ERR_CAPACITY, ERR_UNSUPPORTED = 0, 2, 5, 6
THREADS = 256             # CH_THREADS of csrc/ntk_chain_rule.hpp
BLOCKS_PER_CU = 8         # CH_BLOCKS_PER_CU
RING = 512                # CH_RING = CH_H_MAX
READ_ANCHORS = 1 << 23    # CH_READ_ANCHORS
NONE = 0xFFFFFFFF
CTR_WORDS = 4             # kCtrWords of csrc/ntk_chain.hip
STATS = ("n_reads", "n_anchors", "n_runs", "longest_run", "n_chains", "n_members", "reserved", "device_bytes")
FIELDS = ("c_offsets", "chain_rows", "m_offsets", "members", "f", "p", "read_rows")
MUTANTS = ("tie_smallest", "bw_lt", "max_dist_lt", "window_short", "seam_lane", "run_split_ge", "dropped_unused", "stop_not_subtracted")
U64, U32, I32 = np.uint64, np.uint32, np.int32

Params = collections.namedtuple("Params", "k max_dist bw h min_score min_cnt r0 r1", defaults=(5000, 500, 64, 40, 3, 0, 0))
Result = collections.namedtuple("Result", FIELDS)


def as_anchors(offsets, ref_rev, rpos, qpos):
    return (np.asarray(offsets, dtype=U64), np.asarray(ref_rev, dtype=U32), np.asarray(rpos, dtype=U32), np.asarray(qpos, dtype=U32))


def one_read(triples):
    """One read of the anchors (ref_rev, rpos, qpos), in the order given."""
    t = list(triples)
    return as_anchors([0, len(t)], [a[0] for a in t], [a[1] for a in t], [a[2] for a in t])


def reads_of(lists):
    """A batch of reads, each a list of (ref_rev, rpos, qpos)."""
    flat = [a for t in lists for a in t]
    return as_anchors(np.cumsum([0] + [len(t) for t in lists]), [a[0] for a in flat], [a[1] for a in flat], [a[2] for a in flat])


def check_params(p):
    """What run_device refuses before any device call."""
    ok = (1 <= p.k <= 255 and 1 <= p.max_dist <= (1 << 31) - 1 and 0 <= p.bw <= p.max_dist and 1 <= p.h <= RING and
          1 <= p.min_score < 1 << 32 and 1 <= p.min_cnt < 1 << 32 and p.r0 == 0 and p.r1 == 0)
    return OK if ok else ERR_BAD_ARG


def verify(anchors):
    """The status of the verification of the arrays."""
    off, ref_rev, rpos, qpos = anchors
    n, n_reads = rpos.size, off.size - 1
    if n >= 1 << 32 or n_reads >= 1 << 31:
        return ERR_BAD_ARG
    if np.any(off[1:] < off[:-1]) or int(off[-1]) > n:
        return ERR_BAD_ARG
    for q in range(n_reads):
        t = list(zip(ref_rev[int(off[q]): int(off[q + 1])].tolist(), rpos[int(off[q]): int(off[q + 1])].tolist(), qpos[int(off[q]): int(off[q + 1])].tolist()))
        if any(not a < b for a, b in zip(t, t[1:])):
            return ERR_BAD_ARG
    if np.any(np.diff(off.astype(np.int64)) >= READ_ANCHORS):
        return ERR_UNSUPPORTED
    return OK


def ilog2(v):
    return v.bit_length() - 1


def gap_cost(dd, k):
    return 0 if dd == 0 else ((dd * k * 41) >> 12) + (ilog2(dd) >> 1)


def pair(rev, rj, qj, ri, qi, p, mutant=None):
    """None where j = (rj, qj) may not precede i = (ri, qi), else (gain, gap)."""
    dr = ri - rj
    dq = qj - qi if rev else qi - qj
    far = (lambda d: d >= p.max_dist) if mutant == "max_dist_lt" else (lambda d: d > p.max_dist)
    if dr < 1 or dq < 1 or far(dr) or far(dq):
        return None
    dd = abs(dr - dq)
    if dd >= p.bw if mutant == "bw_lt" else dd > p.bw:
        return None
    return min(dr, dq, p.k), gap_cost(dd, p.k)


def _run_ids(ref_rev, rpos, lo, hi, max_dist, mutant=None):
    """The run of every anchor of the read [lo, hi), numbered from 0 within the read."""
    ids, r = [], -1
    for i in range(lo, hi):
        gap = rpos[i] - rpos[i - 1] if i > lo else 0
        if i == lo or ref_rev[i] != ref_rev[i - 1] or (gap >= max_dist if mutant == "run_split_ge" else gap > max_dist):
            r += 1
        ids.append(r)
    return ids


def recurrence(anchors, p, mutant=None):
    """f and p of every anchor (lists; anchors of no read: 0 and NONE)."""
    off, ref_rev, rpos, qpos = (a.tolist() for a in anchors)
    n = len(rpos)
    f, pred = [0] * n, [NONE] * n
    h = p.h - 1 if mutant == "window_short" else p.h
    for q in range(len(off) - 1):
        lo, hi = off[q], off[q + 1]
        ids = _run_ids(ref_rev, rpos, lo, hi, p.max_dist, mutant) if mutant == "run_split_ge" else None
        for i in range(lo, hi):
            best, at = p.k, NONE
            for j in range(i - 1, max(lo, i - h) - 1, -1):     # the window is by index, nearest first
                if ref_rev[j] != ref_rev[i]:
                    break
                if mutant == "seam_lane" and (i - j) % 64 == 0:
                    continue
                if ids is not None and ids[j - lo] != ids[i - lo]:
                    continue
                step = pair(ref_rev[i] & 1, rpos[j], qpos[j], rpos[i], qpos[i], p, mutant)
                if step is None:
                    continue
                score = f[j] + step[0] - step[1]
                # nearest first: a later equal score is a smaller j
                if score > best or (mutant == "tie_smallest" and score == best and score > p.k):
                    best, at = score, j
            f[i], pred[i] = best, at
    return f, pred


def chain(anchors, p, mutant=None, trace=None):
    """The whole result of run_device.  trace: a list that takes (read, start, walk, stop, score, kept) of every walk of the backtrack."""
    assert verify(anchors) == OK and check_params(p) == OK
    off, ref_rev, rpos, qpos = (a.tolist() for a in anchors)
    f, pred = recurrence(anchors, p, mutant)
    n_reads = len(off) - 1
    c_offsets, rows, m_offsets, members, read_rows = [0], [], [0], [], []
    for q in range(n_reads):
        lo, hi = off[q], off[q + 1]
        used, kept, best = set(), 0, 0
        for i in sorted(range(lo, hi), key=lambda a: (-f[a], a)):
            if i in used or f[i] < p.min_score:
                continue
            walk, t = [], i
            while t != NONE and t not in used:
                walk.append(t)
                used.add(t)
                t = pred[t]
            score = f[i] - (f[t] if t != NONE and mutant != "stop_not_subtracted" else 0)
            if trace is not None:
                trace.append((q, i, tuple(walk), t, score, score >= p.min_score and len(walk) >= p.min_cnt))
            if score >= p.min_score and len(walk) >= p.min_cnt:
                first, last = walk[-1], walk[0]
                rows.append([score, len(walk), ref_rev[i], rpos[first], qpos[first], rpos[last], qpos[last], 0])
                members += walk[::-1]
                m_offsets.append(len(members))
                kept += len(walk)
                best = max(best, score)
            elif mutant == "dropped_unused":
                used -= set(walk)
        c_offsets.append(len(rows))
        read_rows.append([hi - lo, len(rows) - c_offsets[q], kept, best])
    return Result(np.array(c_offsets, dtype=U64), np.array(rows, dtype=U32).reshape(-1, 8), np.array(m_offsets, dtype=U64),
                  np.array(members, dtype=U32), np.array(f, dtype=I32), np.array(pred, dtype=U32), np.array(read_rows, dtype=U32).reshape(-1, 4))


def run_lengths(anchors, max_dist, mutant=None):
    off, ref_rev, rpos, qpos = (a.tolist() for a in anchors)
    out = []
    for q in range(len(off) - 1):
        ids = _run_ids(ref_rev, rpos, off[q], off[q + 1], max_dist, mutant)
        out += np.bincount(ids).tolist() if ids else []
    return out


def stats(anchors, p, result, mutant=None):
    """The stats without device_bytes."""
    runs = run_lengths(anchors, p.max_dist, mutant)
    return {"n_reads": anchors[0].size - 1, "n_anchors": anchors[1].size, "n_runs": len(runs), "longest_run": max(runs, default=0),
            "n_chains": result.chain_rows.shape[0], "n_members": result.members.size, "reserved": 0}


EMPTY_STATS = dict.fromkeys(STATS[:-1], 0)


def device_bytes(n_reads=None, n_anchors=0, n_runs=0, n_chains=0, n_members=0):
    """stats.device_bytes of a handle since its last trim, term by term as the header states them; every argument is the largest of
    the runs since then (every array grows to exactly the largest size needed so far).  The counter words; then, with any run: the result,
    8 B per anchor (f and p), 8 + 16 B per read and 8 more (c_offsets and the read rows), 32 + 8 B per chain and 8 more (the chain rows
    and m_offsets) and 4 B per member; the work arrays, 25 B per anchor (run heads and their scan, the visit keys twice, the used
    marks), 4 B per run and 4 more (where each run starts) and 16 B per read and 16 more (the chain and member counts and the member
    bases).  rocPRIM's temporary storage is held inside a call only: no term."""
    if n_reads is None:
        return 0
    return 8 * CTR_WORDS + 8 * n_anchors + 24 * n_reads + 8 + 40 * n_chains + 8 + 4 * n_members + 25 * n_anchors + 4 * n_runs + 4 + 16 * n_reads + 16
