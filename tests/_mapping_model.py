"""The host model of the mapping library (include_pending/needletail_amd/mapping.h): the rule in plain Python integers, written from the
header's text, and the device memory the header states.  The chains of a batch are (c_offsets, chain_rows, m_offsets, members, rpos,
qpos) as numpy arrays, the shape AnchorChains and SeedIndex hand out on the device.

tests/test_mapping_model.py holds the model to hand-computed fixtures, to a sequential mm_set_parent-style loop written separately and
to the float formula of the mapping quality; the GPU tests hold the library to it.  The `mutant` arguments restate nine wrong libraries
(tests/test_mapping_inputs.py shows that the GPU cases tell each of them from the right one)."""
import collections

import numpy as np

OK, ERR_BAD_ARG, ERR_CAPACITY, ERR_UNSUPPORTED = 0, 2, 5, 6
THREADS = 256             # MP_THREADS of csrc/ntk_map_rule.hpp
BLOCKS_PER_CU = 8         # MP_BLOCKS_PER_CU
LDS_CHAINS = 512          # MP_LDS_CHAINS
READ_CHAINS = 1 << 16     # MP_READ_CHAINS
NONE = 0xFFFFFFFF
CTR_WORDS = 6             # kCtrWords of csrc/ntk_mapping.hip
STATS = ("n_reads", "n_chains", "n_primary", "n_secondary", "n_reported", "most_chains", "reserved", "device_bytes")
FIELDS = ("rows", "order", "out_offsets", "out", "read_rows")
ROW = ("qs", "qe", "rs", "re", "ref_rev", "score", "cnt", "mlen", "blen", "parent", "subsc", "n_sub", "mapq", "flags", "rank", "zero")
W = {name: i for i, name in enumerate(ROW)}
PRIMARY, SECONDARY = 1, 2
MUTANTS = ("parent_link", "mask_ge", "link_highest", "tie_desc_index", "seam_lane", "best_n_ineligible", "n_sub_kept", "no_strand_swap",
           "mlen_no_cap")
U64, U32 = np.uint64, np.uint32

Params = collections.namedtuple("Params", "k mask_level_pm pri_ratio_pm best_n min_chain_score r0 r1 r2", defaults=(500, 800, 5, 40, 0, 0, 0))
Result = collections.namedtuple("Result", FIELDS)
Chains = collections.namedtuple("Chains", "c_offsets chain_rows m_offsets members rpos qpos")


def batch_of(reads, lead=0, tail=0):
    """A batch of reads, each a list of chains (score, ref_rev, [(rpos, qpos), ...]); every chain's anchors are its own.  lead / tail:
    that many one-member chains of no read in front of the first read and behind the last."""
    loose = (7, 0, [(5, 5)])
    flat = [loose] * lead + [c for r in reads for c in r] + [loose] * tail
    c_offsets = np.cumsum([lead] + [len(r) for r in reads])
    rows = [[score, len(m), ref_rev, 0, 0, 0, 0, 0] for score, ref_rev, m in flat]
    m_offsets = np.cumsum([0] + [len(m) for _, _, m in flat])
    anchors = [a for _, _, m in flat for a in m]
    return Chains(np.asarray(c_offsets, dtype=U64), np.asarray(rows, dtype=U32).reshape(-1, 8), np.asarray(m_offsets, dtype=U64),
                  np.arange(len(anchors), dtype=U32), np.asarray([a[0] for a in anchors], dtype=U32), np.asarray([a[1] for a in anchors], dtype=U32))


def span(score, qs, qe, k, ref_rev=0, rs=1000):
    """A chain of this score over the query interval [qs, qe): one member where qe - qs == k, else two, on the diagonal."""
    assert qe - qs >= k
    if qe - qs == k:
        return (score, ref_rev, [(rs, qs)])
    ends = [(rs, qs), (rs + qe - k - qs, qe - k)]
    return (score, ref_rev, ends if not ref_rev & 1 else [(rs, qe - k), (rs + qe - k - qs, qs)])


def check_params(p):
    """What run_device refuses before any device call."""
    ok = (1 <= p.k <= 255 and 0 <= p.mask_level_pm <= 1000 and 0 <= p.pri_ratio_pm <= 1000 and 0 <= p.best_n <= 65535 and
          1 <= p.min_chain_score < 1 << 32 and p.r0 == 0 and p.r1 == 0 and p.r2 == 0)
    return OK if ok else ERR_BAD_ARG


def steps(ch, c):
    """(dr, dq) of the consecutive members of chain c, dq taken strand-wise."""
    m = ch.members[int(ch.m_offsets[c]): int(ch.m_offsets[c + 1])].tolist()
    rev = int(ch.chain_rows[c, 2]) & 1
    out = []
    for j, i in zip(m, m[1:]):
        dr = int(ch.rpos[i]) - int(ch.rpos[j])
        dq = int(ch.qpos[j]) - int(ch.qpos[i]) if rev else int(ch.qpos[i]) - int(ch.qpos[j])
        out.append((dr, dq))
    return out


def verify(ch, k):
    """The status of the verification of the arrays."""
    n_reads, n_chains, n_members, n_anchors = ch.c_offsets.size - 1, ch.chain_rows.shape[0], ch.members.size, ch.rpos.size
    if n_chains >= 1 << 32 or n_reads >= 1 << 32:
        return ERR_BAD_ARG
    co, mo = ch.c_offsets.tolist(), ch.m_offsets.tolist()
    if any(a > b for a, b in zip(co, co[1:])) or any(a > b for a, b in zip(mo, mo[1:])) or co[-1] > n_chains or mo[-1] > n_members:
        return ERR_BAD_ARG
    unsupported = any(b - a >= READ_CHAINS for a, b in zip(co, co[1:]))
    for c in range(co[0], co[-1]):
        if mo[c + 1] <= mo[c] or not 1 <= int(ch.chain_rows[c, 0]) < 1 << 31:
            return ERR_BAD_ARG
        m = ch.members[mo[c]: mo[c + 1]].tolist()
        if any(i >= n_anchors for i in m) or any(dr < 1 or dq < 1 for dr, dq in steps(ch, c)):
            return ERR_BAD_ARG
        q = (int(ch.qpos[m[0]]), int(ch.qpos[m[-1]]))
        if int(ch.rpos[m[-1]]) + k >= 1 << 32 or max(q) + k >= 1 << 32 or k + sum(max(s) for s in steps(ch, c)) >= 1 << 32:
            unsupported = True
    return ERR_UNSUPPORTED if unsupported else OK


def ilog2(v):
    return v.bit_length() - 1


def lg8(v):
    """floor(256 * log2 v) by eight squarings of the mantissa."""
    e = ilog2(v)
    m, frac = v << (31 - e), 0
    for _ in range(8):
        m = (m * m) >> 31
        frac <<= 1
        if m >> 32:
            frac |= 1
            m >>= 1
    return e << 8 | frac


def mapq(score, cnt, subsc, n_sub, min_chain_score):
    pen = min(min(score, 100), 10 * min(cnt, 10))
    sub = max(subsc, min_chain_score)
    d = score - sub if score > sub else 0
    t = (40 * pen * d * lg8(score)) // score
    assert 40 * pen * d * lg8(score) < 1 << 56
    raw = ((t * 45426) >> 16) // 25600
    return max(0, min(60, raw - ((lg8(n_sub + 1) * 771 + 32768) >> 16)))


def overlap(qs_i, qe_i, qs_j, qe_j, mask_level_pm, mutant=None):
    ol = min(qe_i, qe_j) - max(qs_i, qs_j)
    if ol <= 0:
        return False
    least = mask_level_pm * min(qe_i - qs_i, qe_j - qs_j)
    return ol * 1000 >= least if mutant == "mask_ge" else ol * 1000 > least


def rank_key(score, c):
    return (0x7FFFFFFF - score) << 32 | c


def chain_fields(ch, c, k, mutant=None):
    """qs, qe, rs, re, ref_rev, score, cnt, mlen, blen of chain c."""
    m = ch.members[int(ch.m_offsets[c]): int(ch.m_offsets[c + 1])].tolist()
    q0, q1 = int(ch.qpos[m[0]]), int(ch.qpos[m[-1]])
    qs, qe = (q0, q1 + k) if mutant == "no_strand_swap" else (min(q0, q1), max(q0, q1) + k)
    st = steps(ch, c)
    mlen = k + sum(min(dr, dq) if mutant == "mlen_no_cap" else min(dr, dq, k) for dr, dq in st)
    return [qs & 0xFFFFFFFF, qe & 0xFFFFFFFF, int(ch.rpos[m[0]]), int(ch.rpos[m[-1]]) + k, int(ch.chain_rows[c, 2]), int(ch.chain_rows[c, 0]), len(m),
            mlen, k + sum(max(s) for s in st)]


def links(iv, mask_level_pm, mutant=None):
    """link of every rank of a read whose intervals in rank order are iv: the lowest overlapping rank below it, or None."""
    out = []
    for i, (qs, qe) in enumerate(iv):
        hits = [j for j in range(i) if overlap(qs, qe, iv[j][0], iv[j][1], mask_level_pm, mutant)
                and not (mutant == "seam_lane" and j >= 64 and j % 64 == 0)]
        out.append(None if not hits else hits[-1] if mutant == "link_highest" else hits[0])
    return out


def parents(iv, mask_level_pm, mutant=None):
    """The rank of the parent of every rank: the root of the link tree."""
    link = links(iv, mask_level_pm, mutant)
    par = []
    for i, l in enumerate(link):
        par.append(i if l is None else l if mutant == "parent_link" else par[l])
    return par


def run(ch, p, mutant=None):
    """The whole result of run_device."""
    assert verify(ch, p.k) == OK and check_params(p) == OK
    n_reads, n_chains = ch.c_offsets.size - 1, ch.chain_rows.shape[0]
    rows, order = np.zeros((n_chains, 16), dtype=np.int64), np.zeros(n_chains, dtype=np.int64)
    out_offsets, out, read_rows = [0], [], []
    for q in range(n_reads):
        lo, hi = int(ch.c_offsets[q]), int(ch.c_offsets[q + 1])
        for c in range(lo, hi):
            rows[c, :9] = chain_fields(ch, c, p.k, mutant)
        by_rank = sorted(range(lo, hi), key=lambda c: (-rows[c, W["score"]], -c if mutant == "tie_desc_index" else c))
        order[lo:hi] = by_rank
        par = parents([(int(rows[c, 0]), int(rows[c, 1])) for c in by_rank], p.mask_level_pm, mutant)
        eligible_before = counted_before = n_pri = n_kept = 0
        kept_of = {}
        for r, c in enumerate(by_rank):
            pc = by_rank[par[r]]
            primary = par[r] == r
            eligible = not primary and int(rows[c, W["score"]]) * 1000 >= p.pri_ratio_pm * int(rows[pc, W["score"]])
            before = counted_before if mutant == "best_n_ineligible" else eligible_before
            kept = eligible and before < p.best_n
            rows[c, W["parent"]], rows[c, W["flags"]], rows[c, W["rank"]] = pc, PRIMARY if primary else SECONDARY if kept else 0, r
            eligible_before += eligible
            counted_before += not primary
            n_pri, n_kept = n_pri + primary, n_kept + kept
            if not primary and (kept or mutant != "n_sub_kept"):
                rows[pc, W["n_sub"]] += 1
                rows[pc, W["subsc"]] = max(rows[pc, W["subsc"]], rows[c, W["score"]])
            if primary or kept:
                out.append(c)
        for c in by_rank:
            if rows[c, W["flags"]] & PRIMARY:
                rows[c, W["mapq"]] = mapq(*(int(rows[c, W[n]]) for n in ("score", "cnt", "subsc", "n_sub")), p.min_chain_score)
        out_offsets.append(len(out))
        read_rows.append([hi - lo, n_pri, n_kept, int(rows[by_rank[0], W["mapq"]]) if by_rank else 0])
    return Result(rows.astype(U32), order.astype(U32), np.array(out_offsets, dtype=U64), np.array(out, dtype=U32),
                  np.array(read_rows, dtype=U32).reshape(-1, 4))


def stats(ch, result):
    """The stats without device_bytes."""
    return {"n_reads": ch.c_offsets.size - 1, "n_chains": ch.chain_rows.shape[0], "n_primary": int(result.read_rows[:, 1].sum()),
            "n_secondary": int(result.read_rows[:, 2].sum()), "n_reported": result.out.size,
            "most_chains": int(result.read_rows[:, 0].max(initial=0)), "reserved": 0}


EMPTY_STATS = dict.fromkeys(STATS[:-1], 0)


def device_bytes(n_reads=None, n_chains=0, n_reported=0):
    """stats.device_bytes of a handle since its last trim, term by term as the header states them; every argument is the largest of the
    runs since then (every array grows to exactly the largest size needed so far).  The counter words; then, with any run: the result,
    64 + 4 B per chain (the rows and order), 8 + 16 B per read and 8 more (out_offsets and the read rows) and 4 B per reported chain
    (out); the work arrays, 24 B per chain (the rank keys twice, the parents and the places among the reported) and 4 B per read and 4
    more (the reported counts).  rocPRIM's temporary storage is held inside a call only: no term."""
    if n_reads is None:
        return 0
    return 8 * CTR_WORDS + 68 * n_chains + 24 * n_reads + 8 + 4 * n_reported + 24 * n_chains + 4 * n_reads + 4
