"""The fabricated cases of the mapping library, shared by tests/test_mapping_inputs.py (no GPU: no case is vacuous, and every wrong
library of tests/_mapping_model.py is told from the right one by the case named for it) and tests/test_gpu_mapping.py."""
import numpy as np

import _mapping_model as M

K = 15
DEFAULT = M.Params(K)
SEAM_SIZES = (1, 2, 63, 64, 65, 128, 129, 200)
BIG_READS = ((600, 0), (600, 575), (700, 576), (700, 635))   # more chains than the LDS strip buffer holds
RANDOM_SEEDS = (11, 12)
# the GPU case that tells each wrong library of the model from the right one
MUTANT_CASE = {"parent_link": "roots", "mask_ge": "boundary", "link_highest": "roots", "tie_desc_index": "ties", "seam_lane": "seams",
               "best_n_ineligible": "secondaries", "n_sub_kept": "secondaries", "no_strand_swap": "spans", "mlen_no_cap": "spans"}


def tiny_cases():
    one = (50, 0, [(7, 3)])
    return {"no reads": M.batch_of([]), "no chains": M.batch_of([[], []]), "reads without chains": M.batch_of([[], [one], [], []]),
            "one chain of one member": M.batch_of([[one]]), "chains of no read around": M.batch_of([[one], []], lead=2, tail=3)}


def seam_read(n, at):
    """n chains by descending score on disjoint intervals, but the last lies where the chain of rank `at` lies: its only overlap."""
    chains = [M.span(5000 - r, 100 * r, 100 * r + 50, K) for r in range(n - 1)]
    return chains + [M.span(5000 - (n - 1), 100 * at, 100 * at + 50, K)]


def seam_ats(n):
    return sorted({at for at in (0, 63, 64, n - 1 - 64) if 0 <= at < n - 1})


def seam_reads():
    """(n, at) of every read of seams_case, in its order; n == 1 has no other chain to overlap."""
    return [(1, None)] + [(n, at) for n in SEAM_SIZES for at in seam_ats(n)]


def seams_case():
    return M.batch_of([[M.span(100, 0, 50, K)] if at is None else seam_read(n, at) for n, at in seam_reads()])


def big_reads_case():
    return M.batch_of([seam_read(n, at) for n, at in BIG_READS])


def roots_case():
    """A [0,100), B [40,140), C [98,180) by descending score: C overlaps B and not A, yet its parent is A.  Then A [0,100), B [90,200),
    C [40,150): C overlaps both primaries and its link is A, the lowest rank."""
    return M.batch_of([[M.span(300, 0, 100, K), M.span(200, 40, 140, K), M.span(100, 98, 180, K)],
                       [M.span(300, 0, 100, K), M.span(200, 90, 200, K), M.span(100, 40, 150, K)]])


def boundary_case():
    """B [40,140) and C [100,180): ol * 1000 == 500 * min exactly, so C is primary; one base more and it is not."""
    return M.batch_of([[M.span(200, 40, 140, K), M.span(100, 100, 180, K)], [M.span(200, 40, 140, K), M.span(100, 99, 179, K)]])


MASK_PARAMS = (M.Params(K, mask_level_pm=0), M.Params(K, mask_level_pm=1000), M.Params(K, mask_level_pm=1), M.Params(K, mask_level_pm=999))


def ties_case():
    """Equal scores rank by chain index: the first is the primary, and its two equal children give subsc and n_sub."""
    return M.batch_of([[M.span(100, 0, 100, K), M.span(100, 0, 100, K, 3), M.span(100, 10, 100, K)],
                       [M.span(90, 0, 60, K), M.span(100, 200, 300, K), M.span(100, 210, 300, K), M.span(90, 5, 60, K)]])


def secondaries_case():
    """Two primaries, 1000 on [0,100) and 500 on [200,300).  Read 0: children at exactly 800 per mille of the parent (kept) and one
    below (dropped).  Read 1: seven eligible children, with ineligible ones ranked between them that must not count."""
    a, b = (lambda s: M.span(s, 10, 100, K)), (lambda s: M.span(s, 210, 300, K, 5))
    return M.batch_of([[M.span(1000, 0, 100, K), a(800), a(799), M.span(500, 200, 300, K), b(400), b(399)],
                       [M.span(1000, 0, 100, K), a(900), a(850), a(700), a(600), M.span(500, 200, 300, K), b(450), b(420), b(410), b(405), b(401)]])


BEST_N_PARAMS = (M.Params(K, best_n=0), M.Params(K, best_n=1), DEFAULT, M.Params(K, best_n=7), M.Params(K, pri_ratio_pm=0), M.Params(K, pri_ratio_pm=1000))


def member_chain(score, ref_rev, pairs, rs=500, q_lo=20):
    """A chain whose consecutive members step by `pairs` (dr, dq); on the reverse strand the first member has the largest qpos."""
    r, q = [rs], [0]
    for dr, dq in pairs:
        r.append(r[-1] + dr)
        q.append(q[-1] + dq)
    q = [q_lo + (q[-1] - x if ref_rev & 1 else x) for x in q]
    return (score, ref_rev, list(zip(r, q)))


STEPS = ((K - 1, K - 1), (K, K), (K + 1, K + 1), (K - 3, K + 4), (K + 5, K - 2), (1, 1), (30, 31), (K + 1, K + 2), (2, K), (K, 3))


def spans_case():
    """Both strands; dr and dq below, at and above k; chains of 1, 2, 64, 65 and 1000 members."""
    reads = []
    for cnt in (1, 2, 64, 65, 1000):
        pairs = [STEPS[i % len(STEPS)] for i in range(cnt - 1)]
        reads.append([member_chain(300, 4, pairs), member_chain(200, 7, pairs), member_chain(100, 1, pairs[::-1], q_lo=0)])
    return M.batch_of(reads)


def mapq_reads():
    """(score, cnt, scores of the children) of every read of mapq_case."""
    return [(99, 9, (90,)), (100, 10, (90,)), (101, 11, (90,)), (99, 11, (90,)), (101, 9, (90,)), (99, 9, ()), (200, 20, (30,)), (200, 20, (39,)), (200, 20, (40,)), (200, 20, (41,)),
            (200, 20, (150,)), (200, 20, (199,) * 5), (200, 20, (200,)), (50, 3, (49,)), (41, 3, ()), (40, 3, ()), (1000, 50, ()), (60, 5, ()),
            (300, 12, (100,) * 200), ((1 << 31) - 1, 4, ()), (1, 1, ())]


def mapq_case():
    return M.batch_of([[member_chain(score, 0, [(1, 1)] * (cnt - 1), q_lo=0)] + [M.span(s, 0, K, K) for s in subs] for score, cnt, subs in mapq_reads()])


def many_reads_case(n_cu):
    """1.25 steps of the capped grid of one wave per read, at 1 to 3 chains each; (chains, waves of one step)."""
    step = n_cu * M.BLOCKS_PER_CU * (M.THREADS // 64)
    n = step + step // 4
    shapes = ([M.span(100, 0, 100, K)], [M.span(100, 0, 100, K), M.span(90, 50, 150, K)],
              [M.span(80, 200, 300, K), M.span(100, 0, 100, K), M.span(90, 20, 100, K)])
    return M.batch_of([shapes[(q * 7 + q // 5) % 3] for q in range(n)]), step


def random_chain(rng, score, qs, qe, cnt, ref_rev):
    """A chain of at most cnt members over [qs, qe) (one member: over [qs, qs + K)), rpos jittered against qpos."""
    room = qe - K - qs
    cnt = min(cnt, room + 1)
    cuts = [0] if cnt < 2 else sorted({0, room} | set(rng.choice(room + 1, size=cnt - 2, replace=False).tolist()))
    pairs = [(max(1, dq + int(rng.integers(-3, 4))), dq) for dq in np.diff(cuts).tolist()]
    return member_chain(score, ref_rev, pairs, rs=int(rng.integers(0, 100000)), q_lo=qs)


def random_case(seed):
    """Random reads of 0 to 40 chains on a query of 1000, scores with ties; then three reads that pin the mapq range: an isolated strong
    chain (60), an isolated weak one (in between) and two equal ones on one interval (0)."""
    rng = np.random.default_rng(seed)
    reads = []
    for _ in range(40):
        chains = []
        for _ in range(int(rng.integers(0, 41))):
            qs = int(rng.integers(0, 900))
            qe = min(1000, qs + int(rng.integers(K, 400)))
            chains.append(random_chain(rng, int(rng.choice([40, 60, 80, 100, 150, 200, 300]) + rng.integers(0, 3)), qs, qe, int(rng.integers(1, 16)),
                                       int(rng.integers(0, 8))))
        reads.append(chains)
    reads += [[member_chain(300, 0, [(10, 10)] * 11)], [member_chain(60, 1, [(10, 10)] * 4)], [M.span(100, 0, 100, K), M.span(100, 0, 100, K)]]
    return M.batch_of(reads, lead=1, tail=2)


RANDOM_PARAMS = (DEFAULT, M.Params(K, 300, 900, 2, 60), M.Params(K, 800, 500, 65535, 1))


def _edit(ch, **kw):
    return ch._replace(**{name: fn(getattr(ch, name).copy()) for name, fn in kw.items()})


def _set(i, v):
    def fn(a):
        a[i] = v
        return a
    return fn


def refused_cases():
    """(what, chains, status): one input per flag of the verification."""
    base = M.batch_of([[member_chain(100, 0, [(10, 10)] * 3), member_chain(90, 1, [(10, 10)] * 3)], [member_chain(80, 2, [(5, 5)] * 2)]])
    top = (1 << 32) - 1
    long_blen = M.batch_of([[(100, 0, [(0, 0), ((1 << 31) + 10, 1), ((1 << 31) + 11, (1 << 31) + 11)])]])
    fits_blen = M.batch_of([[(100, 0, [(0, 0), ((1 << 31) + 10, 1), ((1 << 31) + 11, (1 << 31) - 10 - K)])]])
    assert M.verify(base, K) == M.OK and M.verify(fits_blen, K) == M.OK
    assert M.chain_fields(fits_blen, 0, K)[8] == top, "the largest blen that fits"
    return [
        ("c_offsets decrease", _edit(base, c_offsets=_set(1, 4)), M.ERR_BAD_ARG),
        ("c_offsets[n_reads] > n_chains", _edit(base, c_offsets=_set(2, 4)), M.ERR_BAD_ARG),
        ("m_offsets decrease", _edit(base, m_offsets=_set(1, 9)), M.ERR_BAD_ARG),
        ("m_offsets[n_chains] > n_members", _edit(base, m_offsets=_set(3, 12)), M.ERR_BAD_ARG),
        ("a chain without a member", _edit(base, m_offsets=_set(1, 0)), M.ERR_BAD_ARG),
        ("a member that is no anchor", _edit(base, members=_set(5, 11)), M.ERR_BAD_ARG),
        ("dr == 0", _edit(base, rpos=_set(2, int(base.rpos[1]))), M.ERR_BAD_ARG),
        ("dq == 0 forward", _edit(base, qpos=_set(2, int(base.qpos[1]))), M.ERR_BAD_ARG),
        ("dq < 0 reverse", _edit(base, qpos=_set(6, int(base.qpos[5]) + 1)), M.ERR_BAD_ARG),
        ("a forward chain marked reverse", _edit(base, chain_rows=_set((0, 2), 1)), M.ERR_BAD_ARG),
        ("score 0", _edit(base, chain_rows=_set((1, 0), 0)), M.ERR_BAD_ARG),
        ("score 2^31", _edit(base, chain_rows=_set((2, 0), 1 << 31)), M.ERR_BAD_ARG),
        ("re does not fit", _edit(base, rpos=_set(10, top - K + 1)), M.ERR_UNSUPPORTED),
        ("qe does not fit", _edit(base, qpos=_set(10, top - K + 1)), M.ERR_UNSUPPORTED),
        ("blen does not fit", long_blen, M.ERR_UNSUPPORTED),
        ("score 0 goes before a long end", _edit(base, rpos=_set(10, top - K + 1), chain_rows=_set((0, 0), 0)), M.ERR_BAD_ARG),
    ]


def accepted_edges():
    """Inputs at the edge of the verification that are accepted: re and qe of 2^32 - 1, the largest blen, the largest score."""
    base = M.batch_of([[member_chain(100, 0, [(10, 10)] * 3)], [member_chain((1 << 31) - 1, 2, [(5, 5)] * 2)]])
    top = (1 << 32) - 1
    return {"re == 2^32 - 1": _edit(base, rpos=_set(6, top - K)), "qe == 2^32 - 1": _edit(base, qpos=_set(6, top - K)),
            "blen == 2^32 - 1": M.batch_of([[(100, 0, [(0, 0), ((1 << 31) + 10, 1), ((1 << 31) + 11, (1 << 31) - 10 - K)])]])}


def bad_params():
    return [M.Params(0), M.Params(256), M.Params(K, mask_level_pm=1001), M.Params(K, pri_ratio_pm=1001), M.Params(K, best_n=65536),
            M.Params(K, min_chain_score=0), M.Params(K, r0=1), M.Params(K, r1=1), M.Params(K, r2=1)]


CASES = {"roots": (roots_case, (DEFAULT,)), "boundary": (boundary_case, (DEFAULT,) + MASK_PARAMS), "ties": (ties_case, (DEFAULT,)),
         "seams": (seams_case, (DEFAULT,)), "big reads": (big_reads_case, (DEFAULT,)), "secondaries": (secondaries_case, BEST_N_PARAMS),
         "spans": (spans_case, (DEFAULT,)), "mapq": (mapq_case, (DEFAULT, M.Params(K, min_chain_score=150)))}


# ---- sequences for the end-to-end test ------------------------------------------------------------------------------------------------------

def revcomp(s):
    return s[::-1].translate(bytes.maketrans(b"ACGT", b"TGCA"))


def sequences(seed=0x3A9, read_len=300, n_unique=60, n_twice=20):
    """Three random references, the third of which holds one 2 000 bp segment twice; reads cut forward and reverse-complemented from the
    unique parts, and reads cut from inside the segment's first copy.  (refs, reads, cuts): cuts[q] = (ref, rev, start) and for a read
    of the segment also the start of the other copy."""
    rng = np.random.default_rng(seed)
    rand = lambda n: bytes(rng.choice(np.frombuffer(b"ACGT", dtype=np.uint8), size=n).tobytes())   # noqa: E731
    seg = rand(2000)
    first, second = 3000, 9000
    refs = [rand(8000), rand(6000), rand(first) + seg + rand(second - first - 2000) + seg + rand(2000)]
    reads, cuts = [], []
    for q in range(n_unique):
        r = q % 3
        limit = first - read_len if r == 2 else len(refs[r]) - read_len
        start = int(rng.integers(0, limit))
        piece = refs[r][start: start + read_len]
        reads.append(revcomp(piece) if q & 1 else piece)
        cuts.append((r, q & 1, start))
    for q in range(n_twice):
        at = int(rng.integers(100, 2000 - read_len - 100))
        piece = refs[2][first + at: first + at + read_len]
        reads.append(revcomp(piece) if q & 1 else piece)
        cuts.append((2, q & 1, first + at, second + at))
    return refs, reads, cuts
