"""The inputs of the GPU tests of the alignment library (tests/test_gpu_align.py), made on the host: tests/test_align_inputs.py proves
with the model that each has what it claims - DP segments, a path on the band's edge, a chain that is too long - without a GPU.

A fabricated chain is (reference, query, anchors, strand): the query in reference-forward orientation, the anchors as (reference
position, query position) in that orientation.  `build` gives every chain a reference record and a read of its own - the read is the
query's reverse complement on the reverse strand - so that a chain's first base is its record's first and its last base the record's
last on both."""
import random

import numpy as np

import _align_model as M

K = 7                                      # the seed length of the fabricated cases
DEFAULT = M.Params(K)
COMP = bytes.maketrans(b"ACGTUacgtu", b"TGCAAtgcaa")


def revcomp(s):
    return bytes(s).translate(COMP)[::-1]


def dna(rng, n, alphabet=b"ACGT"):
    return bytes(rng.choice(alphabet) for _ in range(n))


def mutated(rng, s, rate):
    """s with substitutions, insertions and deletions planted at `rate` each per base."""
    out = bytearray()
    for c in s:
        x = rng.random()
        if x < rate:
            out.append(rng.choice([b for b in b"ACGT" if b != c]))
        elif x < 2 * rate:
            out += bytes([c]) + dna(rng, rng.randint(1, 3))
        elif x >= 3 * rate:
            out.append(c)
    return bytes(out)


def build(chains, k=K, sel=None, pad_records=0):
    """The model's Input of fabricated chains (ref, qry, anchors, rev), one reference record and one read each.  pad_records: that many
    bases in front of and behind every chain in its two records, so that it does not start or end them."""
    rng = random.Random(99)
    refs, reads, rows = [], [], []
    for ref, qry, anchors, rev in chains:
        ref, qry = dna(rng, pad_records) + ref + dna(rng, pad_records), dna(rng, pad_records) + qry + dna(rng, pad_records)
        refs.append(ref)
        reads.append(revcomp(qry) if rev else qry)
        at = [(r + pad_records, len(qry) - (q + pad_records) - k if rev else q + pad_records) for r, q in anchors]
        rows.append([(50, (len(refs) - 1) << 1 | rev, at)])
    n = len(chains)
    return M.Input(M.pack(refs), M.pack(reads), M.chains_of(rows), np.arange(n, dtype=M.U32) if sel is None else np.asarray(sel, dtype=M.U32))


def flank(rng, k=K):
    return dna(rng, k)


def between(ref_mid, qry_mid, rev=0, k=K, seed=5):
    """A chain of two anchors around one between part: n = len(ref_mid) against m = len(qry_mid)."""
    rng = random.Random(seed)
    a, b = flank(rng, k), flank(rng, k)
    return (a + ref_mid + b, a + qry_mid + b, [(0, 0), (k + len(ref_mid), k + len(qry_mid))], rev)


def noisy(rng, n, m=None, rate=0.06):
    """A between part of about n x m: a random piece and a mutated copy, cut or extended to the exact lengths."""
    m = n if m is None else m
    ref = dna(rng, n)
    qry = mutated(rng, ref, rate)
    qry = qry[:m] + dna(rng, max(0, m - len(qry)))
    return ref, qry


# ---- the cases ----------------------------------------------------------------------------------------------------------------------------

def tiny_cases():
    """name -> (Input, Params): no selection; one member; pure gap runs; 1 x 1; overlapping anchors with dr < k, dq < k, dr != dq."""
    rng = random.Random(1)
    one = dna(rng, K)
    s = dna(rng, 30)
    return {
        "nothing selected": (build([between(b"ACG", b"ACG")], sel=[]), DEFAULT),
        "one member": (build([(one, one, [(0, 0)], 0), (one, one[:3] + b"N" + one[4:], [(0, 0)], 1)]), DEFAULT),
        "pure gap runs": (build([between(b"ACGTT", b""), between(b"", b"GG"), between(b"", b""), between(b"", b"T", 1), between(b"CA", b"", 1)]), DEFAULT),
        "one by one": (build([between(b"A", b"A"), between(b"A", b"C"), between(b"N", b"N"), between(b"G", b"G", 1)]), DEFAULT),
        # anchors at reference 0, 3, 8 and query 0, 5, 8: dr = 3, dq = 5, then dr = 5, dq = 3
        "overlapping anchors": (build([(s[:20], s[:3] + b"TT" + s[3:6] + s[8:20], [(0, 0), (3, 5), (8, 8)], 0),
                                       (s[:20], s[:3] + b"TT" + s[3:6] + s[8:20], [(0, 0), (3, 5), (8, 8)], 1)]), DEFAULT),
    }


SEAM_SIZES = ((63, 63), (64, 64), (65, 65), (127, 127), (128, 128), (129, 129), (60, 70), (70, 60), (64, 65), (65, 64), (130, 120), (1, 100), (100, 1))


def seams_case():
    """One chain per size of SEAM_SIZES, alternating strands: the strips of 64 rows and the 64-column blocks of the query's codes."""
    rng = random.Random(2)
    return build([between(*noisy(rng, n, m), rev=i & 1, seed=i) for i, (n, m) in enumerate(SEAM_SIZES)])


def band_cases():
    """name -> (Input, Params, claim): claim is "lo" or "hi" where the path must run along that edge of the band, "pair" where the
    unbanded optimum has an indel pair that band_pad = 0 forbids, "wide" where the band is wider than the matrix, None otherwise."""
    rng = random.Random(3)
    s, j1, j2 = dna(rng, 60), b"G" * 6, b"C" * 6
    p0, p6 = DEFAULT._replace(band_pad=0), DEFAULT._replace(band_pad=6)
    return {
        "pad 0, n != m": (build([between(*noisy(rng, 40, 47)), between(*noisy(rng, 47, 40), rev=1), between(*noisy(rng, 70, 3))]), p0, None),
        # the query is the reference shifted by one: without a band 1D ... 1I, on the diagonal alone mismatches
        "pad 0, n == m": (build([between(b"T" + s[:40], s[:40] + b"A"), between(s[:40] + b"A", b"T" + s[:40], rev=1)]), p0, "pair"),
        # six reference bases the query lacks, then sixty shared, then six the reference lacks: along diagonal -6
        "low edge": (build([between(j1 + s + b"", s + j2), between(j1 + s, s + j2, rev=1)]), p6, "lo"),
        "high edge": (build([between(s + j1, j2 + s), between(s + j1, j2 + s, rev=1)]), p6, "hi"),
        "wider than the matrix": (build([between(*noisy(rng, 5, 5)), between(*noisy(rng, 3, 9))]), DEFAULT, "wide"),
    }


def ties_case():
    """Homopolymers of unequal length, both ways and on both strands, and a part whose optimum is a deletion run beside an insertion
    run (a mismatch costs 255)."""
    chains = [between(b"AAAA", b"AAA"), between(b"AAA", b"AAAA"), between(b"AAAA", b"AAA", 1), between(b"ACA", b"AA"), between(b"AA", b"ACA"),
              between(b"TTTTTTTT", b"TT"), between(b"ACGTCCCCACGT", b"ACGTGGGGACGT"), between(b"ACGTCCCCACGT", b"ACGTGGGGACGT", 1)]
    return build(chains), DEFAULT._replace(b=255)


def bases_case():
    """N and the break byte inside a gap and on the diagonal, lower case against upper case, U against T, on both strands."""
    chains = []
    for rev in (0, 1):
        chains += [between(b"ACGNN\nTTGCA", b"ACGTTGCA", rev), between(b"acgtacgtac", b"ACGTACGTAC", rev), between(b"ACGUUACGU", b"ACGTTACGT", rev),
                   between(b"ACNGT", b"ACNGT", rev), between(b"GATTACA", b"GAT\nNACA", rev), between(b"ugcaugca", b"TGCATGCA", rev)]
    return build(chains)


def strands_case():
    """Chains of three members on both strands that begin and end their records (qs = 0, qe = len, rs = 0, re = len), and the same
    chains inside longer records."""
    rng = random.Random(4)
    chains = []
    for rev in (0, 1):
        a, b, c = flank(rng), flank(rng), flank(rng)
        r1, q1 = noisy(rng, 30, 33)
        r2, q2 = noisy(rng, 12, 9)
        chains.append((a + r1 + b + r2 + c, a + q1 + b + q2 + c, [(0, 0), (K + 30, K + 33), (2 * K + 42, 2 * K + 42)], rev))
    return build(chains), build(chains, pad_records=11)


MAX_SEG = 20


def max_seg_case():
    """max(n, m) at max_seg and one above it, by n and by m; a chain is too long by its second segment alone.  (Input, Params, the
    entries that are too long.)"""
    rng = random.Random(5)
    a, b, c = flank(rng), flank(rng), flank(rng)
    r1, q1 = noisy(rng, 5, 5)
    long_second = (a + r1 + b + dna(rng, MAX_SEG + 1) + c, a + q1 + b + c, [(0, 0), (K + 5, K + 5), (2 * K + 5 + MAX_SEG + 1, 2 * K + 5)], 0)
    chains = [between(*noisy(rng, MAX_SEG, 5)), between(*noisy(rng, MAX_SEG + 1, 5)), between(*noisy(rng, 5, MAX_SEG), rev=1),
              between(*noisy(rng, 5, MAX_SEG + 1), rev=1), long_second, between(dna(rng, MAX_SEG + 1), b"")]
    return build(chains), DEFAULT._replace(max_seg=MAX_SEG), [1, 3, 4, 5]


LARGEST = 4095


def largest_case():
    """One part of 4095 x 4095 with band_pad = 4095, the largest the library takes, between two of 100 x 100."""
    rng = random.Random(6)
    chains = [between(*noisy(rng, 100, 100)), between(*noisy(rng, LARGEST, LARGEST, 0.03), rev=1), between(*noisy(rng, 100, 100))]
    return build(chains), DEFAULT._replace(band_pad=4095, max_seg=4095)


GROUP_PART = 2400


def groups_case():
    """Three parts of 2400 x 2400 with band_pad = 4095, 5.76 MB of direction bytes each: 16 MiB hold two of them, so that workspace
    takes two groups and the default one."""
    rng = random.Random(9)
    chains = [between(*noisy(rng, GROUP_PART, GROUP_PART, 0.03), rev=i & 1, seed=i) for i in range(3)]
    return build(chains), DEFAULT._replace(band_pad=4095, max_seg=4095)


def selection_case():
    """Duplicates and any order: the seams case selected backwards, every third chain twice, some not at all."""
    inp = seams_case()
    n = len(SEAM_SIZES)
    return inp._replace(sel=np.asarray([n - 1 - i for i in range(n) if i % 4 != 1] + [3, 3, 0, 6, 3], dtype=M.U32))


def many_segments_case(n_cu):
    """1.25 steps of the DP kernel's capped grid of chains with one 1 x 1 part each, at k = 2: (Input, Params, step)."""
    step = n_cu * M.BLOCKS_PER_CU * (M.THREADS // 64)
    rng = random.Random(7)
    n = step + step // 4
    mids = [(dna(rng, 1), dna(rng, 1)) for _ in range(n)]
    ref = b"".join(b"AC" + r + b"GT" for r, _ in mids)
    reads = [b"AC" + q + b"GT" for _, q in mids]
    rows = [[(50, 0, [(5 * i, 0), (5 * i + 3, 3)])] for i in range(n)]
    return M.Input(M.pack([ref]), M.pack(reads), M.chains_of(rows), np.arange(n, dtype=M.U32)), M.Params(2), step


def refused_cases():
    """(what, Input, status): one input per flag of the verification."""
    good = strands_case()[1]
    ch = good.chains
    edit = lambda **kw: good._replace(chains=ch._replace(**kw))   # noqa: E731

    def put(a, i, v):
        a = a.copy()
        a[i] = v
        return a
    rows = lambda c, w, v: put(ch.chain_rows.reshape(-1), 8 * c + w, v).reshape(-1, 8)   # noqa: E731
    return [
        ("reference offsets decrease", good._replace(refs=good.refs._replace(offsets=put(good.refs.offsets, 1, 0))), M.ERR_BAD_ARG),
        ("reference offsets beyond the bytes", good._replace(refs=good.refs._replace(offsets=put(good.refs.offsets, 2, good.refs.data.size + 1))), M.ERR_BAD_ARG),
        ("read offsets decrease", good._replace(reads=good.reads._replace(offsets=put(good.reads.offsets, 1, 0))), M.ERR_BAD_ARG),
        ("c_offsets beyond the chains", edit(c_offsets=put(ch.c_offsets, 2, 3)), M.ERR_BAD_ARG),
        ("a selected chain without a member", edit(m_offsets=put(ch.m_offsets, 1, int(ch.m_offsets[0]))), M.ERR_BAD_ARG),
        ("m_offsets beyond the members", edit(m_offsets=put(ch.m_offsets, 2, ch.members.size + 1)), M.ERR_BAD_ARG),
        ("a member beyond the anchors", edit(members=put(ch.members, 4, ch.rpos.size)), M.ERR_BAD_ARG),
        ("dr of 0", edit(rpos=put(ch.rpos, 1, int(ch.rpos[0]))), M.ERR_BAD_ARG),
        ("dq of 0 on the reverse strand", edit(qpos=put(ch.qpos, 4, int(ch.qpos[3]))), M.ERR_BAD_ARG),
        ("a score of 0", edit(chain_rows=rows(0, 0, 0)), M.ERR_BAD_ARG),
        ("a reference beyond the batch", edit(chain_rows=rows(1, 2, 2 << 1 | 1)), M.ERR_BAD_ARG),
        ("re beyond the reference", edit(rpos=put(ch.rpos, 2, int(ch.rpos[2]) + 12)), M.ERR_BAD_ARG),
        ("qe beyond the read", edit(qpos=put(ch.qpos, 2, int(ch.qpos[2]) + 12)), M.ERR_BAD_ARG),
        ("a selected index beyond the chains", good._replace(sel=np.asarray([0, 2], dtype=M.U32)), M.ERR_BAD_ARG),
        ("a selected chain of no read", good._replace(chains=ch._replace(c_offsets=put(ch.c_offsets, 2, 1))), M.ERR_BAD_ARG),
    ]


def long_span_case(span):
    """A chain of two members whose re - rs is `span`, on a reference of 2^28 bases (zero bytes): 2^28 is refused as unsupported, one
    less is accepted and too long."""
    refs = M.Batch(np.zeros((1 << 28) + 1, dtype=M.U8), np.asarray([0, (1 << 28) + 1], dtype=M.U64))
    return M.Input(refs, M.pack([b"A" * 20]), M.chains_of([[(50, 0, [(0, 0), (span - K, 10)])]]), np.zeros(1, dtype=M.U32))


def bad_params():
    good = DEFAULT
    return [good._replace(k=0), good._replace(k=256), good._replace(a=0), good._replace(a=256), good._replace(b=0), good._replace(b=256),
            good._replace(q=256), good._replace(e=0), good._replace(e=256), good._replace(band_pad=4096), good._replace(max_seg=0),
            good._replace(max_seg=4096), good._replace(work_mib=15), good._replace(work_mib=4097)]


def edge_params():
    """Accepted: every score at 255, q = 0, the smallest of everything."""
    return [DEFAULT._replace(a=255, b=255, q=255, e=255), DEFAULT._replace(q=0), DEFAULT._replace(a=1, b=1, q=0, e=1, band_pad=0, max_seg=1, work_mib=16),
            DEFAULT._replace(band_pad=4095, max_seg=4095, work_mib=4096)]


# ---- end to end ---------------------------------------------------------------------------------------------------------------------------

E2E_K, E2E_W = 15, 10
E2E_MAX_DIST = 2000                        # of the chains: consecutive anchors lie at most this far apart on both sequences


def sequences():
    """A random reference of 20 kb and 200 reads of 150 to 2000 bases cut from it, with substitutions, insertions and deletions planted
    at 2 % each, every other one reverse-complemented."""
    rng = random.Random(8)
    ref = dna(rng, 20000)
    reads = []
    for i in range(200):
        n = rng.randint(150, 2000)
        at = rng.randint(0, len(ref) - n)
        read = mutated(rng, ref[at: at + n], 0.02)
        reads.append(revcomp(read) if i & 1 else read)
    return [ref], reads
