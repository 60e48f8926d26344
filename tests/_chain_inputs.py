"""The inputs of the chain library's GPU tests (tests/test_gpu_chain.py), made without a GPU so that tests/test_chain_inputs.py can
show by the model (tests/_chain_model.py) that none of them is vacuous.  An anchor is (ref_rev, rpos, qpos); a case is (anchors,
params) with the anchors as the model's four arrays."""
import numpy as np

import _chain_model as M

K = 15
DEFAULT = M.Params(K)
WINDOW_H = (1, 2, 63, 64, 65, 128, 512)
RANDOM_SEEDS = (0xC4A1, 0xC4A2)
RANDOM_PARAMS = (DEFAULT, M.Params(K, max_dist=300, bw=40, h=8, min_score=30, min_cnt=2), M.Params(21, max_dist=2000, bw=100, h=200, min_score=60, min_cnt=4))


def diagonal(ref_rev, r0, q0, n, step=20):
    """n anchors of one alignment: forward ones share rpos - qpos, reverse ones rpos + qpos."""
    sign = -1 if ref_rev & 1 else 1
    return [(ref_rev, r0 + step * t, q0 + sign * step * t) for t in range(n)]


def tiny_cases():
    """An empty batch, reads without anchors, one anchor, two."""
    return {"empty batch": M.reads_of([]), "reads without anchors": M.reads_of([[], [], []]), "one anchor": M.reads_of([[(0, 100, 50)]]),
            "two anchors": M.reads_of([[(0, 100, 50), (0, 200, 160)]]), "anchors among empty reads": M.reads_of([[], [(2, 7, 7)], [], diagonal(0, 100, 50, 4), []])}


def fixtures():
    """The issue's five: (anchors, f, p of the last anchor or None)."""
    fwd = lambda step: M.one_read([(0, 100 + step * t, 50 + step * t) for t in range(10)])   # noqa: E731
    return [(fwd(20), [15 * (t + 1) for t in range(10)]), (fwd(7), [15 + 7 * t for t in range(10)]),
            (M.one_read([(0, 100, 50), (0, 200, 160)]), [15, 28]), (M.one_read([(0, 100, 100), (0, 110, 90), (0, 200, 190)]), [15, 15, 28]),
            (M.one_read([(1, 100 + 20 * t, 500 - 20 * t) for t in range(10)]), [15 * (t + 1) for t in range(10)])]


def strands_case():
    """One read with a forward and a reverse chain on reference 0 and a forward one on reference 1; a second read, reverse only."""
    first = sorted(diagonal(0, 1000, 40, 6) + diagonal(1, 1000, 900, 7) + diagonal(2, 300, 10, 5))
    return M.reads_of([first, diagonal(5, 50, 400, 4)])


def window_case(back):
    """A run whose last anchor's only possible predecessor lies exactly `back` anchors in front of it: the first anchor, on its
    diagonal.  The back - 1 anchors between them lie 4000 off that diagonal (dd > bw from the first) and behind the last one in qpos
    (dq < 0)."""
    fill = [(0, 1000 + t, 5000 + t) for t in range(1, back)]
    return M.one_read([(0, 1000, 1000)] + fill + [(0, 1000 + back + 20, 1000 + back + 20)])


def ties_case():
    """A tie between predecessors (the issue's fixture) and a tie in f between the ends of two chains of one read."""
    return M.reads_of([[(0, 100, 100), (0, 110, 90), (0, 200, 190)], sorted(diagonal(0, 100, 100, 4) + diagonal(2, 100, 100, 4))])


EDGE_PARAMS = M.Params(K, max_dist=200, bw=10, h=64, min_score=20, min_cnt=2)


def pair_edge_reads():
    """name -> a read of two anchors under EDGE_PARAMS, and whether the second may follow the first."""
    a = (0, 100, 100)
    return {"dd = bw": ([a, (0, 200, 210)], True), "dd = bw + 1": ([a, (0, 200, 211)], False),
            "dr = max_dist": ([a, (0, 300, 295)], True), "dr = max_dist + 1": ([a, (0, 301, 296)], False),
            "dq = max_dist": ([a, (0, 295, 300)], True), "dq = max_dist + 1": ([a, (0, 296, 301)], False),
            "dq = 0": ([a, (0, 150, 100)], False), "dq < 0": ([a, (0, 150, 90)], False), "dr < k": ([a, (0, 107, 107)], True),
            "reverse dq = max_dist": ([(1, 100, 400), (1, 295, 200)], True), "reverse dq = max_dist + 1": ([(1, 100, 400), (1, 296, 199)], False),
            "reverse dq = 0": ([(1, 100, 400), (1, 150, 400)], False)}


def pair_edges_case():
    return M.reads_of([r for r, _ in pair_edge_reads().values()])


def k_cases():
    """k = 1 and k = 255, on one diagonal of 60 anchors with steps 1..300 and two small indels."""
    rng = np.random.default_rng(0xC4)
    steps = rng.integers(1, 301, 59)
    r = np.concatenate([[500], 500 + np.cumsum(steps)])
    q = r - 400
    q[20:] += 7
    q[40:] -= 3
    read = [(0, int(a), int(b)) for a, b in zip(r, q)]
    return {1: (M.one_read(read), M.Params(1, min_score=10)), 255: (M.one_read(read), M.Params(255))}


SEAM_PARAMS = M.Params(K, max_dist=200, bw=10, h=64, min_score=20, min_cnt=2)


def run_seams_case():
    """rpos gaps of max_dist (one run: the pair chains) and max_dist + 1 (two runs) on one diagonal, and a ref_rev change between
    neighbours that would chain otherwise."""
    return M.reads_of([[(0, 100, 100), (0, 300, 300)], [(0, 100, 100), (0, 301, 301)], [(0, 100, 100), (0, 300, 300), (0, 501, 501), (0, 701, 701)],
                       [(0, 100, 100), (2, 120, 120)], [(0, 100, 100), (1, 120, 80)]])


def _fork(branch):
    """A main chain of ten anchors 20 apart on one diagonal and a branch of `branch` anchors 19 apart on a diagonal 40 further in qpos
    that leaves it behind its sixth anchor: 19, not 20, so that a branch anchor gains one more from the branch anchor in front of it than
    from the main anchor just in front of it."""
    return sorted(diagonal(0, 100, 100, 10) + [(0, 205 + 19 * s, 245 + 19 * s) for s in range(branch)])


MIN_CNT_PARAMS = M.Params(K, min_cnt=6)
MARKED_PARAMS = M.Params(K, min_cnt=7)


def forks_case():
    """Read 0: a branch of five, kept with f[i] - f[t] under the defaults and dropped by min_cnt under MIN_CNT_PARAMS.  Read 1: a
    branch of three, dropped by min_score."""
    return M.reads_of([_fork(5), _fork(3)])


def marked_case():
    """Under MARKED_PARAMS: a stem of two anchors and a tip of four, 40 apart on its diagonal, make a chain of six that ends with f = 90 and
    is dropped by min_cnt = 7; a second tip of 20 anchors 3 apart on a diagonal 110 aside leaves the stem's second anchor, ends with
    f = 83, and its walk stops at that anchor, which the dropped chain marked."""
    return M.one_read(sorted(diagonal(0, 1000, 1000, 2) + diagonal(0, 1060, 1060, 4, 40) + diagonal(0, 1145, 1035, 20, 3)))


def long_run_case(n=5000):
    """One run of n anchors: random steps of 1..30, an indel of a few bases every 200 anchors or so, and some anchors off the diagonal."""
    rng = np.random.default_rng(0x5000)
    r = 1000 + np.cumsum(rng.integers(1, 31, n))
    q = r - 900 + np.cumsum(np.where(rng.random(n) < 0.005, rng.integers(-6, 7, n), 0))
    off = rng.random(n) < 0.1
    q = np.where(off, q + rng.integers(-300, 300, n), q)
    t = sorted(set((0, int(a), int(max(b, 0))) for a, b in zip(r, q)))
    return M.one_read(t)


def many_runs_case(n_cu, quarters=5):
    """More one-anchor runs and more three-anchor runs than one step of ch_dp_kernel's capped grid (quarters / 4 steps of each): reads of
    four runs, 10 000 apart in rpos."""
    step = n_cu * M.BLOCKS_PER_CU * (M.THREADS // 64)   # the waves of the capped grid
    n_reads = (quarters * step // 4 + 1) // 2 + 1
    reads = []
    for q in range(n_reads):
        base = 100 + q % 7
        reads.append([(0, base, 50)] + diagonal(0, base + 10_000, 80, 3, 18) + [(0, base + 20_000, 9)] + diagonal(1, base, 300, 3, 21))
    return M.reads_of(reads), step


def random_case(seed, n_reads=200):
    """Reads of random anchors with planted colinear chains that have indels, on two references and both strands."""
    rng = np.random.default_rng(seed)
    reads = []
    for q in range(n_reads):
        anchors = set()
        for _ in range(int(rng.integers(0, 4))):           # planted chains
            ref_rev, n = int(rng.integers(0, 4)), int(rng.integers(2, 40))
            r = int(rng.integers(0, 20_000)) + np.cumsum(rng.integers(1, 60, n))
            shift = np.cumsum(np.where(rng.random(n) < 0.15, rng.integers(-30, 31, n), 0))
            q0 = int(rng.integers(3000, 6000))
            qq = q0 - (r - r[0]) + shift if ref_rev & 1 else q0 + (r - r[0]) + shift
            anchors |= {(ref_rev, int(a), int(b)) for a, b in zip(r, qq) if b >= 0}
        for _ in range(int(rng.integers(0, 30))):          # noise
            anchors.add((int(rng.integers(0, 4)), int(rng.integers(0, 25_000)), int(rng.integers(0, 9000))))
        reads.append(sorted(anchors))
    return M.reads_of(reads)


def refused_cases():
    """(what, anchors, status): arrays the verification on the device refuses."""
    good = strands_case()
    off, ref_rev, rpos, qpos = (a.copy() for a in good)
    swapped = (off, ref_rev, rpos.copy(), qpos)
    swapped[2][[2, 3]] = swapped[2][[3, 2]]
    repeated = (off, ref_rev.copy(), rpos.copy(), qpos.copy())
    for a in repeated[1:]:
        a[5] = a[4]
    qpos_back = (off, ref_rev, rpos.copy(), qpos.copy())
    qpos_back[2][8] = qpos_back[2][7]
    qpos_back[3][8] = qpos_back[3][7] - 1
    decreasing = (off.copy(), ref_rev, rpos, qpos)
    decreasing[0][1] = decreasing[0][2] + 1
    beyond = (off.copy(), ref_rev, rpos, qpos)
    beyond[0][-1] += 1
    return [("unsorted anchors", swapped, M.ERR_BAD_ARG), ("a repeated anchor", repeated, M.ERR_BAD_ARG), ("a qpos going back", qpos_back, M.ERR_BAD_ARG),
            ("decreasing offsets", decreasing, M.ERR_BAD_ARG), ("offsets[n_reads] > n", beyond, M.ERR_BAD_ARG)]


def bad_params():
    d = DEFAULT._asdict()
    make = lambda **kw: M.Params(**{**d, **kw})   # noqa: E731
    return [make(k=0), make(k=256), make(max_dist=0), make(max_dist=1 << 31), make(bw=5001), make(h=0), make(h=513), make(min_score=0), make(min_cnt=0),
            make(r0=1), make(r1=7)]


# ---- end to end --------------------------------------------------------------------------------------------------------------------------

def revcomp(s):
    return s[::-1].translate(bytes.maketrans(b"ACGT", b"TGCA"))


def sequences(n_refs=3, ref_len=3000, n_reads=40, read_len=400, seed=0xE2E):
    """Random references; reads sampled from them on both strands with 1 % substitutions.  cuts[q] = (ref, rev, start)."""
    rng = np.random.default_rng(seed)
    refs = [bytes(rng.choice(np.frombuffer(b"ACGT", dtype=np.uint8), ref_len)) for _ in range(n_refs)]
    reads, cuts = [], []
    for q in range(n_reads):
        r, start, rev = int(rng.integers(0, n_refs)), int(rng.integers(0, ref_len - read_len)), q & 1
        piece = bytearray(refs[r][start: start + read_len])
        for at in np.flatnonzero(rng.random(read_len) < 0.01):
            piece[at] = b"ACGT"[(b"ACGT".index(piece[at]) + 1 + int(rng.integers(0, 3))) % 4]
        reads.append(revcomp(bytes(piece)) if rev else bytes(piece))
        cuts.append((r, rev, start))
    return refs, reads, cuts
