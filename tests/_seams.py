"""Inputs around the tile seams of the scans that cut their input into tiles with a halo, shared by the CPU tests (the inputs' own
conditions, the emulator sweeps) and the device sweeps:

- the k-mer builds of scan2_kernel (test_exact_stride_emu.py, test_gpu_exact_stride.py): stride_of, seam_inputs;
- the windowed minimizers on their three routes (test_minimizer_seam_inputs.py, test_minimizer_seams_emu.py, test_gpu_minimizer_seams.py):
  min_stride, min_seam_inputs, thin_far, minimizer_model;
- k = 33..255 (test_wide_seams_emu.py, test_gpu_wide_seams.py): wide_input, WIDE_SEAMS, wide_reference, wide_tie_insert;
- the lower-case watch of the speculative routes (test_lower_watch_inputs.py, test_gpu_lower_watch.py): lower_watch_input,
  lower_watch_positions, lower_tail_lengths.

Every geometry here is a restatement the tests hold the library to; none is read from the library."""
from concurrent.futures import ThreadPoolExecutor

import numpy as np

ACGT = np.frombuffer(b"ACGT", dtype=np.uint8)
_COMP = bytes.maketrans(b"ACGT", b"TGCA")


def revcomp(s: bytes) -> bytes:
    return s[::-1].translate(_COMP)


def map_threads(fn, items, threads: int = 8):
    """[fn(x) for x in items] on a few threads: the oracle's calls release the interpreter lock, and a sweep asks for thousands of them."""
    items = list(items)
    if items:
        fn(items[0])   # (loads the oracle's library once, on this thread)
    with ThreadPoolExecutor(threads) as ex:
        return list(ex.map(fn, items))


def stride_of(k: int) -> int:
    """Bytes a tile of the k-mer build of k advances by: 1008 for k <= 16 (one halo lane), else 1024 - (k - 1) rounded down to a multiple
    of 4 (ntk_tile.hpp Sv2Geom<K, true>; restated here, the tests hold the library to it)."""
    return 1008 if k <= 16 else (1024 - (k - 1)) & ~3


def seam_inputs(k: int, seed: int = 0):
    """A random 3-tile input of the build of k (the third tile holds the end of the input) and, on it, a break at every offset of
    [stride - 24, stride + 24] around each of the two seams, one at a time; and no break at all.  Yields (tag, bytes)."""
    s = stride_of(k)
    rng = np.random.default_rng(0xE4AC7 + 131 * k + seed)
    base = np.frombuffer(b"ACGT", dtype=np.uint8)[rng.integers(0, 4, 3 * s - 5)].copy()
    yield "none", base.tobytes()
    for seam in (s, 2 * s):
        for d in range(-24, 25):
            a = base.copy()
            a[seam + d] = ord("N")
            yield (seam, d), a.tobytes()


# ---- windowed minimizers ---------------------------------------------------------------------------------------------------------------

WM_TILE = 2048   # positions per tile of window_min_reduce_kernel (ntk_kernels.hpp kWmTile), the second pass of the two-pass route


def min_stride(k: int, w: int, route: str) -> int:
    """Bytes a tile of the windowed-minimizer scan of (k, w) advances by, on each of its three routes:
    "fused"    scan2_kernel<K, ..., W>: two halo lanes (992) where the window of k + w - 1 bytes fits 32, three (976) where it is 33..48;
    "generic"  minimizer_scan_kernel: 2 + ceil((w - 1) / 16) halo lanes of 64, at run time (992, 976, 960 or 944);
    "two_pass" scan_kernel materialises at 992 (window_min_reduce_kernel then runs over WM_TILE positions)."""
    if route == "fused":
        assert k + w - 1 <= 48
        return 992 if k + w - 1 <= 32 else 976
    if route == "generic":
        assert k <= 31 and w <= 49
        return (64 - (2 + (w - 1 + 15) // 16)) * 16
    assert route == "two_pass"
    return 992


def tie_distances(k: int, w: int):
    """The smallest and the largest d in 1 .. w - 1 with k + d even (none: no tie cases)."""
    ds = [d for d in range(1, w) if (k + d) % 2 == 0]
    return sorted({ds[0], ds[-1]}) if ds else []


def tie_insert(k: int, d: int, rng, a_prefix: int = 6) -> bytes:
    """A reverse-complement palindrome u + rc(u) of k + d bases whose u begins with `a_prefix` A: its first k-mer and the one d positions
    later have one canonical value on opposite strands, and (all those A in front) that value is the minimum of a window around them."""
    h = (k + d) // 2
    u = (b"A" * a_prefix)[:h] + ACGT[rng.integers(0, 4, max(0, h - a_prefix))].tobytes()
    return u + revcomp(u)


# (3, 2): with seed 0 the random text's own ties (every 4-base palindrome is one at k = 3) cancel the insert's on 38 cases of 58, and the
# rightmost model equals the oracle there (test_minimizer_seam_inputs.py)
_SEED_OF = {(3, 2): 1}


def min_seam_inputs(k: int, w: int, stride: int, n_bytes: int = None, seams=None, seed: int = 0, a_prefix: int = None):
    """A random ACGT input of 3 stride - 5 bytes (the third tile holds its end) and, for each of the two seams S (or `seams` on `n_bytes`):
    ("none",)            the input as it is;
    ("break", S, off)    one N at byte off, every off of [S - (k + w - 1) - 18, S + 18];
    ("tie", S, p, d)     the palindrome of tie_insert written over the input at p, every p of [S - (k + w - 1) - len - 2, S + 18], for the
                         smallest and the largest d of tie_distances (none when w < 2 or no such d exists).
    Yields (tag, bytes).  The quality-masked runs take the ("none",) bytes with one low quality at the `off` of each break case.
    a_prefix: the A in front of the palindrome; six, ten from w = 50 on (among 50 and more random k-mers one below six A is too common)."""
    n = 3 * stride - 5 if n_bytes is None else n_bytes
    seams = (stride, 2 * stride) if seams is None else tuple(seams)
    if a_prefix is None:
        a_prefix = 6 if w < 50 else 10
    rng = np.random.default_rng(0x5EA35 + 1009 * k + 31 * w + stride + seed + _SEED_OF.get((k, w), 0))
    base = ACGT[rng.integers(0, 4, n)].copy()
    span = k + w - 1
    yield ("none",), base.tobytes()
    seen = set()   # seams closer than a sweep is wide share offsets: each once, under the first seam's name
    for S in seams:
        for off in range(max(0, S - span - 18), min(n, S + 19)):
            if off in seen:
                continue
            seen.add(off)
            a = base.copy()
            a[off] = ord("N")
            yield ("break", S, off), a.tobytes()
    for d in tie_distances(k, w):
        s = np.frombuffer(tie_insert(k, d, rng, a_prefix), dtype=np.uint8)
        for S in seams:
            for p in range(max(0, S - span - len(s) - 2), min(n - len(s), S + 18) + 1):
                if (d, p) in seen:
                    continue
                seen.add((d, p))
                a = base.copy()
                a[p: p + len(s)] = s
                yield ("tie", S, p, d), a.tobytes()


def thin_far(cases, k: int, w: int, step: int = 4):
    """Every case whose swept byte (the break, the palindrome's start) lies within k + w + 2 of its seam, and every `step`-th beyond it."""
    for tag, buf in cases:
        if tag[0] == "none" or abs(tag[2] - tag[1]) <= k + w + 2 or (tag[2] - tag[1]) % step == 0:
            yield tag, buf


FUSED_PAIRS = ((15, 5), (16, 12), (17, 9), (19, 10), (21, 11), (22, 12), (23, 9), (23, 12))   # both strides, one- and two-word values, short and long windows
FUSED_Q_PAIRS = ((21, 11), (15, 10))                                                         # the two quality builds of the fused kernel
# all four strides ((24, 1): 992, no window to tie in), both sides of the f64 / general key split
GENERIC_PAIRS = ((3, 2), (21, 11), (24, 11), (25, 17), (26, 18), (21, 19), (16, 34), (31, 33), (11, 49), (24, 1))
TWO_PASS_PAIRS = ((21, 50), (32, 11), (21, 64), (21, 256))                                   # beyond the fused kernels: the two-pass route alone
TWO_PASS_N = 3 * WM_TILE - 5
TWO_PASS_SEAMS = (WM_TILE, 2 * WM_TILE, 2 * 992, 4 * 992)                                    # the 2048-position seams and the 992-byte seams nearest to them


def two_pass_inputs(k: int, w: int, seams=TWO_PASS_SEAMS):
    """The cases of a two-pass-only pair: 3 x 2048 - 5 bytes, swept around TWO_PASS_SEAMS (or those of them in `seams`: the input is the
    same); at w = 256 (the oracle walks 256 k-mers per window) the palindromes at every fourth start."""
    for tag, buf in min_seam_inputs(k, w, 992, n_bytes=TWO_PASS_N, seams=seams):
        if w >= 256 and tag[0] == "tie" and (tag[2] - tag[1]) % 4:
            continue
        yield tag, buf


def min_input_sets():
    """Every distinct input set of the minimizer sweeps as (k, w, stride, routes): a register-fused pair is swept at its own stride, at
    the generic kernel's (NTK_ROUTE_NO_REGFUSED) and at the two-pass route's; a generic pair at the generic kernel's."""
    sets = {}
    for k, w in FUSED_PAIRS:
        for route in ("fused", "generic", "two_pass"):
            sets.setdefault((k, w, min_stride(k, w, route)), []).append(route)
    for k, w in GENERIC_PAIRS:
        routes = sets.setdefault((k, w, min_stride(k, w, "generic")), [])
        if "generic" not in routes:
            routes.append("generic")
    return [(k, w, s, tuple(r)) for (k, w, s), r in sets.items()]


def owner_tiles(tag, k: int, w: int):
    """Of a tie case: "split" when the two tied k-mers end in different tiles (one before the seam, one at or behind it), "halo" when both
    end before the seam and a window over both ends at or behind it (the later tile imports both), else None."""
    _, S, p, d = tag
    if p + k - 1 < S <= p + d + k - 1:
        return "split"
    if p + d + k - 1 < S <= p + k + w - 2:
        return "halo"
    return None


def _codes(buf: bytes):
    code = np.full(256, 4, dtype=np.uint8)
    for i, ch in enumerate(b"ACGT"):
        code[ch] = i
    return code[np.frombuffer(buf, dtype=np.uint8)]


def minimizer_model(buf: bytes, k: int, w: int, tie_rc: bool, rightmost: bool = False):
    """(n_total, n_fwd, n_rc) of "the minimizer of every window" on upper-case ACGT input where every other byte is a break: a window is
    k + w - 1 bases without a break; its minimizer is the k-mer of smallest canonical 2-bit value, the leftmost among equals (rightmost:
    the rule a wrong import across a seam would follow); the strand is that k-mer's own (tie_rc: a k-mer equal to its reverse complement
    counts as rc)."""
    c = _codes(buf)
    n, span = len(c), k + w - 1
    if n < span:
        return 0, 0, 0
    nk = n - k + 1
    f = np.zeros(nk, dtype=np.uint64)
    r = np.zeros(nk, dtype=np.uint64)
    for j in range(k):
        x = (c[j: j + nk] & 3).astype(np.uint64)
        f = (f << np.uint64(2)) | x
        r = r | ((np.uint64(3) - x) << np.uint64(2 * j))
    canon = np.minimum(f, r)
    is_rc = ~(f < r) if tie_rc else (f > r)
    bad = np.concatenate(([0], np.cumsum(c > 3)))
    ok = (bad[span:] - bad[:n - span + 1]) == 0                       # window starting at i
    win = np.lib.stride_tricks.sliding_window_view(canon, w)          # nk - w + 1 = n - span + 1 windows
    if rightmost:
        arg = w - 1 - np.argmin(win[:, ::-1], axis=1)
    else:
        arg = np.argmin(win, axis=1)
    chosen_rc = is_rc[np.arange(len(arg)) + arg]
    n_total = int(ok.sum())
    n_rc = int((chosen_rc & ok).sum())
    return n_total, n_total - n_rc, n_rc


# ---- k = 33 .. 255 ---------------------------------------------------------------------------------------------------------------------

WK_TILE, WK_ROW, WK_WAVE = 4096, 256, 1024   # wide_canonical_reduce_kernel: bytes per tile (kWkTile), per row of 16 lanes, per wave of 64
WIDE_N = 2 * WK_TILE + 300
# row, wave and tile seams of the first tile, the same behind the second tile's start, and the tile seam 300 bytes before the input ends
WIDE_SEAMS = (WK_ROW, WK_WAVE, WK_TILE, WK_TILE + WK_ROW, WK_TILE + WK_WAVE, 2 * WK_TILE)
WIDE_KS = (33, 48, 49, 64, 255)
WIDE_TIE_KS = (34, 64, 255)


def wide_input(seed: int = 0) -> np.ndarray:
    """2 x 4096 + 300 random upper-case ACGT bytes."""
    return ACGT[np.random.default_rng(0x3D1DE + seed).integers(0, 4, WIDE_N)].copy()


def wide_break_offsets(k: int, n: int = WIDE_N, seams=WIDE_SEAMS):
    """(seam, off) for every off of [seam - k - 18, seam + 18] inside the input."""
    for S in seams:
        for off in range(max(0, S - k - 18), min(n, S + 19)):
            yield S, off


def wide_reference(buf: bytes, k: int) -> dict:
    """CanonicalKmers with 33 <= k <= 255 restated in numpy for upper-case ACGT input where every other byte is a break: a window is valid
    iff it holds no break; the strand comes from the first position at which the k-mer and its reverse complement differ, none (the k-mer is
    its own reverse complement) counting as rc; the bin is the leading six bases of the chosen strand.  Pinned against the literal
    iterator in test_wide_seams_emu.py."""
    c = _codes(buf).astype(np.int8)
    n = len(c)
    st = {"n_total": 0, "n_fwd": 0, "n_rc": 0, "sum": 0, "xor": 0, "hist": np.zeros(4096, dtype=np.uint64)}
    if n < k:
        return st
    bad = np.concatenate(([0], np.cumsum(c > 3)))
    starts = np.flatnonzero((bad[k:] - bad[:n - k + 1]) == 0)
    is_rc = np.ones(len(starts), dtype=bool)               # no difference found: rc
    open_ = np.arange(len(starts))
    for j in range(k):
        if not len(open_):
            break
        a = c[starts[open_] + j]
        b = 3 - c[starts[open_] + k - 1 - j]
        differ = a != b
        is_rc[open_[differ]] = a[differ] > b[differ]
        open_ = open_[~differ]
    bins = np.zeros(len(starts), dtype=np.int64)
    for m in range(6):
        bins = bins * 4 + np.where(is_rc, 3 - c[starts + k - 1 - m], c[starts + m])
    st["n_total"] = len(starts)
    st["n_rc"] = int(is_rc.sum())
    st["n_fwd"] = st["n_total"] - st["n_rc"]
    st["hist"] = np.bincount(bins, minlength=4096).astype(np.uint64)
    return st


def wide_tie_insert(k: int, seed: int = 0) -> bytes:
    """k bases whose first 32 equal the reverse complement of their last 32 (the packed-stream kernel cannot tell the strand from 32 bases
    and hands the launch to the byte-walking kernel): h + rc(h) with |h| = min(32, k // 2), padded in the middle to k."""
    rng = np.random.default_rng(0x71E + 7 * k + seed)
    h = ACGT[rng.integers(0, 4, min(32, k // 2))].tobytes()
    pad = ACGT[rng.integers(0, 4, k - 2 * len(h))].tobytes()
    return h + pad + revcomp(h)


def wide_tie_starts(k: int, n: int = WIDE_N, seams=WIDE_SEAMS):
    """(seam, p) for every start p of [seam - k - 2, seam + 2] at which the insert lies inside the input."""
    for S in seams:
        for p in range(max(0, S - k - 2), min(n - k, S + 2) + 1):
            yield S, p


# ---- one lower-case byte ---------------------------------------------------------------------------------------------------------------

LOWER_KS = (4, 16, 17, 21, 22, 23, 24, 32)


def lower_watch_input(k: int, seed: int = 0) -> np.ndarray:
    """Three tiles of the k-mer build of k (3 stride_of(k) - 5 bytes) of upper-case ACGT with a few N and line feeds, none near a seam."""
    s = stride_of(k)
    rng = np.random.default_rng(0x10CA5E + 17 * k + seed)
    a = ACGT[rng.integers(0, 4, 3 * s - 5)].copy()
    for frac, ch in ((0.21, b"N"), (0.43, b"\n"), (0.58, b"N"), (0.77, b"\n"), (0.9, b"N")):
        a[int(frac * len(a))] = ch[0]
    return a


LOWER_TAIL_OFFSETS = (3, 4, 5, 14, 15, 16)


def lower_tail_lengths(n: int):
    """(offset, n') for the longest n' <= n whose last byte lies at offset 3, 4, 5, 14, 15 and 16 (byte 0 of a line of its own) of its
    16-byte line: the last line then holds 4, 5, 6, 15, 16 bytes and 1 byte of input - a dword that is exactly full, one byte more, a line
    with one byte of padding, a full line.  Behind byte n' the padding is lower case (the caller's fill): it is nobody's base and must not
    be watched, while the last byte itself must (the mutation audit's or_of_input_bytes findings, profiles/mutation_audit/README.md)."""
    return [(off, n - ((n - 1 - off) % 16)) for off in LOWER_TAIL_OFFSETS]


def lower_watch_positions(n: int, seams, near=(40, 24), ends: int = 48, step: int = 16):
    """Every position of the first and the last `ends` bytes and of [S - near[0], S + near[1]] around each seam, every `step`-th elsewhere."""
    keep = set(range(0, min(ends, n))) | set(range(max(0, n - ends), n)) | set(range(0, n, step))
    for S in seams:
        keep |= set(range(max(0, S - near[0]), min(n, S + near[1] + 1)))
    return sorted(keep)
