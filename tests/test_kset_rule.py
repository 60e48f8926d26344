"""The rule of the exact k-mer set algebra (needletail_amd/csrc/ntk_kset_rule.hpp) on the CPU: the header is compiled with g++ into a
stand-alone program (tests/kset_rule_main.cpp) that walks the merged order tile by tile exactly as the kernels do, and is held to
tests/_kmer_sets_model.py on all three outputs: compare's histogram and totals, every op x rule, and the order of what is emitted.  The
same program is built with -fsanitize=address,undefined and run on exactly-sized heap arrays: a search past a range's end is then a
heap overflow.  Nothing is loaded into python."""
import os
import subprocess

import numpy as np
import pytest

import _kmer_sets_model as KM

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
MAIN = os.path.join(ROOT, "tests", "kset_rule_main.cpp")
HPP = os.path.join(ROOT, "needletail_amd", "csrc", "ntk_kset_rule.hpp")
M64 = KM.M64
# both key edge values, neighbours, and keys on both sides of 2^63
NARROW = np.array([0, 1, 5, (1 << 63) - 1, 1 << 63, (1 << 63) + 7, M64 - 1, M64], dtype=np.uint64)
# {hi, lo} rows: neighbours that differ only in lo (rows 0-2, 3-4) and only in hi (1 and 4; 5 and 6), and the edges of both words
WIDE = np.array([[0, 0], [0, 1], [0, M64], [1, 0], [1, 1], [(1 << 63) - 1, 5], [1 << 63, 5], [M64, M64]], dtype=np.uint64)
UNIVERSE = {1: NARROW, 2: WIDE}
# a == b (keys 0, 2), a == b + 1 (key 1), a < b, counts at, below and above the last bin of each axis, a sum that saturates (keys 6, 7)
CA = np.array([1, 2, 3, 5, 2, 7, M64, 4], dtype=np.uint64)
CB = np.array([1, 1, 3, 2, 6, 8, 9, M64 - 3], dtype=np.uint64)
BINS_A, BINS_B = 4, 3
TILES = (1, 2, 3, 5, 8)


def _build(tmp, name, *flags):
    exe = os.path.join(tmp, name)
    r = subprocess.run(["g++", "-std=c++17", "-O1", "-g", "-Wall", "-Werror", *flags, "-o", exe, MAIN], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    return exe


@pytest.fixture(scope="module")
def exe(tmp_path_factory):
    return _build(str(tmp_path_factory.mktemp("kset_rule")), "kset_rule_main")


@pytest.fixture(scope="module")
def exe_san(tmp_path_factory):
    return _build(str(tmp_path_factory.mktemp("kset_rule_san")), "kset_rule_main_san", "-fsanitize=address,undefined",
                  "-fno-sanitize-recover=all", "-fno-omit-frame-pointer")


def _run(exe, *args):
    r = subprocess.run([exe, *map(str, args)], capture_output=True)
    assert r.returncode == 0, (r.returncode, r.stderr.decode(errors="replace")[-2000:])
    return np.frombuffer(r.stdout, dtype=np.uint64)


def _row_words(kw):
    return BINS_A * BINS_B + 13 + len(KM.OPS) * (1 + 8 * kw + 8)


def _subsets(exe, kw, tile):
    out = _run(exe, "subsets", kw, tile, BINS_A, BINS_B, *UNIVERSE[kw].reshape(-1).tolist(), *CA.tolist(), *CB.tolist())
    return out.reshape(65536, _row_words(kw))


def _rule_np(rule, a, b):
    if rule == KM.MIN:
        return np.minimum(a, b)
    if rule == KM.MAX:
        return np.maximum(a, b)
    if rule == KM.SUM:
        s = a + b
        return np.where(s < a, np.uint64(M64), s)
    return a if rule == KM.LEFT else b


_expected = {}


def _expected_subsets(kw):
    """Every row kset_rule_main's subsets mode writes, restated with numpy over all 65536 pairs at once (held to the dict model by
    test_the_numpy_restatement_is_the_model)."""
    if kw in _expected:
        return _expected[kw]
    masks = np.arange(65536)
    bit = np.arange(8)
    in_a, in_b = ((masks >> 8)[:, None] >> bit & 1).astype(bool), ((masks & 255)[:, None] >> bit & 1).astype(bool)
    ca, cb = np.where(in_a, CA, np.uint64(0)), np.where(in_b, CB, np.uint64(0))
    both, present = in_a & in_b, in_a | in_b
    rows = np.arange(65536)
    hist = np.zeros((65536, BINS_A * BINS_B), dtype=np.uint64)
    bins = np.minimum(ca, np.uint64(BINS_A - 1)) * np.uint64(BINS_B) + np.minimum(cb, np.uint64(BINS_B - 1))
    for j in range(8):
        np.add.at(hist, (rows, bins[:, j].astype(np.int64)), present[:, j].astype(np.uint64))
    z = np.uint64(0)
    sums = lambda v, m: np.where(m, v, z).sum(axis=1, dtype=np.uint64)
    n = lambda m: m.sum(axis=1).astype(np.uint64)
    totals = np.stack([n(in_a), n(in_b), n(both), n(in_a & ~in_b), n(in_b & ~in_a), sums(ca, in_a), sums(cb, in_b), sums(ca, both),
                       sums(cb, both), sums(ca, in_a & ~in_b), sums(cb, in_b & ~in_a), sums(np.minimum(ca, cb), both),
                       sums(np.maximum(ca, cb), present)], axis=1)
    parts = [hist, totals]
    uni = UNIVERSE[kw].reshape(8, kw)
    for op, rule in KM.OPS:
        if op == KM.INTERSECT:
            emit, count = both, _rule_np(rule, ca, cb)
        elif op == KM.UNION:
            emit, count = present, np.where(both, _rule_np(rule, ca, cb), np.where(in_a, ca, cb))
        elif op == KM.SUBTRACT:
            emit, count = in_a & ~in_b, ca
        else:
            emit, count = in_a & (ca > cb), ca - cb
        pos = np.cumsum(emit, axis=1) - 1
        r, c = np.nonzero(emit)
        keys, counts = np.zeros((65536, 8, kw), dtype=np.uint64), np.zeros((65536, 8), dtype=np.uint64)
        keys[r, pos[r, c]] = uni[c]
        counts[r, pos[r, c]] = count[r, c]
        parts += [n(emit)[:, None], keys.reshape(65536, 8 * kw), counts]
    _expected[kw] = np.concatenate(parts, axis=1)
    return _expected[kw]


def _model_row(a, b, kw, bins_a, bins_b, pad):
    """What the program writes for one case, from the dict model."""
    hist, totals = KM.compare(a, b, bins_a, bins_b)
    words = [hist, np.array([totals[name] for name in KM.TOTALS], dtype=np.uint64)]
    for op, rule in KM.OPS:
        keys, counts = KM.as_list(KM.apply(op, rule, a, b), kw)
        pk, pc = np.zeros(pad * kw, dtype=np.uint64), np.zeros(pad, dtype=np.uint64)
        pk[: keys.size] = keys.reshape(-1)
        pc[: counts.size] = counts
        words += [np.array([counts.size], dtype=np.uint64), pk, pc]
    return np.concatenate(words)


def _subset(kw, mask, counts):
    picks = [j for j in range(8) if mask >> j & 1]
    return KM.as_dict(UNIVERSE[kw][picks], counts[picks])


def test_header_is_plain_constexpr_cpp_and_compiles_alone(tmp_path):
    src = open(HPP).read()
    assert not any(word in src for word in ("hip_runtime", "threadIdx", "blockIdx", "__shfl", "__ballot", "__popcll", "__shared__"))
    assert not any(line.startswith("#include") and "stdint.h" not in line for line in src.splitlines())
    assert not any(word in src for word in ("double", "float")), "no floating point anywhere in the library"
    unit = tmp_path / "alone.cpp"
    unit.write_text(f'#include "{HPP}"\n' + """
constexpr uint64_t a[3] = {1, 5, 9}, b[3] = {1, 2, 9};
static_assert(ks_split<1>(a, 3, b, 3, 0) == 0 && ks_split<1>(a, 3, b, 3, 1) == 1 && ks_split<1>(a, 3, b, 3, 2) == 1, "A first on a tie");
static_assert(ks_split<1>(a, 3, b, 3, 3) == 1 && ks_split<1>(a, 3, b, 3, 4) == 2 && ks_split<1>(a, 3, b, 3, 5) == 3, "");
static_assert(ks_split<1>(a, 3, b, 3, 6) == 3 && ks_split<1>(a, 3, b, 0, 2) == 2 && ks_split<1>(a, 0, b, 3, 2) == 0, "");
constexpr uint64_t w[6] = {0, 7, 0, 8, 1, 7};
static_assert(ks_less<2>(w, w + 2) && ks_less<2>(w + 2, w + 4) && !ks_less<2>(w + 4, w) && ks_equal<2>(w, w) && !ks_equal<2>(w, w + 4), "");
static_assert(ks_lower_bound<2>(w, 3, w + 2) == 1 && ks_upper_bound<2>(w, 3, w + 2) == 2 && ks_lower_bound<1>(a, 0, b) == 0, "");
static_assert(ks_sat_add(~(uint64_t)0, 1) == ~(uint64_t)0 && ks_sat_add(3, 4) == 7 && ks_rule(KS_SUM, ~(uint64_t)0 - 1, 1) == ~(uint64_t)0, "");
static_assert(ks_bin(0, 2) == 0 && ks_bin(1, 2) == 1 && ks_bin(~(uint64_t)0, 2) == 1 && ks_bin(2, 4) == 2 && ks_bin(3, 4) == 3, "");
static_assert(ks_op_ok(KS_UNION, KS_RIGHT) && !ks_op_ok(KS_UNION, 0) && !ks_op_ok(KS_UNION, 6) && ks_op_ok(KS_SUBTRACT, 0) &&
              !ks_op_ok(KS_SUBTRACT, KS_MIN) && !ks_op_ok(KS_COUNTERS_SUBTRACT, KS_LEFT) && !ks_op_ok(0, 0) && !ks_op_ok(5, 0), "");
int main() { return 0; }
""")
    r = subprocess.run(["g++", "-std=c++17", "-Wall", "-Werror", "-pedantic", "-o", str(tmp_path / "alone"), str(unit)],
                       capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    assert subprocess.run([str(tmp_path / "alone")]).returncode == 0


@pytest.mark.parametrize("kw", (1, 2))
def test_the_numpy_restatement_is_the_model(kw):
    want = _expected_subsets(kw)
    rng = np.random.default_rng(0x51 + kw)
    picks = list(rng.integers(0, 65536, 300)) + [0, 255, 255 << 8, 65535, (1 << 8) | 1, (0x80 << 8) | 0x80, (0x40 << 8) | 0x80]
    for case in picks:
        case = int(case)
        row = _model_row(_subset(kw, case >> 8, CA), _subset(kw, case & 255, CB), kw, BINS_A, BINS_B, 8)
        assert np.array_equal(row, want[case]), (case >> 8, case & 255)


@pytest.mark.parametrize("tile", TILES)
@pytest.mark.parametrize("kw", (1, 2))
def test_every_pair_of_subsets_of_eight_keys(exe, kw, tile):
    """256 x 256 pairs of subsets at this tile length and key width: the histogram, the totals, and all twelve op x rule outputs with
    their order."""
    got, want = _subsets(exe, kw, tile), _expected_subsets(kw)
    bad = np.nonzero((got != want).any(axis=1))[0]
    assert bad.size == 0, (int(bad[0]) >> 8, int(bad[0]) & 255, np.nonzero(got[bad[0]] != want[bad[0]])[0][:8])


def _random_lists(rng, kw, n_a, n_b, pool_size, big_counts):
    if kw == 1:
        pool = np.unique(np.concatenate([rng.integers(0, 1 << 64, pool_size, dtype=np.uint64), np.array([0, M64], dtype=np.uint64)]))
    else:   # few distinct hi values, so that many neighbours share one
        rows = np.stack([rng.integers(0, 4, pool_size, dtype=np.uint64) * np.uint64(M64 // 3), rng.integers(0, 1 << 64, pool_size, dtype=np.uint64)], 1)
        rows = np.concatenate([rows, np.array([[0, 0], [M64, M64]], dtype=np.uint64)])
        pool = np.unique(rows, axis=0)   # sorted by hi, then lo
    top = (1 << 64) if big_counts else 12
    out = []
    for n in (n_a, n_b):
        pick = np.sort(rng.choice(pool.shape[0], min(n, pool.shape[0]), replace=False))
        out.append((pool[pick], rng.integers(1, top, pick.size, dtype=np.uint64)))
    return out


def _write_cases(path, cases):
    words = [np.array([len(cases)], dtype=np.uint64)]
    for kw, tile, (a, ca), (b, cb), bins_a, bins_b in cases:
        words += [np.array([kw, tile, ca.size, cb.size, bins_a, bins_b], dtype=np.uint64), a.reshape(-1), ca, b.reshape(-1), cb]
    np.concatenate(words).tofile(path)


def _random_cases(seed):
    rng = np.random.default_rng(seed)
    cases = []
    for kw in (1, 2):
        for tile, sizes in ((1, (0, 1, 7)), (3, (0, 5, 9)), (8, (7, 8, 9, 17)), (64, (63, 64, 65, 200)), (KM.TILE_WORDS // kw, (KM.TILE_WORDS // kw - 1, KM.TILE_WORDS // kw, KM.TILE_WORDS // kw + 1, 3))):
            for n_a in sizes:
                for n_b in sizes:
                    big = bool(rng.integers(0, 2))
                    a, b = _random_lists(rng, kw, n_a, n_b, max(n_a, n_b) * 3 // 2 + 2, big)
                    cases.append((kw, tile, a, b, *((2, 2) if big else (16, 5))))
    return cases


def _hold_to_the_model(got, cases):
    at = 0
    for kw, tile, (a, ca), (b, cb), bins_a, bins_b in cases:
        want = _model_row(KM.as_dict(a, ca), KM.as_dict(b, cb), kw, bins_a, bins_b, ca.size + cb.size)
        assert np.array_equal(got[at: at + want.size], want), (kw, tile, ca.size, cb.size)
        at += want.size
    assert at == got.size


def test_random_lists_at_the_tile_seams(exe, tmp_path):
    """Lengths around one and two tiles of 1, 3, 8, 64 and the kernel's own tile length, both key widths, keys 0 and 2^64 - 1 in the pool,
    counts up to 2^64 - 1 in half of the cases (sums wrap, SUM saturates)."""
    cases = _random_cases(0x52)
    _write_cases(tmp_path / "cases.bin", cases)
    _hold_to_the_model(_run(exe, "file", tmp_path / "cases.bin"), cases)


def test_a_shared_key_across_every_seam(exe, tmp_path):
    """The A element last in a tile and its B twin first in the next, at each of the first three seams, and with the roles swapped (B's
    element last, then the next key's A element first), for lists that are otherwise all-shared, disjoint or interleaved."""
    tile, cases = 8, []
    base = np.arange(10, 10 + 2 * 40, 2, dtype=np.uint64)
    one = lambda v: np.arange(1, v.size + 1, dtype=np.uint64)
    for seam in (1, 2, 3):
        for a, b in ((base, base), (base, base + np.uint64(1)), (base[::2], base[1::2])):
            # drop leading elements of one side until a shared key's A element sits at merged position seam * tile - 1
            for drop_a in range(4):
                for drop_b in range(4):
                    cases.append((1, tile, (a[drop_a:], one(a[drop_a:])), (b[drop_b:], one(b[drop_b:]) + np.uint64(3)), 8, 8))
        shared = np.array([100], dtype=np.uint64)
        for before_a in range(seam * tile - 2, seam * tile + 2):   # A = before_a small keys then the shared key; B = the shared key and more
            a = np.concatenate([np.arange(before_a, dtype=np.uint64), shared])
            b = np.concatenate([shared, np.arange(200, 220, dtype=np.uint64)])
            cases.append((1, tile, (a, one(a)), (b, one(b)), 4, 4))
            cases.append((1, tile, (b, one(b)), (a, one(a)), 4, 4))
            wide = lambda v: np.stack([v // np.uint64(50), v], 1)
            cases.append((2, tile, (wide(a), one(a)), (wide(b), one(b)), 4, 4))
    _write_cases(tmp_path / "seams.bin", cases)
    _hold_to_the_model(_run(exe, "file", tmp_path / "seams.bin"), cases)


def test_sanitized_build_runs_clean(exe, exe_san, tmp_path):
    """-fsanitize=address,undefined on the stand-alone program: the same answers, and no report."""
    cases = _random_cases(0x53)[::2]
    _write_cases(tmp_path / "cases.bin", cases)
    assert np.array_equal(_run(exe_san, "file", tmp_path / "cases.bin"), _run(exe, "file", tmp_path / "cases.bin"))
    for kw, tile in ((1, 3), (2, 2)):
        assert np.array_equal(_subsets(exe_san, kw, tile), _expected_subsets(kw))


def test_lists_that_do_not_ascend_stay_inside_their_arrays(exe_san, tmp_path):
    """Unsorted and duplicated keys: the answer is unspecified, but the sanitized walk over exactly-sized arrays reports nothing."""
    rng = np.random.default_rng(0x54)
    cases = []
    for kw in (1, 2):
        for tile in (1, 2, 3, 8, 64):
            for n_a, n_b in ((0, 9), (9, 0), (5, 5), (40, 33), (130, 70)):
                shape = (lambda n: (n,)) if kw == 1 else (lambda n: (n, 2))
                a, b = rng.integers(0, 6, shape(n_a), dtype=np.uint64), rng.integers(0, 6, shape(n_b), dtype=np.uint64)
                cases.append((kw, tile, (a, np.ones(n_a, dtype=np.uint64)), (b, np.ones(n_b, dtype=np.uint64)), 2, 2))
    _write_cases(tmp_path / "unsorted.bin", cases)
    assert _run(exe_san, "file", tmp_path / "unsorted.bin").size > 0
