"""The per-lane logic of the all-pairs MinHash comparison (needletail_amd/csrc/ntk_mhset_rank.hpp) on the CPU: the header is compiled
with g++ into a stand-alone program (tests/mhset_rank_main.cpp) that walks A in rounds of 64 with an emulated ballot, as the kernel
does, and is held to tests/_minhash_model.py's compare.  The same program is built with -fsanitize=address,undefined and run: it hands
the search exactly the cut sketches, so a probe past a sketch's end is a heap overflow."""
import itertools
import os
import subprocess

import numpy as np
import pytest

import _mhset_model as SM
import _minhash_model as M

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
MAIN = os.path.join(ROOT, "tests", "mhset_rank_main.cpp")
HPP = os.path.join(ROOT, "needletail_amd", "csrc", "ntk_mhset_rank.hpp")
FIELDS = ("n_a", "n_b", "n_shared", "n_union", "dot", "norm2_a", "norm2_b")
# both hash edge values, neighbours, and hashes on both sides of 2^63
UNIVERSE = (0, 1, 5, (1 << 63) - 1, 1 << 63, (1 << 63) + 7, M.ALL - 1, M.ALL)
CA = (2, 3, 5, 7, 11, 13, 17, 19)
CB = (23, 29, 31, 37, 41, 43, 47, 53)
CUTS = (M.ALL, UNIVERSE[3], 0)   # all, middle, 0
LENGTHS = (0, 1, 63, 64, 65, 127, 128, 129, 1000)


def _build(tmp, name, *flags):
    exe = os.path.join(tmp, name)
    r = subprocess.run(["g++", "-std=c++17", "-O1", "-g", "-Wall", "-Werror", *flags, "-o", exe, MAIN], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    return exe


@pytest.fixture(scope="module")
def exe(tmp_path_factory):
    return _build(str(tmp_path_factory.mktemp("mhset_rank")), "mhset_rank_main")


@pytest.fixture(scope="module")
def exe_san(tmp_path_factory):
    return _build(str(tmp_path_factory.mktemp("mhset_rank_san")), "mhset_rank_main_san", "-fsanitize=address,undefined",
                  "-fno-sanitize-recover=all", "-fno-omit-frame-pointer")


def _run(exe, *args):
    r = subprocess.run([exe, *map(str, args)], capture_output=True)
    assert r.returncode == 0, r.stderr.decode(errors="replace")[-2000:]
    return np.frombuffer(r.stdout, dtype=np.float64).reshape(-1, 7)


def _subsets(exe, num, cut):
    return _run(exe, "subsets", num, cut, *UNIVERSE, *CA, *CB)


def _subset(mask, counts):
    picks = [j for j in range(8) if mask >> j & 1]
    return np.array([UNIVERSE[j] for j in picks], dtype=np.uint64), np.array([counts[j] for j in picks], dtype=np.uint64)


def _write_cases(path, cases):
    words = [np.array([len(cases)], dtype=np.uint64)]
    for a, ca, b, cb, num, cut in cases:
        words += [np.array([a.size, b.size, num, cut], dtype=np.uint64), a, ca, b, cb]
    np.concatenate(words).tofile(path)


def _random_cases(seed, big_counts=False):
    """Pairs of every two lengths of LENGTHS from one pool (many hashes are shared), with 0 and 2^64 - 1 in some of them."""
    rng = np.random.default_rng(seed)
    pool = np.unique(np.concatenate([rng.integers(0, 1 << 64, 1500, dtype=np.uint64), np.array([0, M.ALL], dtype=np.uint64)]))
    top = (1 << 64) if big_counts else (1 << 20)
    cases = []
    for n_a, n_b in itertools.product(LENGTHS, LENGTHS):
        a, b = np.sort(rng.choice(pool, n_a, replace=False)), np.sort(rng.choice(pool, n_b, replace=False))
        ca, cb = rng.integers(1, top, a.size, dtype=np.uint64), rng.integers(1, top, b.size, dtype=np.uint64)
        num = [0, 1, 10, 64, 65, 500, 1000, 10 ** 6][int(rng.integers(0, 8))]
        cut = [M.ALL, int(pool[pool.size // 2]), int(pool[3]), 0][int(rng.integers(0, 4))]
        cases.append((a, ca, b, cb, num, cut))
    return cases


def test_header_has_no_device_call_and_compiles_alone(tmp_path):
    src = open(HPP).read()
    assert not any(word in src for word in ("hip_runtime", "threadIdx", "blockIdx", "__shfl", "__ballot", "__popcll", "__shared__"))
    assert not any(line.startswith("#include") and "stdint.h" not in line for line in src.splitlines())
    unit = tmp_path / "alone.cpp"
    unit.write_text(f'#include "{HPP}"\nint main() {{ const uint64_t b[2] = {{1, 2}}; return (int)ms_lower_bound(b, 2, 3) - 2; }}\n')
    r = subprocess.run(["g++", "-std=c++17", "-Wall", "-Werror", "-pedantic", "-o", str(tmp_path / "alone"), str(unit)],
                       capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    assert subprocess.run([str(tmp_path / "alone")]).returncode == 0


def test_lower_bound_at_the_ends(tmp_path):
    """p = |B| (above everything), p = 0, an empty B, and both edge values as the searched hash and as B's ends."""
    unit = tmp_path / "lb.cpp"
    unit.write_text(f'#include "{HPP}"\n' + """
int main() {
    const uint64_t top = ~(uint64_t)0, b[5] = {0, 3, 9, top - 1, top};
    if (ms_lower_bound(b, 5, 0) != 0 || ms_lower_bound(b, 5, 1) != 1 || ms_lower_bound(b, 5, top) != 4 || ms_lower_bound(b, 4, top) != 4) return 1;
    if (ms_lower_bound(b, 0, 7) != 0 || ms_lower_bound(b + 1, 2, 0) != 0 || ms_lower_bound(b, 3, 10) != 3) return 2;
    if (ms_probe(b, 4, top).shared || ms_probe(b, 4, top).p != 4 || !ms_probe(b, 5, top).shared || !ms_probe(b, 5, 0).shared) return 3;
    if (ms_probe(b + 1, 4, 0).shared || ms_probe(b, 0, 0).shared || ms_probe(b, 0, top).shared) return 4;
    if (ms_cut_length(b, 5, top) != 5 || ms_cut_length(b, 5, 0) != 1 || ms_cut_length(b + 1, 4, 0) != 0 || ms_cut_length(b, 0, 9) != 0 ||
        ms_cut_length(b, 5, 9) != 3 || ms_cut_length(b, 5, 8) != 2) return 5;
    if (ms_union(0, 5, 4, 2) != 7 || ms_union(7, 5, 4, 2) != 7 || ms_union(6, 5, 4, 2) != 6 || ms_union(8, 5, 4, 2) != 7) return 6;
    if (!ms_union_is_num(5, 5, 0) || ms_union_is_num(6, 5, 5) || ms_union_is_num(0, 5, 5)) return 7;
    return 0;
}
""")
    r = subprocess.run(["g++", "-std=c++17", "-Wall", "-Werror", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-o",
                        str(tmp_path / "lb"), str(unit)], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    assert subprocess.run([str(tmp_path / "lb")]).returncode == 0


@pytest.mark.parametrize("cut", CUTS)
def test_every_pair_of_subsets_of_eight_hashes(exe, cut):
    """256 x 256 pairs x num 0..9 at this cut, against the model; every number is a small integer, so the doubles are exact."""
    # (plain lists of Python ints: the model walks them element by element)
    sets_a = [tuple(x.tolist() for x in _subset(m, CA)) for m in range(256)]
    sets_b = [tuple(x.tolist() for x in _subset(m, CB)) for m in range(256)]
    for num in range(10):
        got = _subsets(exe, num, cut)
        assert got.shape == (65536, 7)
        want = np.array([[float(v) for v in map(M.compare(a, ca, b, cb, num, cut).get, FIELDS)] for a, ca in sets_a for b, cb in sets_b])
        bad = np.nonzero((got != want).any(axis=1))[0]
        assert bad.size == 0, (num, cut, int(bad[0]) >> 8, int(bad[0]) & 255, got[bad[0]], want[bad[0]])


def test_the_numpy_rank_rule_is_the_model(exe):
    """tests/_mhset_model.py's restatement of the rule, on a sample of the subsets and on the random pairs."""
    rng = np.random.default_rng(0x71)
    for ma, mb in rng.integers(0, 256, (400, 2)):
        (a, ca), (b, cb) = _subset(int(ma), CA), _subset(int(mb), CB)
        for num in (0, 1, 3, 8):
            for cut in CUTS:
                assert SM.rank_rule(a, ca, b, cb, num, cut) == M.compare(a, ca, b, cb, num, cut), (ma, mb, num, cut)
    for a, ca, b, cb, num, cut in _random_cases(0x72)[::3]:
        assert SM.rank_rule(a, ca, b, cb, num, cut) == M.compare(a, ca, b, cb, num, cut), (a.size, b.size, num, cut)


def _hold_to_the_model(got, cases, exact):
    assert got.shape == (len(cases), 7)
    for row, (a, ca, b, cb, num, cut) in zip(got, cases):
        want = M.compare(a, ca, b, cb, num, cut)
        for f, v in zip(FIELDS, row):
            if exact or f in FIELDS[:4]:
                assert v == want[f], (f, a.size, b.size, num, cut, v, want[f])
            else:
                assert v == pytest.approx(want[f], rel=1e-12), (f, a.size, b.size, num, cut)


def test_random_pairs_at_the_round_seams(exe, tmp_path):
    """Lengths 0, 1, 63 .. 65, 127 .. 129 and 1000 against each other, 0 and 2^64 - 1 among the hashes; counts below 2^20 make every
    partial sum an integer below 2^53, so the doubles are exact; counts up to 2^64 - 1 are held to rel 1e-12."""
    cases = _random_cases(0x73)
    assert any(a.size and a[0] == 0 for a, *_ in cases) and any(a.size and a[-1] == M.ALL for a, *_ in cases)
    _write_cases(tmp_path / "cases.bin", cases)
    _hold_to_the_model(_run(exe, "file", tmp_path / "cases.bin"), cases, exact=True)
    big = _random_cases(0x74, big_counts=True)
    _write_cases(tmp_path / "big.bin", big)
    _hold_to_the_model(_run(exe, "file", tmp_path / "big.bin"), big, exact=False)


def test_the_num_th_member_of_the_union(exe, tmp_path):
    """A shared, an A-only and a B-only hash at union position num - 1 (counted) and at position num (not counted), across a round seam."""
    base = np.arange(10, 10 + 2 * 70, 2, dtype=np.uint64)   # 70 hashes: the 64th .. 70th lie in A's second round
    one = lambda n: np.arange(1, n + 1, dtype=np.uint64)
    cases = []
    for at in (3, 63, 64, 66):
        h = base[at]
        for a, b in ((base, base[[at]]), (base, base[at + 1:]), (base[:at], base[at:]), (base, base)):   # shared; A-only; B-only; all
            position = int(np.searchsorted(np.union1d(a, b), h))
            for num in (position + 1, position):
                if num:
                    cases.append((a, one(a.size), b, one(b.size) + np.uint64(100), num, M.ALL))
    _write_cases(tmp_path / "nth.bin", cases)
    _hold_to_the_model(_run(exe, "file", tmp_path / "nth.bin"), cases, exact=True)


def test_sanitized_build_runs_clean(exe, exe_san, tmp_path):
    """-fsanitize=address,undefined on the stand-alone program: the same answers, and no report."""
    cases = _random_cases(0x75)[::2]
    _write_cases(tmp_path / "cases.bin", cases)
    assert np.array_equal(_run(exe_san, "file", tmp_path / "cases.bin"), _run(exe, "file", tmp_path / "cases.bin"))
    for num, cut in ((0, M.ALL), (3, M.ALL), (2, CUTS[1]), (1, 0)):
        assert np.array_equal(_subsets(exe_san, num, cut), _subsets(exe, num, cut))
