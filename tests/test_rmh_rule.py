"""The guess / accept / raise rule of the per-record MinHash sketches (needletail_amd/csrc/ntk_rmh_rule.hpp) on the CPU: the header is
compiled with g++ into a stand-alone program (tests/rmh_rule_main.cpp) that runs a record's rounds as the library does - filter,
distinct, accept, raise - and is held to the plain cut, exhaustively on small universes and against tests/_minhash_model.py.  The same
program is built with -fsanitize=address,undefined and run directly."""
import math
import os
import subprocess

import numpy as np
import pytest

import _minhash_model as M

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
MAIN = os.path.join(ROOT, "tests", "rmh_rule_main.cpp")
HPP = os.path.join(ROOT, "needletail_amd", "csrc", "ntk_rmh_rule.hpp")
ALL = M.ALL
# both hash edge values and their neighbours, small hashes a raise multiplies, and hashes on both sides of 2^63
UNIVERSE = (0, 1, 2, 7, 1000, (1 << 62) + 5, (1 << 63) - 1, 1 << 63, ALL - 1, ALL)
ALLPASS, MIN_RAISE = 4, 4
want = lambda num: 2 * num + 16


def _build(tmp, name, *flags):
    exe = os.path.join(tmp, name)
    r = subprocess.run(["g++", "-std=c++17", "-O1", "-g", "-Wall", "-Werror", *flags, "-o", exe, MAIN], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    return exe


@pytest.fixture(scope="module")
def exe(tmp_path_factory):
    return _build(str(tmp_path_factory.mktemp("rmh_rule")), "rmh_rule_main")


@pytest.fixture(scope="module")
def exe_san(tmp_path_factory):
    return _build(str(tmp_path_factory.mktemp("rmh_rule_san")), "rmh_rule_main_san", "-fsanitize=address,undefined",
                  "-fno-sanitize-recover=all", "-fno-omit-frame-pointer")


def _run(exe, *args):
    r = subprocess.run([exe, *map(str, args)], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-2000:]
    return r.stdout


def test_header_has_no_device_call_and_compiles_alone(tmp_path):
    src = open(HPP).read()
    assert not any(word in src for word in ("hip_runtime", "threadIdx", "blockIdx", "__shfl", "__ballot", "__device__", "__shared__"))
    assert not any(line.startswith("#include") and "stdint.h" not in line for line in src.splitlines())
    unit = tmp_path / "alone.cpp"
    unit.write_text(f'#include "{HPP}"\nstatic_assert(rmh_guess(10, 1000) == kRmhAll && rmh_accept(kRmhAll, 0, 5) && !rmh_accept(9, 4, 5), "");\n'
                    "int main() { return rmh_raise(5, 0, 3) == kRmhAll ? 0 : 1; }\n")
    r = subprocess.run(["g++", "-std=c++17", "-Wall", "-Werror", "-pedantic", "-o", str(tmp_path / "alone"), str(unit)],
                       capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    assert subprocess.run([str(tmp_path / "alone")]).returncode == 0
    hdr = open(os.path.join(ROOT, "include", "needletail_amd_record_minhash.h")).read()
    assert f"#define NTK_RECORD_MINHASH_ALLPASS {ALLPASS}ull" in hdr and f"kRmhAllPass = {ALLPASS};" in src
    assert f"kRmhMinRaise = {MIN_RAISE};" in src and "return 2 * num + 16;" in src


def test_every_multiset_of_eight_from_ten(exe):
    """Every multiset of at most 8 hashes of the universe x num 1..9 x every first threshold of the universe and ~0: the program fails
    unless every accepted result is the plain cut, every raise rises and every record's rounds end."""
    cases, rounds_max, raises = map(int, _run(exe, "walk", *UNIVERSE).split())
    assert cases == sum(math.comb(10 + n - 1, n) for n in range(9)) * 9 * 11
    assert 2 <= rounds_max <= 33 and raises > cases // 4   # a raise at least quadruples: 32 of them pass 2^64 from 1


def _trace(exe, num, tau, hashes):
    lines = _run(exe, "trace", num, tau, *hashes).splitlines()
    taus = [int(x) for x in lines[0].split()]
    pairs = np.array([[int(x) for x in line.split()] for line in lines[1:]], dtype=np.uint64).reshape(-1, 2)
    return taus, pairs[:, 0], pairs[:, 1]


def test_rounds_against_the_model(exe):
    """Random records with repeats, first thresholds from far too low to ~0: the result is the model's cut, the thresholds rise strictly,
    each by at least the factor, and only ~0 accepts fewer than num hashes."""
    rng = np.random.default_rng(0x524D48)
    for _ in range(300):
        distinct = rng.integers(0, 1 << 64, int(rng.integers(1, 60)), dtype=np.uint64)
        hashes = rng.choice(distinct, int(rng.integers(1, 200)))
        num = int(rng.integers(1, 80))
        tau = [0, 1, int(rng.integers(0, 1 << 64, dtype=np.uint64)) >> int(rng.integers(0, 64)), ALL][int(rng.integers(0, 4))]
        taus, h, c = _trace(exe, num, tau, hashes.tolist())
        u, n = np.unique(hashes, return_counts=True)
        wh, wc = M.cut(u, n, num=num)
        assert np.array_equal(h, wh) and np.array_equal(c, wc), (num, tau)
        assert taus[0] == tau and all(b > a and (b == ALL or b >= MIN_RAISE * max(a, 1)) for a, b in zip(taus, taus[1:]))
        assert taus[-1] == ALL or h.size == num
        assert len(taus) <= 33


def test_the_guess(exe):
    """~0 up to max(ALLPASS * num, 2 num + 16) window ends, then the hash below which 2 num + 16 of n are expected; monotone in n."""
    for num in (1, 2, 16, 64, 1000, 1 << 20):
        top = max(ALLPASS * num, want(num))
        lo = max(0, top - 40)
        got = [int(x) for x in _run(exe, "guess", num, top + 3000).split()]
        assert all(g == ALL for g in got[:top + 1]) and got[top + 1] != ALL, num
        assert got[lo:] == [ALL if n <= top else (ALL // n) * want(num) for n in range(lo, top + 3001)]
        assert all(a >= b for a, b in zip(got, got[1:])), "a longer record never gets a higher threshold"
        # the expectation: want(num) of n hashes lie at or below the guess, within one
        n = top + 3000
        assert abs(got[n] / 2 ** 64 * n - want(num)) < 1


def test_sanitized_build_runs_clean(exe, exe_san):
    """-fsanitize=address,undefined on the stand-alone program, run directly: the same answers, and no report."""
    assert _run(exe_san, "walk", *UNIVERSE) == _run(exe, "walk", *UNIVERSE)
    rng = np.random.default_rng(0x5A)
    for num, tau in ((1, 0), (9, ALL - 1), (64, 12345), (3, ALL)):
        hashes = rng.integers(0, 1 << 64, 50, dtype=np.uint64).tolist() + [0, ALL, ALL]
        assert _run(exe_san, "trace", num, tau, *hashes) == _run(exe, "trace", num, tau, *hashes)
    assert _run(exe_san, "guess", 1000, 5000) == _run(exe, "guess", 1000, 5000)
