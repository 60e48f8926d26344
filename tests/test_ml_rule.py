"""The rule of the minimizer-list library (needletail_amd/csrc/ntk_ml_rule.hpp) on the CPU: tests/ml_rule_main.cpp, a stand-alone g++
program, takes window ends tile by tile as ml_select_kernel does - staged pairs, the doubling, two overlapping ranges per window, the
word of every end - and reads the spans as ml_scatter_kernel does.  It is swept exhaustively over every short array and held to the
definition (the leftmost smallest key of each window, by numpy's argmin), and run on long arrays with the kernels' own tile length
against tests/_minimizer_list_model.py.  The same program runs under -fsanitize=address,undefined."""
import os
import re
import subprocess

import numpy as np
import pytest

import _minimizer_list_model as MM

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "tests", "ml_rule_main.cpp")
RULE_HPP = os.path.join(ROOT, "needletail_amd", "csrc", "ntk_ml_rule.hpp")
WHOLE, OPEN, DELTA = 0x100, 0x200, 0xFF


def _compile(tmp, name, flags):
    exe = os.path.join(str(tmp), name)
    r = subprocess.run(["g++", "-std=c++17", "-Wall", "-Wextra", "-Werror", *flags, "-o", exe, SRC], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    return exe


@pytest.fixture(scope="module")
def program(tmp_path_factory):
    return _compile(tmp_path_factory.mktemp("ml_rule"), "ml_rule", ["-O2"])


@pytest.fixture(scope="module")
def sanitized(tmp_path_factory):
    return _compile(tmp_path_factory.mktemp("ml_rule_san"), "ml_rule_san",
                    ["-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-fno-omit-frame-pointer"])


def by_definition(sym, w):
    """sym[case, end] in 0..3 (3: not valid) -> (whole, picked, opens, span) per case and end, from the definition alone."""
    cases, n = sym.shape
    whole = np.zeros((cases, n), dtype=bool)
    picked = np.full((cases, n), -1, dtype=np.int64)
    for e in range(w - 1, n):
        win = sym[:, e - w + 1: e + 1]
        whole[:, e] = (win != 3).all(axis=1)
        picked[:, e] = e - w + 1 + np.argmin(win, axis=1)    # the first of equal keys: the leftmost
    opens = whole.copy()
    opens[:, 1:] &= ~(whole[:, :-1] & (picked[:, :-1] == picked[:, 1:]))
    span = np.zeros((cases, n), dtype=np.int64)
    run = np.zeros(cases, dtype=np.int64)     # the windows behind end e that continue the entry of e: walked from the right
    for e in range(n - 1, -1, -1):
        span[:, e] = np.where(opens[:, e], 1 + run, 0)
        run = np.where(whole[:, e] & ~opens[:, e], run + 1, 0)
    return whole, picked, opens, span


def arrays(length):
    code = np.arange(1 << 2 * length, dtype=np.int64)
    return np.stack([(code >> (2 * i)) & 3 for i in range(length)], axis=1)


@pytest.mark.parametrize("tile", [4, 1024])
def test_every_short_array_matches_the_definition(program, tile):
    """Every array of length <= 9 over three keys with every validity pattern, w = 1..9: argmin, open flag and span.  tile 4 puts a
    tile seam at every fourth end; 1024 is the kernels' tile."""
    r = subprocess.run([program, "sweep", str(tile)], capture_output=True)
    assert r.returncode == 0, r.stderr[-2000:]
    got = np.frombuffer(r.stdout, dtype="<u2").astype(np.int64)
    at = 0
    for w in range(1, 10):
        for length in range(1, 10):
            sym = arrays(length)
            part = got[at: at + sym.size].reshape(sym.shape)
            at += sym.size
            whole, picked, opens, span = by_definition(sym, w)
            assert np.array_equal((part & WHOLE) != 0, whole), (w, length)
            assert np.array_equal((part & OPEN) != 0, opens), (w, length)
            ends = np.arange(length)[None, :]
            assert np.array_equal(np.where(whole, ends - (part & DELTA), -1), np.where(whole, picked, -1)), (w, length)
            assert np.array_equal(part >> 12, span), (w, length)
            assert span.max() <= w and np.array_equal(part[~whole], np.zeros_like(part[~whole]))
    assert at == got.size


def _cases(seed, n_cases=24):
    """Long arrays with the kernels' tile and with short ones: few distinct values (ties), runs of one value, gaps of every length
    around w, w up to 256, both orders."""
    rng = np.random.default_rng(seed)
    out = []
    for i in range(n_cases):
        w = int([1, 2, 3, 11, 16, 17, 64, 255, 256][i % 9])
        tile = int([1024, 1024, 7, 300][i % 4])
        n = int(rng.integers(1, 5000))
        values = rng.integers(0, [2, 5, 1 << 62][i % 3], n, dtype=np.uint64)
        if i % 5 == 0:
            values[:] = values[0]
        valid = np.ones(n, dtype=bool)
        for _ in range(int(rng.integers(0, 12))):
            s = int(rng.integers(0, n))
            valid[s: s + int(rng.integers(1, 3))] = False
        if n > 2 * w + 2:
            valid[w: w + 1] = False           # a run of exactly w - 1 valid ends in front of it, then w, then w + 1
            valid[2 * w + 1: 2 * w + 2] = False
        out.append((i % 2, w, tile, values, valid))
    return out


def _run(exe, cases):
    text = "".join(f"{order} {w} {tile} {len(v)}\n" + " ".join(f"{int(x):x}" if ok else "-" for x, ok in zip(v, valid)) + "\n"
                   for order, w, tile, v, valid in cases)
    r = subprocess.run([exe], input=text, capture_output=True, text=True)
    assert r.returncode == 0, (r.returncode, r.stderr[-4000:])
    return [np.array([int(t, 16) for t in line.split()], dtype=np.int64) for line in r.stdout.splitlines()]


def _hold(got, case):
    order, w, tile, values, valid = case
    whole, picked = MM.windows(values, valid, w, order)
    assert np.array_equal((got & WHOLE) != 0, whole), (w, tile)
    ends = np.arange(values.size)
    assert np.array_equal((ends - (got & DELTA))[whole], picked[whole]), (w, tile)
    opens = whole & ~(np.concatenate([[False], whole[:-1]]) & (np.concatenate([[-1], picked[:-1]]) == picked))
    assert np.array_equal((got & OPEN) != 0, opens), (w, tile)
    cont = whole & ~opens
    span = np.zeros(values.size, dtype=np.int64)
    run = 0
    for e in range(values.size - 1, -1, -1):
        span[e] = 1 + run if opens[e] else 0
        run = run + 1 if cont[e] else 0
    assert np.array_equal(got >> 16, span), (w, tile)
    assert span.max() <= w


def test_long_arrays_match_the_model(program):
    cases = _cases(0x3117)
    got = _run(program, cases)
    assert len(got) == len(cases)
    for g, c in zip(got, cases):
        _hold(g, c)


def test_the_same_program_under_the_sanitizers(sanitized):
    cases = _cases(0x3118, 12)
    for g, c in zip(_run(sanitized, cases), cases):
        _hold(g, c)


def test_the_header_is_plain_cxx_and_states_the_constants():
    """No HIP, no atomics, nothing of the scaffold: g++ compiles it alone (the program above did).  Its constants are the public
    header's and the model's, and its hash is the scaffold's, text for text."""
    text = open(RULE_HPP).read()
    code = re.sub(r"//[^\n]*", "", text)
    assert re.findall(r'#include\s+[<"]([^>"]+)[>"]', text) == ["stdint.h"]
    assert not re.search(r"\bhip[A-Z_]\w*|__global__|__shared__|threadIdx|blockIdx|__syncthreads|__shfl|__ballot", code)
    assert not re.search(r"atomic|__hip_|\basm\b|__asm", code)
    assert not re.search(r"\b(?:double|float)\b", code)
    assert not re.search(r"hip(?:Host)?(?:Malloc|Free)\b|ntk_wide_walk", text)
    for name, value in (("ML_W_MAX", MM.W_MAX), ("ML_TILE", MM.TILE), ("ML_BLOCKS_PER_CU", MM.BLOCKS_PER_CU), ("ML_THREADS", 256)):
        assert re.search(rf"constexpr uint32_t {name} = {value};", text), name
    assert "ML_ORDER_LEX = 0, ML_ORDER_HASH = 1;" in text and "ML_XOR = 0x9E3779B97F4A7C15ull;" in text and MM.XOR == 0x9E3779B97F4A7C15
    consumer = open(os.path.join(ROOT, "needletail_amd", "csrc", "ntk_consumer.hpp")).read()
    body = lambda t, name: re.sub(r"\s+", " ", re.search(name + r"\(uint64_t x\)\s*\{(.*?)\n\}", t, re.S).group(1))   # noqa: E731
    assert body(text, "ml_fmix64") == body(consumer, "fmix64")
    hdr = open(os.path.join(ROOT, "include", "needletail_amd", "minimizer_list.h")).read()
    assert "#define NTK_MINIMIZER_LIST_W_MAX 256u" in hdr and "#define NTK_MINIMIZER_LIST_XOR 0x9E3779B97F4A7C15ull" in hdr
