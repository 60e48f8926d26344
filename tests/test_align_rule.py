"""The rule of the alignment library (needletail_amd/csrc/ntk_align_rule.hpp) on the CPU: tests/align_rule_main.cpp, a stand-alone g++
program with its own main, compiled with -fsanitize=address,undefined.  Fuzzed between parts are written here and answered by the
program twice - by the header's row-major loop, and by the DP kernel's strip sweep restated lane by lane over the same cell, band, storage
and traceback functions - and every answer is the host model's (tests/_align_model.py): H[n][m], the cells in band and the runs.  The
program is the sanitizer run: nothing loaded into Python is sanitized."""
import os
import random
import subprocess

import pytest

import _align_model as M

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "tests", "align_rule_main.cpp")
SANITIZE = ["-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-fno-omit-frame-pointer"]


@pytest.fixture(scope="module")
def sanitized(tmp_path_factory):
    exe = os.path.join(str(tmp_path_factory.mktemp("align_rule")), "align_rule")
    r = subprocess.run(["g++", "-std=c++17", "-Wall", "-Wextra", "-Werror", *SANITIZE, "-o", exe, SRC], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    return exe


def _cases():
    """(Params, ref codes, qry codes): tiny parts on every parameter edge, parts around the strips of 64 rows and the blocks of 64 columns,
    bands of 0, 1 and wider than the matrix, similar and unrelated sequences, alphabets of 2 and 5 codes."""
    rng = random.Random(11)
    cases = []

    def add(n, m, pad, alphabet, similar, scores=None):
        a, b, q, e = scores or (rng.randint(1, 6), rng.randint(1, 6), rng.randint(0, 6), rng.randint(1, 4))
        ref = [rng.randrange(alphabet) for _ in range(n)]
        qry = [rng.randrange(alphabet) for _ in range(m)]
        if similar:
            qry = (ref[rng.randint(0, 3):] + qry)[:m]
            for _ in range(m // 12):
                qry[rng.randrange(m)] = rng.randrange(alphabet)
        cases.append((M.Params(7, a, b, q, e, pad), ref, qry))

    for _ in range(400):
        add(rng.randint(1, 12), rng.randint(1, 12), rng.choice((0, 1, 2, 64)), rng.choice((2, 5)), rng.random() < 0.5)
    for scores in ((255, 255, 255, 255), (1, 1, 0, 1), (2, 4, 0, 2), (255, 1, 0, 255), (1, 255, 255, 1)):
        for _ in range(10):
            add(rng.randint(1, 40), rng.randint(1, 40), rng.choice((0, 3, 64)), 4, True, scores)
    for n, m in ((63, 63), (64, 64), (65, 65), (64, 65), (65, 64), (127, 129), (129, 127), (128, 128), (1, 130), (130, 1), (200, 70), (70, 200), (193, 193)):
        for pad in (0, 1, 5, 64, 300):
            add(n, m, pad, 4, True)
        add(n, m, 7, 5, False)
    return cases


def _ask(exe, mode, cases):
    text = "".join(" ".join(str(x) for x in (p.a, p.b, p.q, p.e, p.band_pad, len(r), len(q), *r, *q)) + "\n" for p, r, q in cases)
    r = subprocess.run([exe, mode], input=text, capture_output=True, text=True)
    assert r.returncode == 0, (r.returncode, r.stderr[-4000:])
    return [[int(t) for t in line.split()] for line in r.stdout.splitlines()]


@pytest.mark.parametrize("mode", ["segment", "sweep"])
def test_fuzzed_segments_match_the_model(sanitized, mode):
    cases = _cases()
    got = _ask(sanitized, mode, cases)
    assert len(got) == len(cases) > 500
    for (p, ref, qry), line in zip(cases, got):
        want = M.segment(ref, qry, p)
        runs = [n << 4 | op for op, n in want.runs]
        assert line == [want.score, want.cells, len(runs), *runs], (mode, p, len(ref), len(qry))
        assert want.in_band and want.score == M.score_of(want.runs, p)


def test_the_program_refuses_other_modes(sanitized):
    assert subprocess.run([sanitized, "other"], input="", capture_output=True, text=True).returncode == 2
