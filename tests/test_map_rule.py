"""The rule of the mapping library (needletail_amd/csrc/ntk_map_rule.hpp) on the CPU: tests/map_rule_main.cpp, a stand-alone g++ program
with its own main, compiled with -fsanitize=address,undefined.  The sweeps are written here and answered by the program: mp_lg8 over
every v below 2^12, every 2^e and its neighbours and random 32-bit v; the overlap predicate at its boundary; mp_mapq up to
score = 2^31 - 1, cnt = 2^23 and n_sub = 65534; the rank key; eligibility at its boundary; the steps on both strands; the search.
Every answer is the host model's (tests/_mapping_model.py).  Without the cap of pen by cnt the output changes.  The program is the sanitizer
run: nothing loaded into Python is sanitized."""
import os
import re
import subprocess

import numpy as np
import pytest

import _mapping_model as M

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "tests", "map_rule_main.cpp")
RULE_HPP = os.path.join(ROOT, "needletail_amd", "csrc", "ntk_map_rule.hpp")
SANITIZE = ["-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-fno-omit-frame-pointer"]
TOP = (1 << 32) - 1


def _compile(tmp, name, flags):
    exe = os.path.join(str(tmp), name)
    r = subprocess.run(["g++", "-std=c++17", "-Wall", "-Wextra", "-Werror", *flags, "-o", exe, SRC], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    return exe


@pytest.fixture(scope="module")
def sanitized(tmp_path_factory):
    return _compile(tmp_path_factory.mktemp("map_rule"), "map_rule", SANITIZE)


def _ask(exe, mode, cases):
    text = "".join(" ".join(str(x) for x in c) + "\n" for c in cases)
    r = subprocess.run([exe, mode], input=text, capture_output=True, text=True)
    assert r.returncode == 0, (r.returncode, r.stderr[-4000:])
    got = [tuple(int(t) for t in line.split()) for line in r.stdout.splitlines()]
    answers = 2 if mode == "step" else 1
    assert len(got) == len(cases) and [g[:-answers] for g in got] == [tuple(c) for c in cases]
    return got


def _v_sweep():
    v = set(range(1, 1 << 12)) | {TOP}
    for e in range(32):
        v |= {x for x in ((1 << e) - 1, 1 << e, (1 << e) + 1) if 1 <= x <= TOP}
    v |= {int(x) for x in np.random.default_rng(8).integers(1, 1 << 32, size=2000)}
    return sorted(v)


def test_lg8_matches_the_model(sanitized):
    got = _ask(sanitized, "lg8", [(v,) for v in _v_sweep()])
    assert got == [(v, M.lg8(v)) for v in _v_sweep()] and len(got) > 6000
    assert (1, 0) in got and (2, 256) in got and (3, 405) in got and (TOP, 32 * 256 - 1) in got


def _overlap_sweep():
    cases = []
    for mask in (0, 1, 499, 500, 501, 999, 1000):
        for qs_j, qe_j in ((40, 140), (0, 15), (0, TOP)):
            for qs_i in (0, 39, 40, 41, 99, 100, 101, 139, 140, 141):
                for length in (15, 16, 79, 80, 81, 100, 200):
                    cases.append((qs_i, qs_i + length, qs_j, qe_j, mask))
    cases += [(100, 180, 40, 140, 500), (99, 179, 40, 140, 500), (TOP - 15, TOP, 0, TOP, 1000), (TOP - 15, TOP, 0, TOP, 999), (0, TOP, 0, TOP, 1000)]
    return cases


def test_the_overlap_predicate_matches_the_model(sanitized):
    cases = _overlap_sweep()
    got = _ask(sanitized, "overlap", cases)
    assert got == [c + (int(M.overlap(*c)),) for c in cases]
    assert (100, 180, 40, 140, 500, 0) in got and (99, 179, 40, 140, 500, 1) in got, "ol * 1000 == mask * min is no overlap"
    assert 200 < sum(g[-1] for g in got) < len(got) - 200


def _mapq_sweep():
    cases = []
    for score in (1, 2, 39, 40, 41, 99, 100, 101, 150, 1000, 65535, 1 << 20, (1 << 31) - 1):
        for cnt in (1, 2, 9, 10, 11, 1 << 23):
            for subsc in (0, 1, 39, 40, 41, score // 2, score - 1, score):
                for n_sub in (0, 1, 2, 10, 1000, 65534):
                    for min_sc in (1, 40, 150):
                        cases.append((score, cnt, subsc, n_sub, min_sc))
    return cases


def test_mapq_matches_the_model(sanitized, tmp_path):
    cases = _mapq_sweep()
    got = _ask(sanitized, "mapq", cases)
    assert got == [c + (M.mapq(*c),) for c in cases] and len(got) > 10000
    assert ((1 << 31) - 1, 1 << 23, 0, 65534, 40) + (M.mapq((1 << 31) - 1, 1 << 23, 0, 65534, 40),) in got
    seen = {g[-1] for g in got}
    assert {0, 60} <= seen and len(seen) > 40, "the clamps and what lies between them"
    wrong = _ask(_compile(tmp_path, "map_rule_wrong", SANITIZE + ["-DMAP_RULE_WRONG_PEN"]), "mapq", cases)
    assert wrong != got and [g[:-1] for g in wrong] == [g[:-1] for g in got]


def test_rank_key_eligibility_steps_and_search(sanitized):
    keys = [(s, c) for s in (1, 2, 100, (1 << 31) - 1) for c in (0, 1, 7, TOP)]
    got = _ask(sanitized, "key", keys)
    assert got == [k + (M.rank_key(*k),) for k in keys]
    chains = [(40, 3), (40, 1), (90, 7), (15, 0), (90, TOP)]
    assert sorted(chains, key=lambda a: M.rank_key(*a)) == sorted(chains, key=lambda a: (-a[0], a[1])), "ascending keys: score descending, index ascending"
    assert len({M.rank_key(*k) for k in keys}) == len(keys)
    el = [(s, p, pm) for p in (1, 500, 1000, (1 << 31) - 1) for pm in (0, 1, 800, 999, 1000) for s in (1, p * pm // 1000, -(-p * pm // 1000), max(1, -(-p * pm // 1000) - 1), p)
          if s >= 1]
    got = _ask(sanitized, "eligible", el)
    assert got == [c + (int(c[0] * 1000 >= c[2] * c[1]),) for c in el] and (800, 1000, 800, 1) in got and (799, 1000, 800, 0) in got
    k = 15
    steps = [(rev, 1000, 1000, 1000 + dr, 1000 - dq if rev else 1000 + dq, k) for rev in (0, 1) for dr in (0, 1, k - 1, k, k + 1, 500) for dq in (-1, 0, 1, k - 1, k, k + 1, 700)]
    steps += [(0, 0, 0, TOP, TOP, 255), (1, 0, TOP, TOP, 0, 255), (0, 0, 0, TOP, 1, 1)]
    got = _ask(sanitized, "step", steps)
    want = []
    for rev, rj, qj, ri, qi, kk in steps:
        dr, dq = ri - rj, (qj - qi if rev else qi - qj)
        ok = dr >= 1 and dq >= 1
        want.append((rev, rj, qj, ri, qi, kk, min(dr, dq, kk) if ok else 0, max(dr, dq) if ok else 0))
    assert got == want and (0, 0, 0, TOP, TOP, 255, 255, TOP) in got
    off = [2, 2, 5, 5, 5, 9]
    assert _ask(sanitized, "search", [(x,) for x in range(11)]) == [(x, sum(o <= x for o in off)) for x in range(11)]


def test_the_header_is_plain_cxx_and_states_the_constants():
    """No HIP, no atomics, nothing of the scaffold, no floating point: g++ compiles it alone (the program above did).  Its constants are
    the model's and the binding's; the public header exports none of the untuned ones."""
    text = open(RULE_HPP).read()
    code = re.sub(r"//[^\n]*", "", text)
    assert re.findall(r'#include\s+[<"]([^>"]+)[>"]', text) == ["stdint.h"]
    assert not re.search(r"\bhip[A-Z_]\w*|__global__|__shared__|threadIdx|blockIdx|__syncthreads|__shfl|__ballot", code)
    assert not re.search(r"atomic|__hip_|\basm\b|__asm", code)
    assert not re.search(r"\b(?:double|float)\b", code)
    for name, value in (("MP_THREADS", M.THREADS), ("MP_BLOCKS_PER_CU", M.BLOCKS_PER_CU), ("MP_LDS_CHAINS", M.LDS_CHAINS)):
        assert re.search(rf"constexpr uint32_t {name} = {value};", text), name
    assert "MP_NONE = 0xFFFFFFFFu;" in text and "MP_READ_CHAINS = (uint64_t)1 << 16;" in text and "MP_ROW_WORDS = 16;" in text
    words = re.search(r"constexpr uint32_t MP_QS = 0,(.*?);", text, re.S).group(0)
    assert [int(v) for v in re.findall(r"= (\d+)", words)] == list(range(15))
    assert [n.lower() for n in re.findall(r"MP_(\w+) =", words)] == list(M.ROW[:15])
    for fn in ("mp_ilog2", "mp_lg8", "mp_step", "mp_overlap", "mp_eligible", "mp_mapq", "mp_rank_key", "mp_at_or_before"):
        assert re.search(rf"MP_FN \w+ {fn}\(", text), fn
    hdr = open(os.path.join(ROOT, "include_pending", "needletail_amd", "mapping.h")).read()
    assert "#define" not in re.sub(r"#define NEEDLETAIL_AMD_MAPPING_H", "", hdr)
    from needletail_amd import mapping
    assert mapping.LDS_CHAINS == M.LDS_CHAINS and mapping.READ_CHAINS == M.READ_CHAINS and mapping.ROW == M.ROW
    assert (mapping.PRIMARY, mapping.SECONDARY) == (M.PRIMARY, M.SECONDARY)
