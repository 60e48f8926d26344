"""The rule of the chain library (needletail_amd/csrc/ntk_chain_rule.hpp) on the CPU: tests/ch_rule_main.cpp, a stand-alone g++ program,
compiled with -fsanitize=address,undefined.  It sweeps ch_ilog2, the gap cost and the pair predicate and score over dd of 0..4, every
2^e and 2^e +- 1, bw and bw + 1; dr and dq of 0, 1, k - 1, k, k + 1, max_dist, max_dist + 1 and negative dq; both strands; k of 1, 15 and
255 - held here to the host model (tests/_chain_model.py).  Costed with 40 / 4096 for 41 / 4096 the output changes."""
import os
import re
import subprocess

import pytest

import _chain_model as M

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "tests", "ch_rule_main.cpp")
RULE_HPP = os.path.join(ROOT, "needletail_amd", "csrc", "ntk_chain_rule.hpp")
SANITIZE = ["-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-fno-omit-frame-pointer"]
KS = (1, 15, 255)
SETS = ((5000, 500), (200, 10))


def _compile(tmp, name, flags):
    exe = os.path.join(str(tmp), name)
    r = subprocess.run(["g++", "-std=c++17", "-Wall", "-Wextra", "-Werror", *flags, "-o", exe, SRC], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    return exe


@pytest.fixture(scope="module")
def sanitized(tmp_path_factory):
    return _compile(tmp_path_factory.mktemp("ch_rule"), "ch_rule", SANITIZE)


def _lines(exe, mode):
    r = subprocess.run([exe, mode], capture_output=True, text=True)
    assert r.returncode == 0, (r.returncode, r.stderr[-4000:])
    return [tuple(int(t) for t in line.split()) for line in r.stdout.splitlines()]


def _dd_sweep():
    v = {0, 1, 2, 3, 4, (1 << 31) - 1}
    for e in range(31):
        v |= {x for x in ((1 << e) - 1, 1 << e, (1 << e) + 1) if 0 <= x < 1 << 31}
    for _, bw in SETS:
        v |= {bw, bw + 1}
    return sorted(v)


def test_ilog2_and_the_gap_cost_match_the_model(sanitized, tmp_path):
    got = _lines(sanitized, "gap")
    want = [(k, dd, M.ilog2(max(dd, 1)), M.gap_cost(dd, k)) for k in KS for dd in _dd_sweep()]
    assert len(want) == 3 * len(_dd_sweep()) > 280 and got == want
    assert (15, 10, 3, 2) in got and (15, 500, 8, 79) in got and (255, (1 << 31) - 1, 30, M.gap_cost((1 << 31) - 1, 255)) in got
    assert max(g[3] for g in got) >= 1 << 32, "the cost of the largest dd does not fit 32 bits: the rule carries it in 64"
    wrong = _lines(_compile(tmp_path, "ch_rule_wrong", SANITIZE + ["-DCH_RULE_WRONG_GAP"]), "gap")
    assert wrong != got and [g[:3] for g in wrong] == [g[:3] for g in got]


def test_the_pair_predicate_and_score_match_the_model(sanitized):
    got = _lines(sanitized, "pair")
    want = []
    for k in KS:
        for s, (max_dist, bw) in enumerate(SETS):
            p = M.Params(k, max_dist=max_dist, bw=bw)
            d = [0, 1, k - 1, k, k + 1, max_dist, max_dist + 1]
            sweep = [(dr, dq) for dr in d for dq in d] + [x for dr in d for x in ((dr, -1), (dr, -max_dist))]
            sweep += [x for a in (1, k, 100) for extra in (bw, bw + 1) for x in ((a, a + extra), (a + extra, a))]
            base = 1_000_000
            for rev in (0, 1):
                for dr, dq in sweep:
                    step = M.pair(rev, base, base, base + dr, base - dq if rev else base + dq, p)
                    gain, gap = step if step is not None else (0, 0)
                    score = 100 + gain - gap if step is not None else None
                    chained = score is not None and score > k
                    want.append((k, s, rev, dr, dq, int(step is not None), gain, gap, score if chained else k, 7 if chained else M.NONE))
    assert len(want) == 3 * 2 * 2 * (49 + 14 + 12) and got == want
    ok = [g for g in got if g[5]]
    assert 200 < len(ok) < len(got) - 200
    # both sides of every edge are in the sweep, on both strands
    for rev in (0, 1):
        assert (15, 0, rev, 5000, 5000, 1, 15, 0, 115, 7) in got and (15, 0, rev, 5001, 5001, 0, 0, 0, 15, M.NONE) in got
        assert (15, 1, rev, 100, 110, 1, 15, 2, 113, 7) in got and (15, 1, rev, 100, 111, 0, 0, 0, 15, M.NONE) in got
        assert (15, 0, rev, 14, 14, 1, 14, 0, 114, 7) in got and (15, 0, rev, 1, 0, 0, 0, 0, 15, M.NONE) in got and (15, 0, rev, 1, -1, 0, 0, 0, 15, M.NONE) in got
    # a step that costs more than it may: no candidate (the score does not exceed k)
    assert any(g[5] == 1 and g[9] == M.NONE for g in got)


def test_run_heads_order_search_and_visit_key(sanitized):
    got = _lines(sanitized, "misc")
    assert got[0] == (1, 1, 0, 1, 1) and got[1] == (1, 0, 1, 1, 0, 0)
    off = [2, 2, 5, 5, 5, 9]
    assert got[2] == tuple(sum(o <= x for o in off) for x in range(11)) + (0,)
    assert got[3] == (0, (0x7FFFFFFF - 15) << 32 | 0xFFFFFFFF, 0x7FFFFFFF << 32 | 1)
    # ascending keys visit f descending, then index ascending
    key = lambda f, i: (0x7FFFFFFF - f) << 32 | i   # noqa: E731
    anchors = [(40, 3), (40, 1), (90, 7), (15, 0)]
    assert sorted(anchors, key=lambda a: key(*a)) == sorted(anchors, key=lambda a: (-a[0], a[1]))


def test_the_header_is_plain_cxx_and_states_the_constants():
    """No HIP, no atomics, nothing of the scaffold, no floating point: g++ compiles it alone (the program above did).  Its constants are
    the model's and the binding's; the public header exports none of the untuned ones."""
    text = open(RULE_HPP).read()
    code = re.sub(r"//[^\n]*", "", text)
    assert re.findall(r'#include\s+[<"]([^>"]+)[>"]', text) == ["stdint.h"]
    assert not re.search(r"\bhip[A-Z_]\w*|__global__|__shared__|threadIdx|blockIdx|__syncthreads|__shfl|__ballot", code)
    assert not re.search(r"atomic|__hip_|\basm\b|__asm", code)
    assert not re.search(r"\b(?:double|float)\b", code)
    for name, value in (("CH_THREADS", M.THREADS), ("CH_BLOCKS_PER_CU", M.BLOCKS_PER_CU), ("CH_RING", M.RING)):
        assert re.search(rf"constexpr uint32_t {name} = {value};", text), name
    assert "CH_H_MAX = CH_RING;" in text and "CH_NONE = 0xFFFFFFFFu;" in text and "CH_READ_ANCHORS = (uint64_t)1 << 23;" in text
    assert "CH_BAD_OFFSETS = 1, CH_BAD_ORDER = 2, CH_LONG_READ = 4;" in text
    for fn in ("ch_ilog2", "ch_gap", "ch_pair", "ch_candidate", "ch_run_head", "ch_before", "ch_at_or_before", "ch_visit_key"):
        assert re.search(rf"CH_FN \w+ {fn}\(", text), fn
    hdr = open(os.path.join(ROOT, "include_pending", "needletail_amd", "chain.h")).read()
    assert "#define" not in re.sub(r"#define NEEDLETAIL_AMD_CHAIN_H", "", hdr)
    from needletail_amd import chaining
    assert chaining.H_MAX == M.RING and chaining.NONE == M.NONE
