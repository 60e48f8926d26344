"""The rule of the seed-index library (needletail_amd/csrc/ntk_si_rule.hpp) on the CPU: tests/si_rule_main.cpp, a stand-alone g++ program,
compiled with -fsanitize=address,undefined.  It sweeps si_find, si_at_or_before and the classification over every key set of up to 6
keys from a universe of 8 values and every max_occ 0..4, held here to the definition (bisect and set membership), and sorts a set of
anchors with the rule's key and comparison, held to Python's tuple order; sorted on a key with rpos above ref_rev the output changes."""
import bisect
import os
import re
import subprocess

import pytest

import _seed_index_model as M

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "tests", "si_rule_main.cpp")
RULE_HPP = os.path.join(ROOT, "needletail_amd", "csrc", "ntk_si_rule.hpp")
SANITIZE = ["-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-fno-omit-frame-pointer"]
UNIVERSE = [i * 0x2492492492492492 for i in range(7)] + [(1 << 64) - 1]
ABSENT, REPETITIVE, HIT = 0, 1, 2


def _compile(tmp, name, flags):
    exe = os.path.join(str(tmp), name)
    r = subprocess.run(["g++", "-std=c++17", "-Wall", "-Wextra", "-Werror", *flags, "-o", exe, SRC], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    return exe


@pytest.fixture(scope="module")
def sanitized(tmp_path_factory):
    return _compile(tmp_path_factory.mktemp("si_rule"), "si_rule", SANITIZE)


def _lines(exe, mode):
    r = subprocess.run([exe, mode], capture_output=True, text=True)
    assert r.returncode == 0, (r.returncode, r.stderr[-4000:])
    return [tuple(int(t) for t in line.split()) for line in r.stdout.splitlines()]


def test_search_and_classification_match_the_definition(sanitized):
    got = _lines(sanitized, "sweep")
    want = []
    for mask in range(256):
        if bin(mask).count("1") > 6:
            continue
        keys = [UNIVERSE[i] for i in range(8) if mask >> i & 1]
        for max_occ in range(5):
            for v in range(8):
                at = bisect.bisect_left(keys, UNIVERSE[v])     # the LOWER bound: the first key that is not below the value
                if UNIVERSE[v] not in keys:
                    cls = ABSENT
                else:
                    occ = 1 + keys.index(UNIVERSE[v]) % 5
                    cls = REPETITIVE if max_occ != 0 and occ > max_occ else HIT
                want.append((mask, max_occ, v, at, cls))
        want += [(mask, v, sum(k <= UNIVERSE[v] for k in keys)) for v in range(8)]
    assert len(want) == 247 * 48 and got == want
    classes = [g[4] for g in got if len(g) == 5]
    assert {ABSENT, REPETITIVE, HIT} == set(classes)
    # occ == max_occ is kept and occ == max_occ + 1 is not: both are in the sweep
    assert (255 & ~0x81, 2, 2, 1, HIT) in got and (255 & ~0x81, 2, 3, 2, REPETITIVE) in got


def test_sort_key_orders_by_ref_rev_then_rpos_then_qpos(sanitized, tmp_path):
    got = _lines(sanitized, "sort")
    assert len(got) == len(set(got)) == 36 and got == sorted(got)
    assert len({g[0] for g in got}) == 4 and {g[1] for g in got} == {g[2] for g in got} == {0, 77, 0xFFFFFFFF}
    swapped = _lines(_compile(tmp_path, "si_rule_swapped", SANITIZE + ["-DSI_RULE_SWAPPED_KEY"]), "sort")
    assert sorted(swapped) == got and swapped != got, "a key with rpos above ref_rev is another order"
    assert swapped == sorted(got, key=lambda a: (a[1], a[0], a[2]))


def test_the_header_is_plain_cxx_and_states_the_constants():
    """No HIP, no atomics, nothing of the scaffold: g++ compiles it alone (the program above did).  Its constants are the model's and
    the public header's."""
    text = open(RULE_HPP).read()
    code = re.sub(r"//[^\n]*", "", text)
    assert re.findall(r'#include\s+[<"]([^>"]+)[>"]', text) == ["stdint.h"]
    assert not re.search(r"\bhip[A-Z_]\w*|__global__|__shared__|threadIdx|blockIdx|__syncthreads|__shfl|__ballot", code)
    assert not re.search(r"atomic|__hip_|\basm\b|__asm", code)
    assert not re.search(r"\b(?:double|float)\b", code)
    for name, value in (("SI_SORT_TILE", M.SORT_TILE), ("SI_BLOCKS_PER_CU", M.BLOCKS_PER_CU), ("SI_THREADS", M.THREADS)):
        assert re.search(rf"constexpr uint32_t {name} = {value};", text), name
    assert "SI_ABSENT = 0, SI_REPETITIVE = 1, SI_HIT = 2;" in text
    for fn in ("si_find", "si_classify", "si_ref_rev", "si_sort_key"):
        assert re.search(rf"SI_FN \w+ {fn}\(", text), fn
    # the tile is the rule header's alone: the public header exports no such constant, and the binding's copy is this one
    hdr = open(os.path.join(ROOT, "include_staged", "needletail_amd", "seed_index.h")).read()
    assert "#define" not in re.sub(r"#define NEEDLETAIL_AMD_SEED_INDEX_H", "", hdr)
    from needletail_amd import seeding
    assert seeding.SORT_TILE == M.SORT_TILE == int(re.search(r"constexpr uint32_t SI_SORT_TILE = (\d+);", text).group(1))
