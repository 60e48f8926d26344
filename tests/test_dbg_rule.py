"""The rule of the compacted de Bruijn graph (needletail_amd/csrc/ntk_dbg_rule.hpp) on the CPU: tests/dbg_rule_main.cpp, a stand-alone
g++ program, walks the directory, the bucket search, the edge byte, the mate, the link and the ranking rounds step by step as the kernels
of ntk_dbg.hip do, and is held to tests/_dbg_model.py (strings, a set, one walk per unitig) on edges, totals, k-mer rows, unitig rows
and spelled bases.  On every case: a bit is set iff its mate's is, and the unitigs' k-mers add up to n.  The same program runs under
-fsanitize=address,undefined on heap arrays of exactly the library's sizes, also on lists that do not ascend."""
import itertools
import os
import subprocess

import numpy as np
import pytest

import _dbg_model as DM

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "tests", "dbg_rule_main.cpp")
RULE_HPP = os.path.join(ROOT, "needletail_amd", "csrc", "ntk_dbg_rule.hpp")


def _compile(tmp, name, flags):
    exe = os.path.join(str(tmp), name)
    r = subprocess.run(["g++", "-std=c++17", "-Wall", "-Wextra", "-Werror", *flags, "-o", exe, SRC], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    return exe


@pytest.fixture(scope="module")
def program(tmp_path_factory):
    return _compile(tmp_path_factory.mktemp("dbg_rule"), "dbg_rule", ["-O2"])


@pytest.fixture(scope="module")
def sanitized(tmp_path_factory):
    return _compile(tmp_path_factory.mktemp("dbg_rule_san"), "dbg_rule_san",
                    ["-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-fno-omit-frame-pointer"])


def run(exe, cases):
    """cases: (k, keys, counts).  Returns one dict per case: what the program printed."""
    text = []
    for k, keys, counts in cases:
        text.append(f"{k} {len(keys)}")
        text.extend(f"{int(a):x} {int(b):x}" for a, b in zip(keys, counts))
    r = subprocess.run([exe], input="\n".join(text) + "\n", capture_output=True, text=True)
    assert r.returncode == 0, (r.returncode, r.stderr[-4000:])
    out, lines = [], iter(r.stdout.splitlines())
    for line in lines:
        assert line.startswith("E"), line
        cur = {"edges": np.array(line.split()[1:], dtype=np.uint8)}
        cur["totals"] = [int(v) for v in next(lines).split()[1:]]
        cur["kmer_rows"] = np.array(next(lines).split()[1:], dtype=np.uint32).reshape(-1, 2)
        u = next(lines).split()
        cur["n_unitigs"], cur["n_bases"], cur["n_rounds"], cur["mates_ok"] = int(u[1]), int(u[2]), int(u[3]), int(u[4])
        rows, spelled = [], []
        for _ in range(cur["n_unitigs"]):
            rows.append([int(v) for v in next(lines).split()[1:]])
            spelled.append(next(lines)[2:])
        cur["unitig_rows"], cur["spelled"] = np.array(rows, dtype=np.uint64).reshape(-1, 4), spelled
        out.append(cur)
    assert len(out) == len(cases)
    return out


def flat_totals(t):
    return [t["n_half_edges"], *[int(v) for v in t["deg_hist"].reshape(-1)], t["n_isolated"], t["n_tips"], t["n_branching"], t["n_self"],
            t["n_links"]]


def hold(got, k, keys, counts, name):
    g = DM.Graph(keys, counts, k)
    assert got["mates_ok"] == 1, name
    assert np.array_equal(got["edges"], g.edges), name
    assert got["totals"] == flat_totals(g.totals()), name
    assert np.array_equal(got["kmer_rows"], g.kmer_rows), name
    assert np.array_equal(got["unitig_rows"], g.unitig_rows), name
    assert got["spelled"] == g.spelled, name
    assert (got["n_unitigs"], got["n_bases"]) == (g.n_unitigs, g.n_bases), name
    assert int(got["unitig_rows"][:, 1].sum()) == len(keys), name
    return g


def test_rule_header_has_no_device_call():
    text = open(RULE_HPP).read()
    assert "hip/hip_runtime" not in text and "__global__" not in text and "threadIdx" not in text and "atomic" not in text


def test_every_subset_of_the_universe(program):
    """2^14 lists of canonical 3-mers; among them a self loop, a k-mer that targets its own reverse complement, a pair of k-mers linked on
    both sides and a cycle of three."""
    universe = DM.universe_keys()
    names = {DM.decode(int(v), 3) for v in universe}
    assert {"AAA", "ACG"} <= names
    cases = []
    for mask in range(1 << len(universe)):
        keys = universe[[(mask >> j) & 1 == 1 for j in range(len(universe))]]
        cases.append((3, keys, DM.counts_for(keys, mask)))
    got = run(program, cases)
    cycles = set()
    for mask, (res, (k, keys, counts)) in enumerate(zip(got, cases)):
        g = hold(res, k, keys, counts, f"subset {mask:#x}")
        cycles |= {int(r[1]) for r in g.unitig_rows if int(r[3]) & 1}
    assert {2, 3} <= cycles, cycles
    alone = run(program, [(3, np.array([DM.encode("AAA")], dtype=np.uint64), [5]), (3, np.array([DM.encode("ACG")], dtype=np.uint64), [5])])
    assert alone[0]["totals"][29] == 2 and alone[0]["totals"][30] == 0   # AAA: both sides lead back to it, neither is a link
    assert alone[1]["totals"][29] == 1 and alone[1]["totals"][0] == 1    # ACG -> CGT = rc(ACG), on side 0 alone


def test_random_subsets_of_all_3_mers_and_5_mers(program):
    cases = [(k, keys, DM.counts_for(keys)) for _, k, keys in DM.subset_cases()]
    for (name, _, _), res, (k, keys, counts) in zip(DM.subset_cases(), run(program, cases), cases):
        hold(res, k, keys, counts, name)


def test_sequences_at_k_15_and_31(program):
    named = list(DM.sequence_cases())
    cases = [(k, keys, DM.counts_for(keys)) for _, k, keys in named]
    for (name, _, _), res, (k, keys, counts) in zip(named, run(program, cases), cases):
        g = hold(res, k, keys, counts, name)
        if name.endswith("-cycle"):
            assert g.n_unitigs == 1 and int(g.unitig_rows[0, 3]) & 1 and int(g.unitig_rows[0, 1]) == len(keys), name
        if name.endswith("-path"):
            assert g.n_unitigs == 1 and res["n_rounds"] >= int(np.ceil(np.log2(len(keys)))), name
        if name.endswith("-repeat"):
            assert g.totals()["n_branching"] > 0, name
        if name.endswith("-empty"):
            assert res["n_unitigs"] == 0 and res["n_bases"] == 0
        if name.endswith("-one"):
            assert g.spelled == [DM.decode(int(keys[0]), k)]


def test_sanitized_walk_on_good_and_bad_lists(sanitized):
    """Address and undefined-behaviour sanitizers over the same walk: a sample of the cases above held to the model, then lists that do not
    ascend, hold a key twice or hold keys that are not canonical or wider than 2 k bits - any answer, but no report."""
    universe = DM.universe_keys()
    good = [(3, universe[[(mask >> j) & 1 == 1 for j in range(14)]], None) for mask in range(0, 1 << 14, 37)]
    good += [(k, keys, None) for _, k, keys in itertools.chain(DM.subset_cases(), DM.sequence_cases())]
    good = [(k, keys, DM.counts_for(keys)) for k, keys, _ in good]
    for i, (res, (k, keys, counts)) in enumerate(zip(run(sanitized, good), good)):
        hold(res, k, keys, counts, f"sanitized {i}")
    rng = np.random.default_rng(0xBAD)
    bad = []
    for _, k, keys in itertools.chain(DM.subset_cases(), DM.sequence_cases()):
        if len(keys) < 2:
            continue
        bad.append((k, keys[::-1].copy(), DM.counts_for(keys)))                                   # descending
        bad.append((k, rng.permutation(keys), DM.counts_for(keys)))                               # any order
        bad.append((k, np.repeat(keys, 2), DM.counts_for(np.repeat(keys, 2))))                    # every key twice
        wild = rng.integers(0, 1 << 63, len(keys), dtype=np.uint64) * np.uint64(2) + np.uint64(1)  # not canonical, all 64 bits used
        bad.append((k, wild, DM.counts_for(keys)))
        bad.append((k, np.sort(wild), DM.counts_for(keys)))
    for res, (k, keys, _) in zip(run(sanitized, bad), bad):
        assert len(res["edges"]) == len(keys) and res["n_unitigs"] <= len(keys)
