"""The rule of the coloured k-mer index (needletail_amd/csrc/ntk_colors_rule.hpp) on the CPU: tests/colors_rule_main.cpp, a stand-alone g++
program, runs insert-or-OR and lookup over heap arrays of exactly the library's sizes, the per-record accumulation in the kernels' lane
order and the best / second pass, and is held to tests/_colors_model.py (a dict built by OR, rows by definition).  The same program runs
under -fsanitize=address,undefined."""
import os
import subprocess

import numpy as np
import pytest

import _colors_model as KM
import _count_model as CM

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "tests", "colors_rule_main.cpp")
M64 = (1 << 64) - 1


def _compile(tmp, name, flags):
    exe = os.path.join(str(tmp), name)
    r = subprocess.run(["g++", "-std=c++17", "-Wall", "-Wextra", "-Werror", *flags, "-o", exe, SRC], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    return exe


@pytest.fixture(scope="module")
def program(tmp_path_factory):
    return _compile(tmp_path_factory.mktemp("colors_rule"), "colors_rule", ["-O2"])


@pytest.fixture(scope="module")
def sanitized(tmp_path_factory):
    return _compile(tmp_path_factory.mktemp("colors_rule_san"), "colors_rule_san",
                    ["-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-fno-omit-frame-pointer"])


class Case:
    """n_colors, capacity, adds [(key, mask)], queries [key], records [[key or None]]."""

    def __init__(self, name, n_colors, capacity, adds, queries=(), records=()):
        self.name, self.n_colors, self.capacity = name, n_colors, capacity
        self.adds, self.queries, self.records = list(adds), list(queries), [list(r) for r in records]

    def text(self):
        out = [f"C {self.n_colors} {self.capacity} {len(self.adds)}"]
        out += [f"{int(k):x} {int(m):x}" for k, m in self.adds]
        out += [f"Q {len(self.queries)}", " ".join(f"{int(q):x}" for q in self.queries), f"R {len(self.records)}"]
        out += [" ".join([str(len(r))] + ["-" if w is None else f"{int(w):x}" for w in r]) for r in self.records]
        return "\n".join(out) + "\n"


def run(exe, cases):
    r = subprocess.run([exe], input="".join(c.text() for c in cases), capture_output=True, text=True)
    assert r.returncode == 0, (r.returncode, r.stderr[-4000:])
    lines, out = iter(r.stdout.splitlines()), []
    for c in cases:
        s, p, l = next(lines).split(), next(lines).split(), next(lines).split()
        assert (s[0], p[0], l[0]) == ("S", "P", "L"), c.name
        got = {"n_keys": int(s[1]), "n_dropped": int(s[2]), "n_masked_bits": int(s[3]), "slots": int(s[4]), "probe": int(s[5]),
               "side": int(s[6], 16), "per_color": [int(v) for v in p[1:]], "lookup": [int(v, 16) for v in l[1:]], "rows": [], "hits": [],
               "single": []}
        for _ in c.records:
            row, hits, single = next(lines)[2:].split("|")
            got["rows"].append([int(v) for v in row.split()])
            got["hits"].append([int(v) for v in hits.split()])
            got["single"].append([int(v) for v in single.split()])
        out.append(got)
    assert next(lines, None) is None
    return out


def hold(got, c, complete=True):
    """The program's answers against the model; complete: nothing may have been dropped."""
    model = KM.Index(c.n_colors)
    for key, m in c.adds:
        model.add([key], m)
    slots = CM.slots_for(c.capacity)
    assert (got["slots"], got["probe"]) == (slots, CM.probe_bound(slots)), c.name
    assert got["n_masked_bits"] == model.n_masked_bits, c.name
    assert got["side"] == model.masks.get(M64, 0), c.name
    if not complete:
        return model
    assert got["n_dropped"] == 0 and got["n_keys"] == model.n_keys, c.name
    assert got["per_color"] == model.per_color(), c.name
    assert got["lookup"] == [int(v) for v in model.lookup(c.queries)], c.name
    for i, rec in enumerate(c.records):
        row, hits, single = KM.screen_masks(model.lookup([w for w in rec if w is not None]), c.n_colors)
        assert got["rows"][i] == [int(v) for v in row], (c.name, i)
        assert got["hits"][i] == [int(v) for v in hits] and got["single"][i] == [int(v) for v in single], (c.name, i)
    return model


def random_case(seed, n_colors, n_keys=300, n_records=12):
    """Keys from a small universe (so they repeat), masks with 0, 1, several and all bits and some beyond n_colors, keys 0 and 2^64 - 1,
    records of 0 .. 200 windows with gaps, absent keys among them."""
    rng = np.random.default_rng(seed)
    universe = np.concatenate([rng.integers(0, 1 << 63, 150, dtype=np.uint64) * np.uint64(2) + rng.integers(0, 2, 150, dtype=np.uint64),
                               np.array([0, M64], dtype=np.uint64)])
    bits = KM.color_bits(n_colors)

    def mask():
        kind = int(rng.integers(0, 6))
        if kind == 0:
            return 0
        if kind == 1:
            return 1 << int(rng.integers(0, n_colors))
        if kind == 2:
            return bits
        if kind == 3:
            return 1 << (n_colors - 1)
        if kind == 4:   # bits at or above n_colors among them
            return int(rng.integers(0, 1 << 63)) * 2 + 1
        return int(rng.integers(0, 1 << 63)) & bits
    adds = [(int(universe[int(rng.integers(0, universe.size))]), mask()) for _ in range(n_keys)]
    pool = np.concatenate([universe, rng.integers(0, 1 << 63, 40, dtype=np.uint64)])
    records = []
    for length in [0, 1, 63, 64, 65, 128, 129] + [int(v) for v in rng.integers(0, 200, n_records)]:
        records.append([None if rng.random() < 0.1 else int(pool[int(rng.integers(0, pool.size))]) for _ in range(length)])
    return Case(f"random {seed} C={n_colors}", n_colors, 400, adds, [int(v) for v in pool], records)


def edge_cases():
    cases = [random_case(100 + i, c) for i, c in enumerate((1, 2, 63, 64, 3, 8))]
    # three and more keys aimed at the last slot, so the probe wraps past it
    for capacity in (6, 3000):
        slots = CM.slots_for(capacity)
        keys = [int(v) for v in CM.keys_with_home(slots - 1, slots, 32, 5)]
        assert all(int(CM.home(k, slots)) == slots - 1 for k in keys)
        adds = [(k, 1 << (i % 3)) for i, k in enumerate(keys)] + [(keys[1], 4), (keys[1], 4)]
        cases.append(Case(f"wrap {capacity}", 3, capacity, adds, keys + [7], [keys + [None, 7] + keys[:2]]))
    # all ties, a tie between colours 0 and 5, a single colour, no hit, all-zero rows
    tie = [(10 + c, 1 << c) for c in range(8)]
    cases.append(Case("ties", 8, 64, tie, [], [[10 + c for c in range(8)], [10, 15, 12, 10, 15], [13, 13, 13], [99, 98], [], [None] * 70,
                                               [10, 11, 11, 12, 12, 12], [17, 17, 16, 16, 15]]))
    cases.append(Case("mask 0 and beyond", 2, 64, [(1, 0), (2, 4), (3, 7), (M64, 8), (M64, 2), (0, 1)], [0, 1, 2, 3, M64], [[0, 1, 2, 3, M64]]))
    return cases


def test_edge_cases_match_the_model(program):
    cases = edge_cases()
    for got, c in zip(run(program, cases), cases):
        model = hold(got, c)
        if c.name == "ties":
            assert [r[3:] for r in got["rows"]] == [[0, 1], [0, 5], [3, KM.NONE], [KM.NONE, KM.NONE], [KM.NONE, KM.NONE],
                                                    [KM.NONE, KM.NONE], [2, 1], [6, 7]]
        if c.name == "mask 0 and beyond":
            assert model.n_masked_bits == 3 and got["lookup"] == [1, 0, 0, 3, 2] and got["n_keys"] == 3


def test_a_table_filled_to_its_probe_bound_drops(program):
    """capacity 1 (two slots, bound 2) with five keys; and 4097 keys with one home in 8192 slots (bound 4096): the keys that came first
    are held, every later occurrence is dropped, a repeated held key is merged."""
    few = [(k, 1) for k in (11, 22, 33, 44, 55)] + [(11, 2)]
    slots = CM.slots_for(6000)
    assert slots == 8192
    chain = [int(v) for v in CM.keys_with_home(100, slots, 32, 4097)]
    cases = [Case("two slots", 2, 1, few, [], []), Case("chain", 1, 6000, [(k, 1) for k in chain] + [(chain[0], 1), (chain[-1], 1)], [], [])]
    a, b = run(program, cases)
    hold(a, cases[0], complete=False)
    hold(b, cases[1], complete=False)
    assert (a["n_keys"], a["n_dropped"], a["per_color"]) == (2, 3, [2, 1])
    assert (b["n_keys"], b["n_dropped"], b["per_color"]) == (4096, 2, [4096])


def test_the_same_program_under_the_sanitizers(sanitized):
    cases = edge_cases()[:3] + edge_cases()[6:] + [Case("two slots", 2, 1, [(k, 1) for k in (11, 22, 33, 44, 55)], [11, 66], [[11, 66, None]])]
    got = run(sanitized, cases)
    for g, c in zip(got[:-1], cases[:-1]):
        hold(g, c)
    assert got[-1]["n_dropped"] == 3
