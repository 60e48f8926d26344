"""Keeps the mutant list of tests/_tile_mutants.py in step with the sources it edits.  The whole-list audit is a tool
(tools/mutation_audit.py, profiles/mutation_audit/README.md has its verdicts); here, on the CPU:

- every anchor occurs exactly once in today's sources, ids are unique, every replacement differs from its anchor, every covering test file
  exists, and the groups keep their minimum spread - an edit to a header that orphans a mutant fails here, not silently in the next audit;
- at most 15 % of the list is marked equivalent (the cap keeps the audit from waving away its own findings), and each such mark carries
  its argument;
- three pinned mutants with a recorded fast kill, built (g++ only, in temporary copies outside the tree) and run in parallel, still die in
  their recorded test."""
import importlib.util
import os
import sys
from concurrent.futures import ThreadPoolExecutor

import pytest

import _tile_mutants as TM

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "needletail_amd", "csrc")


def _audit_tool():
    spec = importlib.util.spec_from_file_location("mutation_audit", os.path.join(ROOT, "tools", "mutation_audit.py"))
    mod = importlib.util.module_from_spec(spec)
    sys.modules.setdefault("mutation_audit", mod)
    spec.loader.exec_module(mod)
    return mod


def test_every_mutant_still_applies():
    assert len(TM.MUTANTS) >= 60
    ids = [m.id for m in TM.MUTANTS]
    assert len(set(ids)) == len(ids)
    sources = {}
    for m in TM.MUTANTS:
        src = sources.setdefault(m.file, open(os.path.join(CSRC, m.file)).read())
        assert src.count(m.anchor) == 1, (m.id, "anchor occurs", src.count(m.anchor), "times in", m.file)
        assert m.replacement != m.anchor and m.anchor and m.note and m.function, m.id
        assert m.tests, m.id
        for t in m.tests:
            assert os.path.exists(os.path.join(ROOT, t)), (m.id, t)
        # only code the host compiles: the edit does not sit in a device-only branch
        at = src.index(m.anchor)
        before = src[:at]
        last_if, last_else, last_end = (before.rfind(x) for x in ("#if defined(__HIP_DEVICE_COMPILE__)", "#else", "#endif"))
        assert not (last_if > last_end and last_if > last_else), (m.id, "inside a __HIP_DEVICE_COMPILE__ branch")
    for group, least in TM.GROUPS.items():
        assert sum(m.group == group for m in TM.MUTANTS) >= least, group
    assert {m.group for m in TM.MUTANTS} == set(TM.GROUPS)
    for mid, _ in TM.PINNED:
        assert mid in TM.BY_ID and not TM.BY_ID[mid].equivalent


def test_equivalent_share_is_capped():
    eq = [m for m in TM.MUTANTS if m.equivalent]
    assert 100 * len(eq) <= 15 * len(TM.MUTANTS), (len(eq), len(TM.MUTANTS))
    for m in eq:
        assert m.note.startswith("EQUIVALENT.") and len(m.note) > 120, (m.id, "an equivalence mark carries its argument")


def test_pinned_mutants_still_die_in_their_recorded_test():
    tool = _audit_tool()
    assert os.path.exists(os.path.join(ROOT, "needletail_amd", "libneedletail_amd.so")), "build the tree first"

    def one(pin):
        mid, killer = pin
        return tool.audit_one(TM.BY_ID[mid], TM, only_tests=[killer.split("[")[0]])

    with ThreadPoolExecutor(len(TM.PINNED)) as ex:
        records = list(ex.map(one, TM.PINNED))
    for (mid, killer), rec in zip(TM.PINNED, records):
        assert rec["verdict"] == "killed", rec
        assert rec["killer"].split("[")[0].startswith(killer.split("[")[0]), rec
