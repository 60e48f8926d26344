#!/usr/bin/env python3
"""Mutation audit of the tile logic: which small wrong edits to the headers does the CPU suite notice?

A CPU PROGRAM.  A mutant is never compiled with hipcc and never runs on a device: a deliberately wrong kernel has no place on a shared
GPU machine, so this tool is never started through a GPU runner, and nothing it builds is.  It compiles the host side only (g++: the
lock-step emulator of tests/emu/, the oracle, the shims of the host-arithmetic tests) and runs CPU tests (-m "not gpu").  The repository tree is
never edited: every mutant lives in a fresh temporary copy outside it, which is removed afterwards.

For each mutant of tests/_tile_mutants.py:
  0. once, ahead of the mutants: the same test files run on an UNMUTATED copy; a test that fails there (it needs something outside the copy)
     is deselected for every mutant and reported, so that no kill is credited to a test that fails anyway;
  1. tests/, needletail_amd/, oracle/, include/ and examples/ are copied to a temporary directory (with the product library as it is built in the tree -
     unmutated - so that tests/conftest.py finds it and starts no build of its own; the emulator libraries are left out and rebuilt);
  2. the edit is applied to the copy (the anchor must occur exactly once);
  3. the emulator (or, for a host header, a syntax check of it) and the oracle are built with g++ - a failure is the verdict `no_build`;
  4. the test files that cover the mutated function run first, then the rest of the emulator test files (only for the headers an emulator
     includes), with -m "not gpu" -x: the first failing test is the killer.
One JSON record per mutant: {"id", "verdict": killed | survived | no_build, "killer", "phase": covering | rest, "seconds", ...}.  A build or a
test run that exceeds its time limit is no evidence that a test noticed the edit: it is recorded as `timeout`, a verdict of its own that
counts neither as a kill nor as a survivor, and the audit then exits 1.

    python tools/mutation_audit.py --out audit.jsonl              # the whole list, min(16, cpus) workers
    python tools/mutation_audit.py --only keyg_min_le,plan_first_tail
"""
import argparse
import concurrent.futures
import importlib.util
import json
import os
import re
import shutil
import subprocess
import sys
import tempfile
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
COPIED = ("tests", "needletail_amd", "oracle", "include", "examples")   # (examples/: source text some CPU tests read)
MAX_WORKERS = 16
GXX_EMU = ["g++", "-O2", "-std=c++17", "-fPIC", "-shared", "-Wno-unknown-pragmas"]   # the flags of __graft_entry__.build() and of the fixtures


def load_mutants(root=ROOT):
    spec = importlib.util.spec_from_file_location("_tile_mutants", os.path.join(root, "tests", "_tile_mutants.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def _ignore(_dir, names):
    drop = {"__pycache__", ".pytest_cache", ".hypothesis", "_native", "_ref"}
    return [n for n in names if n in drop or n.endswith((".o", ".pyc")) or (n.startswith("libntk_emu") and n.endswith(".so"))]


def copy_tree(dst, root=ROOT):
    """What the CPU tests need, into dst (a fresh directory outside the repository)."""
    assert not os.path.abspath(dst).startswith(ROOT + os.sep), "mutants live outside the repository"
    if not os.path.exists(os.path.join(root, "needletail_amd", "libneedletail_amd.so")):
        raise SystemExit("build the tree first (python -c 'import __graft_entry__ as g; g.build()'): the copy carries the built, unmutated "
                         "product library so that no test session compiles one from a mutated header")
    for d in COPIED:
        shutil.copytree(os.path.join(root, d), os.path.join(dst, d), ignore=_ignore, symlinks=True)


def apply_edit(dst, m):
    path = os.path.join(dst, "needletail_amd", "csrc", m.file)
    with open(path) as f:
        src = f.read()
    if src.count(m.anchor) != 1:
        raise ValueError(f"{m.id}: anchor occurs {src.count(m.anchor)} times in {m.file}")
    with open(path, "w") as f:
        f.write(src.replace(m.anchor, m.replacement))


def _run(cmd, cwd, timeout):
    env = dict(os.environ, PYTHONDONTWRITEBYTECODE="1")
    p = subprocess.run(cmd, cwd=cwd, env=env, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True, timeout=timeout)
    return p.returncode, p.stdout


def build(dst, m, emu_headers):
    """g++ only.  Returns None, or the compiler's last lines."""
    csrc = os.path.join(dst, "needletail_amd", "csrc")
    emu = os.path.join(dst, "tests", "emu")
    if m.file == "ntk_tile.hpp":
        rc, out = _run(GXX_EMU + ["-o", os.path.join(emu, "libntk_emu.so"), os.path.join(emu, "emu_scan.cpp")], dst, 900)
    elif m.file in emu_headers:   # ntk_plan.hpp: only emu_exact.cpp includes it (the command of test_exact_stride_emu.py's fixture)
        rc, out = _run(["g++", "-O1", "-std=c++17", "-fPIC", "-shared", "-Wno-unknown-pragmas", "-o", os.path.join(emu, "libntk_emu_exact.so"),
                        os.path.join(emu, "emu_exact.cpp")], dst, 900)
    else:                         # the CPU tests compile these behind shims of their own: here only "does it still compile"
        rc, out = _run(["g++", "-std=c++17", "-fsyntax-only", "-x", "c++", os.path.join(csrc, m.file)], dst, 300)
    if rc != 0:
        return out[-2000:]
    rc, out = _run(["make", "-s", "-C", os.path.join(dst, "oracle")], dst, 600)
    return None if rc == 0 else out[-2000:]


_FAILED = re.compile(r"^(?:FAILED|ERROR) (\S+)", re.M)
_CRASHED = re.compile(r'File "[^"]*/tests/(test_\w+\.py)", line \d+ in (test_\w+)')


def pytest_files(dst, files, timeout=3600, deselect=()):
    """(passed, first failing test id or None, the end of the output)"""
    files = [f for f in files if os.path.exists(os.path.join(dst, f.split("::")[0]))]
    if not files:
        return True, None, ""
    skip = [x for t in deselect for x in ("--deselect", t)]
    rc, out = _run([sys.executable, "-m", "pytest", "-q", "-x", "-m", "not gpu", "-rfE", "-p", "no:cacheprovider", *skip, *files], dst, timeout)
    if rc == 0:
        return True, None, out[-400:]
    hit = _FAILED.search(out)
    if hit:
        return False, hit.group(1), out[-3000:]
    # no summary line: the emulator took the interpreter down (an index out of range in wrong tile logic); the fault handler names the test
    hit = _CRASHED.search(out)
    return False, (f"crash in tests/{hit.group(1)}::{hit.group(2)}" if hit else "?"), out[-3000:]


def baseline(mod, mutants):
    """The test files of `mutants` on an unmutated copy, all of them to the end: the ids that fail there."""
    files = sorted({t for m in mutants for t in m.tests} | (set(mod.EMU_TEST_FILES) if any(m.file in mod.EMU_HEADERS for m in mutants) else set()))
    dst = tempfile.mkdtemp(prefix="ntk_mutant_base_")
    try:
        copy_tree(dst)
        files = [f for f in files if os.path.exists(os.path.join(dst, f))]
        rc, out = _run([sys.executable, "-m", "pytest", "-q", "-m", "not gpu", "-rfE", "-p", "no:cacheprovider", *files], dst, 3600)
        return sorted(set(_FAILED.findall(out))) if rc != 0 else []
    finally:
        shutil.rmtree(dst, ignore_errors=True)


def audit_one(m, mod, keep=False, only_tests=None, deselect=()):
    """One mutant, start to finish.  only_tests: run these instead of covering + rest (tests/test_tile_mutants.py's pinned kills)."""
    t0 = time.time()
    dst = tempfile.mkdtemp(prefix="ntk_mutant_")
    rec = {"id": m.id, "file": m.file, "function": m.function, "group": m.group, "equivalent": m.equivalent}
    try:
        copy_tree(dst)
        apply_edit(dst, m)
        err = build(dst, m, mod.EMU_HEADERS)
        if err is not None:
            rec.update(verdict="no_build", killer=None, phase="build", detail=err[-600:])
            return rec
        covering = list(only_tests) if only_tests is not None else list(m.tests)
        ok, killer, tail = pytest_files(dst, covering, deselect=deselect)
        phase = "covering"
        if ok and only_tests is None and m.file in mod.EMU_HEADERS:
            rest = [f for f in mod.EMU_TEST_FILES if f not in covering]
            ok, killer, tail = pytest_files(dst, rest, deselect=deselect)
            phase = "rest"
        if ok:
            rec.update(verdict="survived", killer=None, phase=phase)
        else:
            rec.update(verdict="killed", killer=killer, phase=phase, detail=tail[-600:] if killer == "?" else None)
        return rec
    except subprocess.TimeoutExpired as e:
        rec.update(verdict="timeout", killer=None, phase="timeout", detail=" ".join(map(str, e.cmd))[-200:])
        return rec
    finally:
        rec["seconds"] = round(time.time() - t0, 1)
        if not keep:
            shutil.rmtree(dst, ignore_errors=True)


def audit(mutants, mod, workers, keep=False, on_record=None, deselect=()):
    workers = max(1, min(MAX_WORKERS, workers, len(mutants) or 1))
    records = []
    with concurrent.futures.ThreadPoolExecutor(workers) as ex:   # (threads that wait for g++ and pytest child processes)
        for rec in ex.map(lambda m: audit_one(m, mod, keep, deselect=deselect), mutants):
            records.append(rec)
            if on_record:
                on_record(rec)
    return records


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n\n")[0])
    ap.add_argument("--only", help="comma-separated mutant ids (default: the whole list)")
    ap.add_argument("--workers", type=int, default=min(MAX_WORKERS, os.cpu_count() or 1), help="at most 16")
    ap.add_argument("--out", default="-", help="JSON lines, one record per mutant (default: stdout)")
    ap.add_argument("--keep", action="store_true", help="leave the temporary copies in place")
    a = ap.parse_args()
    mod = load_mutants()
    mutants = list(mod.MUTANTS)
    if a.only:
        mutants = [mod.BY_ID[i] for i in a.only.split(",")]
    out = sys.stdout if a.out == "-" else open(a.out, "w")
    t0 = time.time()

    def emit(rec):
        out.write(json.dumps(rec) + "\n")
        out.flush()
        print(f"{rec['id']:34s} {rec['verdict']:9s} {rec['seconds']:7.1f} s  {rec.get('killer') or ''}", file=sys.stderr)

    broken = baseline(mod, mutants)
    if broken:
        out.write(json.dumps({"baseline_failures": broken}) + "\n")
        print("fail on the unmutated copy, deselected:", *broken, file=sys.stderr)
    records = audit(mutants, mod, a.workers, a.keep, emit, deselect=broken)
    n = {v: sum(r["verdict"] == v for r in records) for v in ("killed", "survived", "no_build", "timeout")}
    summary = {"summary": True, "mutants": len(records), **n, "baseline_failures": len(broken), "workers": min(MAX_WORKERS, a.workers), "wall_seconds": round(time.time() - t0, 1)}
    out.write(json.dumps(summary) + "\n")
    out.flush()
    print(json.dumps(summary), file=sys.stderr)
    # survivors that are not marked equivalent are the audit's findings
    open_ = [r["id"] for r in records if r["verdict"] == "survived" and not r["equivalent"]]
    return 1 if open_ or n["no_build"] or n["timeout"] else 0


if __name__ == "__main__":
    sys.exit(main())
