"""Which builds of the dispatch matrix (tests/_builds.py) a profiled run never launched.

    rocprofv3 --kernel-trace --stats -d OUT -- python -m pytest tests/test_gpu_build_matrix.py -m gpu
    python tools/kernel_coverage.py OUT            # the kernel_stats.csv under OUT (or the file itself)

Prints one JSON object: the manifest size, how many of its builds were launched, and the list of those that were not (expected: empty).
Exit status 1 if that list is not empty."""
import csv
import glob
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))
import _builds as B  # noqa: E402


def launched(path: str) -> set:
    files = [path] if os.path.isfile(path) else sorted(glob.glob(os.path.join(path, "**", "*kernel_stats.csv"), recursive=True))
    if not files:
        raise SystemExit(f"no kernel_stats.csv under {path}")
    names = set()
    for f in files:
        with open(f, newline="") as fh:
            for row in csv.DictReader(fh):
                names.add(B.short_name(row.get("Name") or row.get("KernelName") or ""))
    return names


def main() -> int:
    if len(sys.argv) != 2:
        print(__doc__)
        return 2
    seen = launched(sys.argv[1])
    manifest = B.manifest()
    missing = sorted(s for s in manifest if s not in seen)
    print(json.dumps({"manifest": len(manifest), "launched": len(manifest) - len(missing), "never_launched": missing}, indent=1))
    return 1 if missing else 0


if __name__ == "__main__":
    sys.exit(main())
