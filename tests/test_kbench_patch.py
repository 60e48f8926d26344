"""The measuring switches of tools/kbench.hip (seven ablations, the per-wave clock census) live in tools/kbench_ablations.patch, which
tools/build_kbench.sh applies to a COPY of the kernel headers; the product source holds none of them.  Checked here without a GPU: the
product and its host emulation name no switch, the patch still fits the headers exactly, and the floor variant - the one that once stopped
compiling with nobody noticing - passes the device compiler's front end."""
import os
import re
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "needletail_amd", "csrc")
TOOLS = os.path.join(ROOT, "tools")
SWITCH = re.compile(r"NTK_X_|NTK_ABL_|NTK_V_CLOCKS|NTK_KBENCH")
HEADERS = ("ntk_kernels.hpp", "ntk_tile.hpp", "ntk_plan.hpp")   # what kbench.hip includes (build_kbench.sh copies the same three)


def test_product_and_emulation_sources_name_no_switch():
    for d in (CSRC, os.path.join(ROOT, "tests", "emu")):
        for f in sorted(os.listdir(d)):
            path = os.path.join(d, f)
            if os.path.isfile(path):
                hits = SWITCH.findall(open(path, errors="replace").read())
                assert not hits, f"{os.path.relpath(path, ROOT)} names {sorted(set(hits))}"


@pytest.fixture(scope="module")
def patched(tmp_path_factory):
    """(directory, output of patch) of the headers copied and patched the way build_kbench.sh does it."""
    top = tmp_path_factory.mktemp("kbench_src")
    inc = top / "needletail_amd" / "csrc"
    inc.mkdir(parents=True)
    for h in HEADERS:
        shutil.copy(os.path.join(CSRC, h), inc / h)
    p = subprocess.run(["patch", "-p1", "--fuzz=0", "-d", str(top), "-i", os.path.join(TOOLS, "kbench_ablations.patch")],
                       stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
    return inc, p


def test_kbench_takes_the_kernel_headers_from_the_include_path():
    src = open(os.path.join(TOOLS, "kbench.hip")).read()
    assert "../needletail_amd" not in src and '#include "ntk_kernels.hpp"' in src   # i.e. from the patched copy, wherever the build puts it


def test_the_patch_applies_exactly(patched):
    inc, p = patched
    assert p.returncode == 0, p.stdout
    assert not re.search(r"fuzz|FAILED|reject", p.stdout), p.stdout
    assert sorted(os.listdir(inc)) == sorted(HEADERS)   # no .rej, no .orig
    for h in HEADERS[1:]:
        assert open(inc / h).read() == open(os.path.join(CSRC, h)).read()   # the patch is against ntk_kernels.hpp alone
    # every switch build_kbench.sh passes exists in the patched header (a -D nothing reads would build the shipped kernel under an ablation's name)
    text = open(inc / HEADERS[0]).read()
    passed = set(re.findall(r"-D(NTK_ABL_\w+|NTK_V_CLOCKS)", open(os.path.join(TOOLS, "build_kbench.sh")).read()))
    assert len(passed) == 8
    for name in passed:
        assert re.search(r"#\s*(ifdef|if defined|elif defined)\W+" + name + r"\b", text), name


def test_the_floor_variant_compiles_for_the_device(patched):
    hipcc = shutil.which("hipcc") or os.path.join(os.environ.get("ROCM_PATH", "/opt/rocm"), "bin", "hipcc")
    if not os.path.exists(hipcc):
        pytest.skip("no hipcc on this machine")
    inc, p = patched
    assert p.returncode == 0, p.stdout
    # build_kbench.sh's kb_a_floor line, front end only, device side only (kbench serves k = 21 and k = 31 canonical there)
    c = subprocess.run([hipcc, "--offload-arch=gfx950", "-std=c++17", "--cuda-device-only", "-fsyntax-only", f"-I{inc}", "-DNTK_KB_FIX", "-DNTK_KB_SV",
                        "-DNTK_KB_SV2", "-DNTK_KB_HB=14", "-DNTK_ABL_FLOOR", os.path.join(TOOLS, "kbench.hip")],
                       stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
    assert c.returncode == 0, c.stdout[-4000:]
