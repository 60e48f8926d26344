"""The build manifest: which template instantiation of the scan kernels every reachable call launches.

A plain-Python restatement of the dispatch rules of csrc/ntk_api.hip (resolve_mode, pick_scan / pick_materialise, pick_scan_min, pick_min_generic,
run_scan's raw-byte / speculation branch, run_bytes_reduce, minimizers_reduce_impl and its two-pass window_min_reduce_kernel<W> switch) and of
the pick tables of csrc/ntk_scan2.hip.  `calls()` enumerates every reachable call; `kernels(call)` names the matrix kernels it launches, in
the demangled form `short_name` gives a symbol of the library (`scan2_kernel<21, true, true, false, 14, 0, false>`).  fold_kernel, which
every reduce call launches as well, is not a matrix kernel (tests/test_build_manifest.py OTHER_KERNELS).

Preconditions of the restatement: inputs of fewer than 2^22 scan tiles (one launch, so the speculative route is open) and n > 0.
test_build_manifest.py holds the manifest to the shipped code object; test_gpu_build_matrix.py runs every entry against the oracle."""
import os
import re
import subprocess
import tempfile
from typing import NamedTuple

PATH_BYTES_CANONICAL, PATH_BITS, PATH_BITS_CANONICAL = 0, 1, 2          # include/needletail_amd.h
PRE_NONE, PRE_STRIP_RETURNS, PRE_NORMALIZE, PRE_NORMALIZE_IUPAC = 0, 1, 2, 3
ROUTE_NO_REGFUSED, ROUTE_NO_GENERIC, ROUTE_NO_F64, ROUTE_NO_SPECULATION = 1, 2, 4, 8
HIST_BITS = 14                                                          # ntk_scan2.hip kScan2HistBits

PATHS_PRES = [(path, pre) for path in (PATH_BYTES_CANONICAL, PATH_BITS, PATH_BITS_CANONICAL)
              for pre in (PRE_NONE, PRE_STRIP_RETURNS, PRE_NORMALIZE, PRE_NORMALIZE_IUPAC)]
WIDE_KS = (33, 40, 64, 127, 255)          # k = 33..255: a run-time argument of the kernels, a handful is enough
MIN_WS = tuple(range(1, 18)) + (31, 49, 50)   # every compile-time window of the two-pass route, the generic kernel's limit and one past
ROUTES_MIN = (0, ROUTE_NO_F64, ROUTE_NO_REGFUSED, ROUTE_NO_REGFUSED | ROUTE_NO_F64, ROUTE_NO_REGFUSED | ROUTE_NO_GENERIC)

MATRIX_FAMILIES = ("scan2_kernel", "minimizer_scan_kernel", "scan_kernel", "canonical_bytes_reduce_kernel",
                   "wide_canonical_reduce_kernel", "window_min_reduce_kernel")


class Mode(NamedTuple):
    kw: int
    canon: bool
    tie_rc: bool
    accept_u: bool
    raw_bytes: bool


class Call(NamedTuple):
    entry: str        # "reduce" (ntk_reduce_device[_quality], the batch face), "minimizers" (the same with w > 0), "materialize"
    k: int
    w: int
    path: int
    pre: int
    quality: bool     # a quality stream with a cutoff of 1..255
    route: int        # NTK_OPT_MINIMIZER_ROUTE bits


def b(x: bool) -> str:
    return "true" if x else "false"


def resolve_mode(k: int, path: int, pre: int):
    """None where the call is an error (NTK_ERR_BAD_K)."""
    if k < 1 or k > (255 if path == PATH_BYTES_CANONICAL else 32):
        return None
    accept_u = pre >= PRE_NORMALIZE
    if path == PATH_BYTES_CANONICAL:
        return Mode(2 if k > 16 else 1, True, True, accept_u, pre < PRE_NORMALIZE or k > 32)
    return Mode(2 if k > 16 else 1, path == PATH_BITS_CANONICAL, False, accept_u, False)


def scan2(k, tie_rc, accept_u, qm=False, w=0, fwd=False) -> str:
    return f"scan2_kernel<{k}, {b(tie_rc)}, {b(accept_u)}, {b(qm)}, {HIST_BITS}, {w}, {b(fwd)}>"


_QT = ", unsigned char const*, unsigned int, unsigned int"   # the quality builds' trailing parameter pack (ntk_kernels.hpp QualIn)


def bytes_reduce(wide: bool, q: bool) -> str:
    return f"canonical_bytes_reduce_kernel<{b(wide)}, {b(q)}{_QT if q else ''}>"


def wide_reduce(accept_u: bool, q: bool) -> str:
    return f"wide_canonical_reduce_kernel<{b(accept_u)}, {b(q)}{_QT if q else ''}>"


def pick_scan_reduce(m: Mode, k: int, q: bool) -> str:
    if m.canon:
        return scan2(k, m.tie_rc, m.accept_u, q)
    return scan2(k, False, m.accept_u, q, fwd=True)


def pick_scan_materialize(m: Mode, k: int, q: bool) -> str:
    if not q and m.kw == 2 and m.canon and k == 21:
        return f"scan_kernel<2, true, {b(m.tie_rc)}, {b(m.accept_u)}, false, 21, false>"
    return f"scan_kernel<{m.kw}, {b(m.canon)}, {b(m.tie_rc)}, {b(m.accept_u)}, false, 0, {b(q)}>"


FUSED_MIN_KS, FUSED_MIN_WS, FUSED_MIN_Q = range(15, 24), (5, 9, 10, 11, 12), ((15, 10), (21, 11))


def pick_scan_min(m: Mode, k: int, w: int, q: bool):
    if not m.canon or m.raw_bytes:
        return None
    if (not q and k in FUSED_MIN_KS and w in FUSED_MIN_WS) or (q and (k, w) in FUSED_MIN_Q):
        return scan2(k, m.tie_rc, m.accept_u, q, w=w)
    return None


def min_gen_mode(k: int, f64: bool) -> int:
    return 2 if k >= 24 else (3 if f64 and k >= 19 else (1 if k >= 8 else 0))


def pick_min_generic(m: Mode, q: bool, f64: bool, k: int) -> str:
    kw = 2 if f64 else m.kw
    return f"minimizer_scan_kernel<{kw}, {b(m.tie_rc)}, {b(m.accept_u)}, {b(q)}, {b(f64)}, {min_gen_mode(k, f64)}>"


def kernels(c: Call):
    """The matrix kernels the call launches, in launch order; None if the call is an error."""
    m = resolve_mode(c.k, c.path, c.pre)
    if m is None:
        return None
    if c.entry == "reduce":
        if m.raw_bytes:
            if c.k > 32:   # run_bytes_reduce, the packed-stream kernel first
                if c.route & ROUTE_NO_SPECULATION:
                    return (bytes_reduce(True, c.quality),)
                return (wide_reduce(m.accept_u, c.quality), bytes_reduce(True, c.quality))
            if c.route & ROUTE_NO_SPECULATION:   # run_bytes_reduce, the byte walk alone
                return (bytes_reduce(False, c.quality),)
            return (scan2(c.k, True, False, c.quality), bytes_reduce(False, c.quality))   # the speculative build, the raw kernel behind it
        return (pick_scan_reduce(m, c.k, c.quality),)
    if c.entry == "materialize":
        return None if m.raw_bytes else (pick_scan_materialize(m, c.k, c.quality),)
    assert c.entry == "minimizers"
    if not m.canon or m.raw_bytes or not 1 <= c.w <= 256:
        return None
    fn = None if c.route & ROUTE_NO_REGFUSED else pick_scan_min(m, c.k, c.w, c.quality)
    if fn:
        return (fn,)
    if c.k <= 31 and c.w <= 49 and not c.route & ROUTE_NO_GENERIC:
        return (pick_min_generic(m, c.quality, c.k <= 25 and not c.route & ROUTE_NO_F64, c.k),)
    return (pick_scan_materialize(m, c.k, c.quality), f"window_min_reduce_kernel<{c.w if 2 <= c.w <= 16 else 0}>")


def calls():
    """Every reachable call (errors left out), each once."""
    out = []
    for path, pre in PATHS_PRES:
        for q in (False, True):
            for k in list(range(1, 33)) + (list(WIDE_KS) if path == PATH_BYTES_CANONICAL else []):
                m = resolve_mode(k, path, pre)
                for route in ((0, ROUTE_NO_SPECULATION) if m.raw_bytes else (0,)):
                    out.append(Call("reduce", k, 0, path, pre, q, route))
                if not m.raw_bytes:
                    out.append(Call("materialize", k, 0, path, pre, q, 0))
                if m.canon and not m.raw_bytes:
                    for w in MIN_WS:
                        for route in ROUTES_MIN:
                            out.append(Call("minimizers", k, w, path, pre, q, route))
    return [c for c in out if kernels(c) is not None]


def manifest():
    """{symbol: [calls that launch it]}."""
    out = {}
    for c in calls():
        for s in kernels(c):
            out.setdefault(s, []).append(c)
    return out


def family(sym: str) -> str:
    return sym.split("<", 1)[0].split("(", 1)[0]


# ---- the kernels of the shipped code object ---------------------------------------------------------------------------

def short_name(demangled: str) -> str:
    """`void ntk::scan2_kernel<5, ...>(ntk::ScanArgs) (.kd)` -> `scan2_kernel<5, ...>` (the name rocprofv3 reports maps the same way)."""
    s = demangled.strip()
    if s.endswith("(.kd)"):
        s = s[: -len("(.kd)")].rstrip()
    if s.startswith("void "):
        s = s[len("void "):]
    mt = re.match(r"^(.*?)\([^()]*\)$", s)
    if mt:
        s = mt.group(1)
    return s[len("ntk::"):] if s.startswith("ntk::") else s


def llvm_bin(tool: str) -> str:
    for d in (os.environ.get("ROCM_PATH", ""), "/opt/rocm"):
        p = os.path.join(d, "llvm", "bin", tool)
        if d and os.path.exists(p):
            return p
    return tool


_KERNELS = {}   # (path, mtime, size, arch) -> library_kernels: a run unbundles each file once


def library_kernels(so_path: str, arch: str = "gfx950") -> set:
    """The short names of every kernel (its `.kd` symbol) in the library's code objects for `arch`."""
    st = os.stat(so_path)
    key = (os.path.abspath(so_path), st.st_mtime_ns, st.st_size, arch)
    if key not in _KERNELS:
        _KERNELS[key] = frozenset(_unbundled_kernels(so_path, arch))
    return set(_KERNELS[key])


def _unbundled_kernels(so_path: str, arch: str) -> set:
    with tempfile.TemporaryDirectory() as td:
        fb = os.path.join(td, "fatbin")
        subprocess.check_call([llvm_bin("llvm-objcopy"), f"--dump-section=.hip_fatbin={fb}", so_path, os.path.join(td, "stripped")])
        blob = open(fb, "rb").read()
        starts = [mt.start() for mt in re.finditer(re.escape(b"__CLANG_OFFLOAD_BUNDLE__"), blob)] + [len(blob)]
        names = set()
        for i in range(len(starts) - 1):   # one bundle per object file
            part, co = os.path.join(td, f"b{i}"), os.path.join(td, f"b{i}.co")
            with open(part, "wb") as f:
                f.write(blob[starts[i]: starts[i + 1]])
            subprocess.check_call([llvm_bin("clang-offload-bundler"), "--unbundle", "--type=o",
                                   f"--targets=hipv4-amdgcn-amd-amdhsa--{arch}", f"--input={part}", f"--output={co}"])
            out = subprocess.check_output([llvm_bin("llvm-readelf"), "-s", "-W", "--demangle", co]).decode()
            for line in out.splitlines():
                if line.rstrip().endswith("(.kd)"):
                    names.add(short_name(line.split(None, 7)[7]))
        return names
