"""The two sides of the __HIP_DEVICE_COMPILE__ splits of csrc/ntk_tile.hpp against each other.  The CPU suite checks the tile logic on a
host emulation (tests/emu/) that runs a C restatement wherever the kernels run a gfx950 builtin or inline assembly; the emulation is only as
good as those restatements.  tests/emu/dev_helpers.hip evaluates each two-faced helper element-wise; it is built here twice into tmp_path -
with hipcc for gfx950 (a small shared library that runs one bounds-checked block of 256 threads per call) and with g++ (the `#else`
branches) - and both must give the same words on the edge words (0, ~0, 0x80000000, 0x7FFFFFFF, 1, alternating bit and byte patterns, every
byte in {00, 7F, 80, FF}) in every argument, and on 4096 random words.

The header has 28 splits.  Seven are pure functions and are compared here on these domains:
  bitop3      every truth table the headers use (collected from the source text; 0xCA, 0xEA, 0xA8, 0xF4 among them);
  perm        every selector constant the headers pass, and every selector whose bytes are 0..7 or 12..15 (the run-time selectors of encode16
              and encode16_sv2 are bytes 0..7).  The host model returns 0 for a byte selector 8..12; the instruction does so for 12 only (8..11
              replicate sign bits), so no constant of the headers may hold a byte 8..11: asserted on the source text.  12 itself is in use
              (0x0C0C0400 in encode16_sv2) and is compared like the rest;
  alignbit    shifts 0..63;
  add_self, brev32, dot4;
  key_min(KeyF)  v_min_f64 against the integer compare on the key domain: bit 62 set and bit 61 clear, every value width of k = 1..25, equal
              high words, tags that differ in the lowest bit only, equal keys.
Through them: quality_break on all 256 x 256 (quality, cutoff) pairs, lower_watch_or, and - as the kernels compose them - encode16,
encode16_sv2 with bad16_from_letters, key_fields(KeyF).

Nothing to compare (no function of arguments; the host side is the same statement without the annotation):
  18 `#pragma unroll` guards - min_shifted (5), min_overlap (3), bad16_from_letters (1), minimizer_invalid16 (2), minimizer_keys_f64 (1),
     minimizer_keys_general (1), min_van_herk (4), minimizer_slide (1): g++ has no such pragma in that position;
  3 register pins / barriers - the empty asm("" : "+v"(x)) of minimizer_keys_f64 and minimizer_keys_general (keep a wave-uniform operand in a
     VGPR) and the asm volatile("" ::: "memory") of wk_strand (keeps a branch): they emit no instruction.
Run with `pytest -m gpu` on an MI355X."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

HERE = os.path.dirname(os.path.abspath(__file__))
SRC = os.path.join(HERE, "emu", "dev_helpers.hip")
CSRC = os.path.join(HERE, "..", "needletail_amd", "csrc")

(BITOP3, PERM, ALIGNBIT, ADD_SELF, BREV32, DOT4, KEY_MIN_F, QUALITY_BREAK, LOWER_WATCH, ENCODE16, ENCODE16_SV2, KEY_FIELDS_F) = range(12)
NARGS = {BITOP3: 3, PERM: 3, ALIGNBIT: 3, ADD_SELF: 1, BREV32: 1, DOT4: 3, KEY_MIN_F: 4, QUALITY_BREAK: 4, LOWER_WATCH: 2, ENCODE16: 4,
         ENCODE16_SV2: 4, KEY_FIELDS_F: 2}

CORE = [0, 0xFFFFFFFF, 0x80000000, 0x7FFFFFFF, 1, 0x55555555, 0xAAAAAAAA, 0x33333333, 0xCCCCCCCC, 0x0F0F0F0F, 0xF0F0F0F0, 0x00FF00FF,
        0xFF00FF00, 0x0000FFFF, 0xFFFF0000]
EDGE = np.array(CORE + [b0 | b1 << 8 | b2 << 16 | b3 << 24 for b3 in (0, 0x7F, 0x80, 0xFF) for b2 in (0, 0x7F, 0x80, 0xFF)
                        for b1 in (0, 0x7F, 0x80, 0xFF) for b0 in (0, 0x7F, 0x80, 0xFF)], dtype=np.uint32)
N_RANDOM = 4096


def _load(path):
    L = C.CDLL(path)
    L.dh_eval.restype = C.c_int
    L.dh_eval.argtypes = [C.c_int, C.c_uint32] + [C.c_void_p] * 7 + [C.c_uint32]
    L.dh_is_device.restype = C.c_int
    return L


@pytest.fixture(scope="module")
def sides(tmp_path_factory):
    d = tmp_path_factory.mktemp("dev_helpers")
    gpu, host = str(d / "libdev_helpers_gfx950.so"), str(d / "libdev_helpers_host.so")
    hipcc = os.path.join(os.environ.get("ROCM_PATH") or "/opt/rocm", "bin", "hipcc")
    subprocess.check_call([hipcc, "--offload-arch=gfx950", "-O2", "-std=c++17", "-fPIC", "-shared", "-o", gpu, SRC])
    subprocess.check_call(["g++", "-x", "c++", "-O2", "-std=c++17", "-fPIC", "-shared", "-Wno-unknown-pragmas", "-o", host, SRC])
    dev, cpu = _load(gpu), _load(host)
    assert dev.dh_is_device() == 1 and cpu.dh_is_device() == 0
    return dev, cpu


def evaluate(L, op, imm, args):
    n = len(args[0])
    assert 0 < n <= 1 << 16 and all(len(a) == n for a in args)
    full = [np.ascontiguousarray(a, dtype=np.uint32) for a in args] + [np.zeros(n, dtype=np.uint32)] * (4 - len(args))
    outs = [np.zeros(n, dtype=np.uint32) for _ in range(3)]
    rc = L.dh_eval(op, imm, *[a.ctypes.data for a in full], *[o.ctypes.data for o in outs], n)
    assert rc == 0, (op, hex(imm), rc)
    return outs


def assert_sides_equal(sides, op, imm, args, what):
    dev, cpu = sides
    got, want = evaluate(dev, op, imm, args), evaluate(cpu, op, imm, args)
    for o, (g, w) in enumerate(zip(got, want)):
        bad = np.flatnonzero(g != w)
        assert bad.size == 0, (what, "output", o, "element", int(bad[0]), [hex(int(a[bad[0]])) for a in args], hex(int(g[bad[0]])), hex(int(w[bad[0]])))


def domain(nargs, seed, fixed=None):
    """Argument arrays: every edge word in every argument position (the other arguments drawn from the edge words), the full cross of the
    named core words (up to three arguments), 4096 random words.  fixed: {position: array generator(n, rng)} overrides an argument."""
    rng = np.random.default_rng(0xD0E5 + seed)
    cols = [[] for _ in range(nargs)]
    for p in range(nargs):
        for q in range(nargs):
            cols[q].append(EDGE if q == p else EDGE[rng.integers(0, len(EDGE), len(EDGE))])
    core = np.array(CORE, dtype=np.uint32)
    if nargs <= 3:
        grid = np.meshgrid(*[core] * nargs, indexing="ij")
        for q in range(nargs):
            cols[q].append(grid[q].reshape(-1))
    for q in range(nargs):
        cols[q].append(rng.integers(0, 1 << 32, N_RANDOM, dtype=np.uint64).astype(np.uint32))
    args = [np.concatenate(c) for c in cols]
    for p, gen in (fixed or {}).items():
        args[p] = gen(len(args[p]), rng).astype(np.uint32)
    return args


def _header_text():
    return "".join(open(os.path.join(CSRC, f)).read() for f in sorted(os.listdir(CSRC)) if f.endswith((".hpp", ".hip")))


def test_bitop3_every_truth_table_of_the_headers(sides):
    tables = sorted({int(t, 16) for t in re.findall(r"bitop3<(0x[0-9A-Fa-f]+)>", _header_text())})
    assert {0xCA, 0xEA, 0xA8, 0xF4} <= set(tables)
    for tt in tables:
        assert_sides_equal(sides, BITOP3, tt, domain(3, tt), ("bitop3", hex(tt)))


def test_perm_every_selector_of_the_headers(sides):
    text = _header_text()
    # every literal selector: an eight-digit constant that closes an argument list on a line with a perm( call, nested calls included.  The
    # selectors that are no literals (`sel` in encode16: bytes & 0x03; `n` in encode16_sv2: bytes & 0x07) are covered by the run-time domain below.
    consts = sorted({int(s, 16) for s in re.findall(r",\s*(0x[0-9A-Fa-f]{8})u\)", "\n".join(l for l in text.splitlines() if "perm(" in l))})
    assert {0x04000501, 0x06020703, 0x07060302, 0x05040100, 0x0C0C0400} <= set(consts), [hex(c) for c in consts]
    for sel in consts:
        sel_bytes = [(sel >> (8 * i)) & 0xFF for i in range(4)]
        assert not any(8 <= b <= 11 for b in sel_bytes), ("the host model of perm is not the instruction for a byte selector 8..11", hex(sel))
        assert all(b <= 7 or b == 12 for b in sel_bytes), hex(sel)
        assert_sides_equal(sides, PERM, 0, domain(3, sel, {2: lambda n, rng: np.full(n, sel)}), ("perm", hex(sel)))
    # run-time selectors (bytes & 0x03 in encode16, & 0x07 in encode16_sv2), and 12..15 (constants 0x00 / 0xFF)
    ok = np.array(list(range(8)) + [12, 13, 14, 15], dtype=np.uint32)

    def any_ok(n, rng):
        b = ok[rng.integers(0, len(ok), (n, 4))]
        return b[:, 0] | b[:, 1] << 8 | b[:, 2] << 16 | b[:, 3] << 24
    assert_sides_equal(sides, PERM, 0, domain(3, 77, {2: any_ok}), "perm, selectors 0..7 and 12..15")


def test_alignbit_shifts_0_to_63(sides):
    for sh in range(64):
        assert_sides_equal(sides, ALIGNBIT, 0, domain(3, sh, {2: lambda n, rng: np.full(n, sh)})[:3], ("alignbit", sh))


def test_add_self_brev32_dot4(sides):
    assert_sides_equal(sides, ADD_SELF, 0, domain(1, 1), "add_self")
    assert_sides_equal(sides, BREV32, 0, domain(1, 2), "brev32")
    assert_sides_equal(sides, DOT4, 0, domain(3, 3), "dot4")


def _keys(k, value, tag):
    """bit 62 | value << 11 | tag as (hi, lo) words; value < 4^k, tag < 2^11"""
    key = (np.uint64(1) << np.uint64(62)) | (value.astype(np.uint64) << np.uint64(11)) | tag.astype(np.uint64)
    return (key >> np.uint64(32)).astype(np.uint32), (key & np.uint64(0xFFFFFFFF)).astype(np.uint32)


def test_key_min_f64_on_the_key_domain(sides):
    rng = np.random.default_rng(0x6E7)
    a, b, c, d = [], [], [], []
    for k in range(1, 26):
        top = (1 << (2 * k)) - 1
        edge_v = np.array(sorted({0, 1, top, top - 1, top >> 1, (top >> 1) + 1, 0x55555555555555 & top, 0xAAAAAAAAAAAAAA & top,
                                  ((1 << 21) - 1) & top, (1 << 21) & top, ((1 << 21) + 1) & top}), dtype=np.uint64)
        v1 = np.concatenate([np.repeat(edge_v, len(edge_v)), rng.integers(0, top + 1, 160, dtype=np.uint64)])
        v2 = np.concatenate([np.tile(edge_v, len(edge_v)), rng.integers(0, top + 1, 160, dtype=np.uint64)])
        t1 = rng.integers(0, 2048, len(v1), dtype=np.uint64)
        t2 = rng.integers(0, 2048, len(v1), dtype=np.uint64)
        # equal values: tags differing in the lowest bit only, and equal keys; equal high words with different low words
        same = rng.integers(0, top + 1, 64, dtype=np.uint64)
        ts = rng.integers(0, 2048, 64, dtype=np.uint64)
        v1 = np.concatenate([v1, same, same, same]); v2 = np.concatenate([v2, same, same, same ^ np.uint64(1)])
        t1 = np.concatenate([t1, ts, ts, ts]); t2 = np.concatenate([t2, ts ^ np.uint64(1), ts, ts])
        for (hi, lo), (x, y) in ((_keys(k, v1, t1), (a, b)), (_keys(k, v2, t2), (c, d))):
            x.append(hi); y.append(lo)
    args = [np.concatenate(x) for x in (a, b, c, d)]
    assert len(args[0]) <= 1 << 16
    hi = args[0]
    assert ((hi >> 30) & 3 == 1).all()   # bit 62 set, bit 63 clear; bit 61 clear: 2k + 11 <= 61
    assert ((args[0] >> 29) & 1 == 0).all() and ((args[2] >> 29) & 1 == 0).all()
    assert_sides_equal(sides, KEY_MIN_F, 0, args, "key_min(KeyF)")
    assert_sides_equal(sides, KEY_FIELDS_F, 0, args[:2], "key_fields(KeyF)")


def test_quality_break_every_quality_and_cutoff(sides):
    """All 256 x 256 (quality, cutoff) pairs: one dword holds four qualities under one cutoff's (add, sel) - quality_cut's, restated; the
    sequence bytes are every byte value in turn."""
    q = np.arange(256, dtype=np.uint32).reshape(64, 4)
    qw = q[:, 0] | q[:, 1] << 8 | q[:, 2] << 16 | q[:, 3] << 24                      # 64 dwords: the 256 qualities
    s, qq, add, sel = [], [], [], []
    for cutoff in range(256):
        a7 = ((128 - cutoff if cutoff <= 128 else 256 - cutoff) & 0x7F) * 0x01010101    # ntk_tile.hpp quality_cut
        sw = np.roll(qw, cutoff) ^ np.uint32(0x20202020 if cutoff & 1 else 0)
        s.append(sw); qq.append(qw); add.append(np.full(64, a7, dtype=np.uint32)); sel.append(np.full(64, 0xFFFFFFFF if cutoff <= 128 else 0, dtype=np.uint32))
    args = [np.concatenate(x).astype(np.uint32) for x in (s, qq, add, sel)]
    assert len(args[0]) == 256 * 64
    assert_sides_equal(sides, QUALITY_BREAK, 0, args, "quality_break, every pair")
    assert_sides_equal(sides, QUALITY_BREAK, 0, domain(4, 5), "quality_break, edge and random words")
    assert_sides_equal(sides, LOWER_WATCH, 0, domain(2, 6), "lower_watch_or")


def test_encoders_as_the_kernels_compose_them(sides):
    """encode16 (perm, bfi, brev32, and_or, or_and) and encode16_sv2 + bad16_from_letters (perm, dot4, brev32, add_self, bitop3 0x35, or_and)
    on lines of letters, near-letters and arbitrary bytes."""
    rng = np.random.default_rng(0xE2C)
    alphabet = np.frombuffer(b"ACGTUacgtuNn\n\x00\x7f\x80\xff@BDEFHSVtT", dtype=np.uint8)
    lines = alphabet[rng.integers(0, len(alphabet), (4096, 16))]
    lines = np.concatenate([lines, rng.integers(0, 256, (4096, 16), dtype=np.uint8),
                            np.repeat(np.arange(256, dtype=np.uint8), 16).reshape(256, 16)])
    words = np.ascontiguousarray(lines).view("<u4")            # [n, 4]: little-endian dwords, byte 0 of x is base 0
    args = [words[:, i].copy() for i in range(4)]
    for accept_u in (0, 1):
        assert_sides_equal(sides, ENCODE16, accept_u, args, ("encode16", accept_u))
        assert_sides_equal(sides, ENCODE16_SV2, accept_u, args, ("encode16_sv2 + bad16_from_letters", accept_u))
    assert_sides_equal(sides, ENCODE16, 1, domain(4, 8), "encode16, edge and random words")
    assert_sides_equal(sides, ENCODE16_SV2, 1, domain(4, 9), "encode16_sv2, edge and random words")


def test_the_header_still_has_the_28_splits_listed_above():
    text = open(os.path.join(CSRC, "ntk_tile.hpp")).read()
    lines = text.splitlines()
    at = [i for i, l in enumerate(lines) if "defined(__HIP_DEVICE_COMPILE__)" in l]
    pragma = sum(lines[i + 1].strip() == "#pragma unroll" for i in at)
    assert (len(at), pragma) == (28, 18), (len(at), pragma)   # a new split: compare it above, or list it in the docstring
