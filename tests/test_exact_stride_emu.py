"""CPU checks of the exact tile stride of the k-mer builds of scan2_kernel (ntk_tile.hpp Sv2Geom<K, true>): the host planner
(csrc/ntk_plan.hpp) and the tile seams, on the lock-step wave emulation (tests/emu/emu_exact.cpp: the same per-lane source as the kernel, the
kernel's tile geometry, the planner's tiles) against the oracle.  A window emitted by two tiles or by none shows here; the same inputs run
on the device in test_gpu_exact_stride.py."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import oracle as O

from _seams import seam_inputs, stride_of

HERE = os.path.dirname(os.path.abspath(__file__))
EMU_DIR = os.path.join(HERE, "emu")
CSRC = os.path.join(HERE, "..", "needletail_amd", "csrc")

SEAM_KS = (1, 8, 16, 17, 18, 19, 20, 21, 22, 23, 24, 31, 32)
CUTOFF = 53

_EMU = None


def exact_emu():
    global _EMU
    if _EMU is None:
        so = os.path.join(EMU_DIR, "libntk_emu_exact.so")
        srcs = [os.path.join(EMU_DIR, "emu_exact.cpp"), os.path.join(EMU_DIR, "emu_scan.cpp"), os.path.join(CSRC, "ntk_tile.hpp"),
                os.path.join(CSRC, "ntk_plan.hpp")]
        if not os.path.exists(so) or os.path.getmtime(so) < max(os.path.getmtime(s) for s in srcs):
            subprocess.check_call(["g++", "-O1", "-std=c++17", "-fPIC", "-shared", "-Wno-unknown-pragmas", "-o", so, srcs[0]])
        L = C.CDLL(so)
        L.emu_exact_stride.restype = C.c_uint32
        L.emu_exact_stride.argtypes = [C.c_uint32]
        L.emu_scan_exact.restype = C.c_int
        L.emu_scan_exact.argtypes = [C.c_void_p, C.c_void_p, C.c_uint32, C.c_uint64, C.c_uint64, C.c_uint32, C.c_int, C.c_int, C.c_int, C.c_void_p]
        L.emu_plan_launch.restype = None
        L.emu_plan_launch.argtypes = [C.c_uint64] * 6 + [C.c_void_p]
        L.emu_exact_emits.restype = C.c_int
        L.emu_exact_emits.argtypes = [C.c_uint32, C.c_void_p]
        _EMU = L
    return _EMU


@pytest.fixture(scope="module")
def emu():
    return exact_emu()


def scan_exact(L, buf: bytes, k, canon, tie_rc, accept_u, qual: bytes = None):
    n = len(buf)
    npad = (n + 15) // 16 * 16
    arr = np.frombuffer(buf + b"\xAA" * (npad - n), dtype=np.uint8).copy()   # garbage in the 16-byte padding
    q = np.frombuffer(qual + b"\x7e" * (npad - n), dtype=np.uint8).copy() if qual is not None else None
    out = np.zeros(4 + 4096, dtype=np.uint64)
    rc = L.emu_scan_exact(arr.ctypes.data, q.ctypes.data if q is not None else None, CUTOFF, n, npad, k, int(canon), int(tie_rc), int(accept_u),
                          out.ctypes.data)
    assert rc == 0
    return {"n_total": int(out[0]), "n_fwd": int(out[1]), "n_rc": int(out[0] - out[1]), "sum": int(out[2]), "xor": int(out[3]),
            "hist": out[4:].copy()}


def assert_stats_equal(a, b, ctx=""):
    for key in ("n_total", "n_fwd", "n_rc", "sum", "xor"):
        assert a[key] == b[key], (ctx, key, a[key], b[key])
    assert np.array_equal(a["hist"], b["hist"]), ctx


# ---- geometry and planner ------------------------------------------------------------------------------------------

@pytest.mark.parametrize("k", list(range(1, 33)))
def test_stride_and_tile_local_emits(emu, k):
    """Geometry is a pure function of k, the one the issue states; and on a tile of 1024 good bases the tile-local masks emit exactly the
    windows ending in the tile's last `stride` bytes - so tile t, which loads from t stride - (1024 - stride), emits the ends
    [t stride, (t + 1) stride): every end once."""
    s = int(emu.emu_exact_stride(k))
    assert s == stride_of(k) and s % 4 == 0 and 1024 - s >= k - 1
    emits = np.zeros(1024, dtype=np.uint8)
    assert emu.emu_exact_emits(k, emits.ctypes.data) == 0
    want = np.zeros(1024, dtype=np.uint8)
    want[1024 - s:] = 1
    assert np.array_equal(emits, want), (k, np.flatnonzero(emits != want)[:8])


def _plan(L, n, stride, tb, blocks_max=512, wpb=12, max_chunk=24):
    out = np.zeros(10, dtype=np.uint64)
    L.emu_plan_launch(n, stride, tb, blocks_max, wpb, max_chunk, out.ctypes.data)
    keys = ("n_tiles", "tile_begin", "tile_end", "chunk", "blocks", "n_shards", "tiles_per_shard", "tail_rel", "max_tiles", "max_shards")
    return dict(zip(keys, (int(x) for x in out)))


@pytest.mark.parametrize("k", [1, 16, 17, 21, 22, 23, 24, 31, 32])
@pytest.mark.parametrize("grid", [(512, 12, 24), (7, 12, 24), (1, 4, 1)])
def test_planner_covers_every_end_once(emu, k, grid):
    s = stride_of(k)
    sizes = sorted({0, 1, k - 1, k, s - 1, s, s + 1, 2 * s - 1, 2 * s + 1, 1024, (1 << 25) * s + 1})
    for n in sizes:
        first = _plan(emu, n, s, 0, *grid)
        n_tiles, per_launch = first["n_tiles"], first["max_tiles"]
        # tiles of `stride` window ends cover [0, n) and no tile lies wholly beyond it
        assert n_tiles * s >= n and (n_tiles == 0 or (n_tiles - 1) * s < n), (n, n_tiles)
        if n == (1 << 25) * s + 1:
            assert n_tiles == (1 << 25) + 1 and per_launch == 1 << 25   # a second launch of one tile
        covered = 0
        if n == 0:
            assert n_tiles == 0 and first["blocks"] == 0   # nothing to launch
        for tb in range(0, n_tiles, per_launch):
            p = _plan(emu, n, s, tb, *grid)
            assert p["tile_begin"] == tb == covered and tb < p["tile_end"] <= min(tb + per_launch, n_tiles)
            tiles = p["tile_end"] - tb
            covered = p["tile_end"]
            # the shards split the launch's tiles: shard i owns [i tps, (i + 1) tps) clipped, together all of them
            assert 1 <= p["n_shards"] <= min(p["blocks"], p["max_shards"]) and p["blocks"] <= grid[0]
            assert p["n_shards"] * p["tiles_per_shard"] >= tiles > p["n_shards"] * (p["tiles_per_shard"] - 1)
            assert 1 <= p["chunk"] <= grid[2]
            # blocks: enough waves to take every tile in pulls of `chunk`, never more than resident
            assert p["blocks"] == min(grid[0], -(-tiles // (p["chunk"] * grid[1])))
            # tail_tile_rel marks exactly the tiles that touch byte n or later: (t + 1) stride > n
            probe = set(range(tb, min(tb + 4, p["tile_end"]))) | set(range(max(tb, p["tile_end"] - 4), p["tile_end"]))
            probe |= {t for t in (n // s - 1, n // s, n // s + 1) if tb <= t < p["tile_end"]}
            for t in probe:
                assert (t - tb >= p["tail_rel"]) == ((t + 1) * s > n), (n, t, p)
        assert covered == n_tiles


# ---- seams on the emulator -----------------------------------------------------------------------------------------

@pytest.mark.parametrize("k", SEAM_KS)
def test_seams_against_the_oracle(emu, k):
    """A break at every offset around each tile seam: a seam window emitted twice or dropped changes the counters and the digests."""
    modes = ((1, 1, 1), (1, 0, 0), (0, 0, 0))   # byte path (normalised), bit path, forward-only
    for tag, buf in seam_inputs(k):
        for canon, tie_rc, accept_u in modes:
            want = O.reduce_fused(buf, k, bool(canon), bool(tie_rc), bool(accept_u))
            assert_stats_equal(scan_exact(emu, buf, k, canon, tie_rc, accept_u), want, (k, tag, canon, tie_rc, accept_u))


@pytest.mark.parametrize("k", SEAM_KS)
def test_input_ends_around_a_seam(emu, k):
    """Inputs that end just before, on and just after a seam (the tail tile's masking, a last tile of one byte), and tiny ones."""
    s = stride_of(k)
    rng = np.random.default_rng(77 + k)
    alphabet = np.frombuffer(b"ACGT" * 8 + b"acgtNUu\n", dtype=np.uint8)
    full = alphabet[rng.integers(0, len(alphabet), 3 * s + 64)]
    for n in (0, 1, k - 1, k, k + 1, 15, 16, 17, s - 1, s, s + 1, s + k - 1, s + k, 2 * s - 1, 2 * s + 1, 3 * s + 5):
        buf = full[:n].tobytes()
        for canon, tie_rc, accept_u in ((1, 1, 1), (1, 0, 0), (0, 0, 1)):
            want = O.reduce_fused(buf, k, bool(canon), bool(tie_rc), bool(accept_u))
            assert_stats_equal(scan_exact(emu, buf, k, canon, tie_rc, accept_u), want, (k, n, canon, tie_rc, accept_u))


@pytest.mark.parametrize("k", [16, 17, 21, 22, 23, 24, 32])
def test_seams_quality_masked(emu, k):
    """The quality builds load the quality tile with the same geometry: low qualities on both sides of each seam."""
    s = stride_of(k)
    rng = np.random.default_rng(500 + k)
    buf = np.frombuffer(b"ACGT", dtype=np.uint8)[rng.integers(0, 4, 3 * s - 5)].tobytes()
    for seam in (s, 2 * s):
        for d in (-k, -k + 1, -2, -1, 0, 1, 2, k - 2, k - 1):
            q = np.full(len(buf), 70, dtype=np.uint8)
            q[seam + d] = CUTOFF - 1
            masked = O.quality_mask(buf, q.tobytes(), CUTOFF)
            for canon, tie_rc, accept_u in ((1, 1, 1), (1, 0, 0)):
                want = O.reduce_fused(masked, k, bool(canon), bool(tie_rc), bool(accept_u))
                assert_stats_equal(scan_exact(emu, buf, k, canon, tie_rc, accept_u, qual=q.tobytes()), want, (k, seam, d, canon, tie_rc))
