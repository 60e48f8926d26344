"""Seam parity of the k-mer builds of scan2_kernel on the device: the tile stride is 1024 - (k - 1) bytes rounded down to a dword (1008 for
k <= 16), so a window at a tile seam must come from exactly one tile.  The seam inputs of test_exact_stride_emu.py - a break at every offset
of [stride - 24, stride + 24] around each seam of a 3-tile input - inputs that end one byte before / after a seam and five bytes into a
fourth tile, and a 64-tile input under a 7-block launch go through reduce_device on the byte path, the bit path, forward-only, quality-masked
and with reset=True; every result is compared bit for bit (five scalars, 4096 bins) with the oracle.  Run with `pytest -m gpu` on an MI355X."""

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

import needletail_amd as nt  # noqa: E402
import oracle as O  # noqa: E402  (the checker)

from _builds import PATH_BITS, PATH_BITS_CANONICAL, PATH_BYTES_CANONICAL, PRE_NONE, PRE_NORMALIZE  # noqa: E402
from _seams import seam_inputs, stride_of  # noqa: E402

KS = (16, 17, 21, 22, 23, 24, 32)
CUTOFF = 53
# (path, pre) and the oracle's (canonical, tie_rc, accept_u) for it
BYTE_PATH = (PATH_BYTES_CANONICAL, PRE_NORMALIZE, (True, True, True))
BIT_PATH = (PATH_BITS_CANONICAL, PRE_NONE, (True, False, False))
FORWARD = (PATH_BITS, PRE_NONE, (False, False, False))
PATHS = {"bytes": BYTE_PATH, "bits": BIT_PATH, "forward": FORWARD}


@pytest.fixture(scope="module")
def ctx():
    assert torch.cuda.is_available(), "these tests need a GPU"
    c = nt.Context(0, stream=torch.cuda.current_stream().cuda_stream)
    yield c
    c.set_launch(0, 0)
    c.close()


def to_dev(buf: bytes, fill: int):
    """The input on the device, 16-byte aligned; what follows byte n is `fill` ('A' behind a sequence: a base the scan must not take)."""
    n = len(buf)
    t = torch.full(((n + 1023) // 1024 * 1024 + 1024,), fill, dtype=torch.uint8, device="cuda")
    if n:
        t[:n] = torch.frombuffer(bytearray(buf), dtype=torch.uint8).cuda()
    return t


def assert_stats_equal(a, b, what=""):
    for key in ("n_total", "n_fwd", "n_rc", "sum", "xor"):
        assert a[key] == b[key], (what, key, a[key], b[key])
    assert np.array_equal(a["hist"], b["hist"]), what


def qualities(n: int, seed: int, low_at=()):
    rng = np.random.default_rng(seed)
    q = rng.integers(CUTOFF, 75, n, dtype=np.uint8)
    q[rng.random(n) < 0.01] = CUTOFF - 1
    for at in low_at:
        if 0 <= at < n:
            q[at] = CUTOFF - 1
    return q.tobytes()


def check_all_paths(ctx, buf: bytes, qual: bytes, k: int, what):
    """The five paths of the issue on one input.  The accumulators are left holding the previous path's result on purpose: reset=True
    has to start from zero each time; the byte path is run a second time without it, on accumulators zeroed by accum_reset()."""
    d_seq, d_qual = to_dev(buf, 0x41), to_dev(qual, 0)
    want = {}
    for name, (path, pre, mode) in PATHS.items():
        want[name] = O.reduce_fused(buf, k, *mode)
        ctx.reduce_device(d_seq, len(buf), k, path, pre, reset=True)
        assert_stats_equal(ctx.accum_read(), want[name], (what, k, name, "reset=True"))
    masked = O.quality_mask(buf, qual, CUTOFF)
    for name in ("bytes", "forward"):
        path, pre, mode = PATHS[name]
        ctx.reduce_device(d_seq, len(buf), k, path, pre, d_qual=d_qual, quality_cutoff=CUTOFF, reset=True)
        assert_stats_equal(ctx.accum_read(), O.reduce_fused(masked, k, *mode), (what, k, name, "quality-masked"))
    ctx.accum_reset()
    ctx.reduce_device(d_seq, len(buf), k, BYTE_PATH[0], BYTE_PATH[1])
    assert_stats_equal(ctx.accum_read(), want["bytes"], (what, k, "bytes", "accum_reset, reset=False"))


@pytest.mark.parametrize("k", KS)
def test_breaks_around_each_seam(ctx, k):
    ctx.set_launch(0, 0)
    s = stride_of(k)
    for tag, buf in seam_inputs(k):
        low = () if tag == "none" else (tag[0] - tag[1], tag[0] + tag[1] + 1)   # a low quality mirrored on the other side of the seam
        check_all_paths(ctx, buf, qualities(len(buf), 3 * s + k, low), k, tag)


@pytest.mark.parametrize("k", KS)
def test_inputs_ending_around_a_seam(ctx, k):
    ctx.set_launch(0, 0)
    s = stride_of(k)
    rng = np.random.default_rng(900 + k)
    alphabet = np.frombuffer(b"ACGT" * 10 + b"acgtNUu\n", dtype=np.uint8)
    full = alphabet[rng.integers(0, len(alphabet), 3 * s + 5)]
    for n in (s - 1, s + 1, 3 * s + 5):
        check_all_paths(ctx, full[:n].tobytes(), qualities(n, n), k, ("n", n))


@pytest.mark.parametrize("k", KS)
def test_64_tiles_under_a_7_block_launch(ctx, k):
    """Few blocks: every wave pulls several chunks of consecutive tiles, and the shards' edges fall between tiles."""
    s = stride_of(k)
    rng = np.random.default_rng(1300 + k)
    alphabet = np.frombuffer(b"ACGT" * 12 + b"acgtNUu\n", dtype=np.uint8)
    a = alphabet[rng.integers(0, len(alphabet), 64 * s - 3)].copy()
    for t in range(1, 64):                      # a clean stretch across every seam, a break right at every third one
        a[t * s - 40: t * s + 40] = np.frombuffer(b"ACGT", dtype=np.uint8)[rng.integers(0, 4, 80)]
        if t % 3 == 0:
            a[t * s - 1 + (t % 2)] = ord("N")
    buf = a.tobytes()
    ctx.set_launch(7, 0)
    try:
        check_all_paths(ctx, buf, qualities(len(buf), 64 * s), k, "64 tiles, 7 blocks")
    finally:
        ctx.set_launch(0, 0)
