"""CanonicalKmers with k = 33..255 at the seams of wide_canonical_reduce_kernel on the device: 4096-byte tiles with 16 halo slots (256 bytes),
and inside a tile a DPP max-scan of "last break" over rows of 16 lanes (256 bytes) and over waves (1024 bytes), both folded through LDS with
the halo's value - device-only code that the emulator does not run.  On 2 x 4096 + 300 random upper-case ACGT bytes: one N at every offset of
[seam - k - 18, seam + 18] around 256, 1024, 4096, 4096 + 256, 4096 + 1024 and 8192 (at k = 255 a window reaches 254 bytes back: nearly the
whole halo); an insert that ties over 32 bases slid across every seam (the packed-stream kernel cannot tell its strand and the launch is
redone by the byte-walking kernel: NTK_ACC_REDONE counts it); and the byte-walking kernel alone at its own seams.  Every result is compared
with the numpy restatement of tests/_seams.py wide_reference, which test_wide_seams_emu.py pins against the oracle's literal iterator.  The
route of every launch is observed through NTK_ACC_REDONE or forced through NTK_OPT_MINIMIZER_ROUTE.  Run with `pytest -m gpu` on an MI355X."""
from contextlib import contextmanager

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

import needletail_amd as nt  # noqa: E402
from needletail_amd import _lib as NL  # noqa: E402

import _builds as B  # noqa: E402
from _seams import (WIDE_KS, WIDE_N, WIDE_TIE_KS, wide_break_offsets, wide_input, wide_reference, wide_tie_insert, wide_tie_starts)  # noqa: E402
from _mutant_inputs import WIDE_TILE, tail_input  # noqa: E402

PRES = ((B.PRE_NORMALIZE, "normalised"), (B.PRE_NONE, "raw"))
# canonical_bytes_reduce_kernel (ntk_kernels.hpp): 256 threads (kPlThreads) walk PER = 32 window starts each, a block's tile is 8192 bytes
BYTES_PER, BYTES_THREADS = 32, 256
BYTES_TILE = BYTES_PER * BYTES_THREADS
BYTES_SEAMS = (64 * BYTES_PER, BYTES_TILE // 2, BYTES_TILE)   # a wave's, the middle thread's and the tile's; every 32nd byte between is a thread's


@pytest.fixture(scope="module")
def ctx():
    assert torch.cuda.is_available(), "these tests need a GPU"
    c = nt.Context(0, stream=torch.cuda.current_stream().cuda_stream)
    yield c
    c.set_launch(0, 0)
    c.set_option(NL.OPT_MINIMIZER_ROUTE, 0)
    c.close()


@contextmanager
def ctx_option(c, option, value):
    """ntk_ctx_set_option for the duration of a block (the module's ctx is shared: the default is restored)."""
    c.set_option(option, value)
    try:
        yield
    finally:
        c.set_option(option, 0)


class redone_launches:
    """Context manager: binds an accumulator buffer of the test's own and reports NTK_ACC_REDONE (speculative launches since the last reset whose
    result came from the byte-walking kernel queued behind them) - the route a launch took is otherwise invisible in its (equal) result."""
    def __init__(self, ctx):
        self.ctx = ctx
        self.acc = torch.zeros(NL.ACC_WORDS, dtype=torch.int64, device="cuda")
    def __enter__(self):
        self.ctx.accum_bind_device(self.acc)
        return self
    def __exit__(self, *exc):
        self.ctx.accum_bind_device(None)
    def count(self):
        self.ctx.synchronize()
        return int(self.acc[NL.ACC_REDONE])


def to_dev(buf: bytes):
    n = len(buf)
    t = torch.full(((n + 1023) // 1024 * 1024 + 1024,), 0x41, dtype=torch.uint8, device="cuda")  # 'A' padding: must be ignored
    if n:
        t[:n] = torch.frombuffer(bytearray(buf), dtype=torch.uint8).cuda()
    return t


def assert_stats_equal(a, b, what=""):
    for key in ("n_total", "n_fwd", "n_rc", "sum", "xor"):
        assert a[key] == b[key], (what, key, a[key], b[key])
    assert np.array_equal(a["hist"], b["hist"]), what


def launch_and_check(ctx, rl, t, k, pre, want, redone, what):
    ctx.reduce_device(t, WIDE_N, k, B.PATH_BYTES_CANONICAL, pre, reset=True)
    got = ctx.accum_read()   # (the bound accumulators)
    assert_stats_equal(got, want, what)
    assert got["n_undigested"] == got["n_total"], what
    assert rl.count() == redone, what


def break_sweep(ctx, k, offsets, redone, route):
    base = wide_input()
    t = to_dev(base.tobytes())
    n_char = torch.tensor(ord("N"), dtype=torch.uint8, device="cuda")
    try:
        with redone_launches(ctx) as rl:
            for S, off in [(None, None)] + list(offsets):
                a = base.copy()
                if off is not None:
                    a[off] = ord("N")
                    t[off] = n_char
                want = wide_reference(a.tobytes(), k)
                for pre, pname in PRES:
                    for geometry in ((0, 0), (3, 0)):
                        ctx.set_launch(*geometry)
                        launch_and_check(ctx, rl, t, k, pre, want, redone, (route, "k", k, "seam", S, "break at", off, pname, geometry))
                if off is not None:
                    t[off] = int(base[off])
    finally:
        ctx.set_launch(0, 0)


@pytest.mark.parametrize("k", WIDE_KS)
def test_breaks_around_row_wave_and_tile_seams(ctx, k):
    """The packed-stream kernel's own result on every launch: nothing is redone (upper case, no window ties over 32 bases)."""
    for pre, _ in PRES:
        call = B.Call("reduce", k, 0, B.PATH_BYTES_CANONICAL, pre, False, 0)
        assert B.kernels(call) == (B.wide_reduce(pre >= B.PRE_NORMALIZE, False), B.bytes_reduce(True, False))
    break_sweep(ctx, k, wide_break_offsets(k), 0, "speculative route")


@pytest.mark.parametrize("k", [33, 64, 255])
def test_a_base_in_the_padding_is_ignored(ctx, k):
    """wk_stage_slot's tail rule on the device (tests/_mutant_inputs.py tail_input, added for a survivor of the mutation audit): the last
    16-byte line holds 15 input bytes and an 'A' behind them; were the line taken whole, one window more would be emitted.  The
    packed-stream kernel's own result: nothing is redone."""
    ctx.set_launch(0, 0)
    buf = tail_input(WIDE_TILE + 256)
    assert len(buf) % 16 == 15 and wide_reference(buf + b"A", k)["n_total"] == wide_reference(buf, k)["n_total"] + 1
    t = to_dev(buf)
    want = wide_reference(buf, k)
    with redone_launches(ctx) as rl:
        for pre, pname in PRES:
            call = B.Call("reduce", k, 0, B.PATH_BYTES_CANONICAL, pre, False, 0)
            assert B.kernels(call) == (B.wide_reduce(pre >= B.PRE_NORMALIZE, False), B.bytes_reduce(True, False))
            ctx.reduce_device(t, len(buf), k, B.PATH_BYTES_CANONICAL, pre, reset=True)
            got = ctx.accum_read()
            assert_stats_equal(got, want, ("a base in the padding", k, pname))
            assert got["n_undigested"] == got["n_total"] and rl.count() == 0, (k, pname)


def test_breaks_on_the_direct_route(ctx):
    """NTK_ROUTE_NO_SPECULATION at k = 255: canonical_bytes_reduce_kernel alone, at the seams between its threads (32 starts each), its
    waves and its 8192-byte tiles - the input reaches 300 bytes into the second."""
    assert BYTES_TILE < WIDE_N and all(S % BYTES_PER == 0 for S in BYTES_SEAMS)
    call = B.Call("reduce", 255, 0, B.PATH_BYTES_CANONICAL, B.PRE_NONE, False, NL.ROUTE_NO_SPECULATION)
    assert B.kernels(call) == (B.bytes_reduce(True, False),)
    with ctx_option(ctx, NL.OPT_MINIMIZER_ROUTE, NL.ROUTE_NO_SPECULATION):
        break_sweep(ctx, 255, wide_break_offsets(255, seams=BYTES_SEAMS), 0, "direct route")


@pytest.mark.parametrize("k", WIDE_TIE_KS)
def test_ties_over_32_bases_across_every_seam(ctx, k):
    """A window whose first 32 bases equal the reverse complement of its last 32 starts at every offset of [seam - k - 2, seam + 2]: the
    launch is redone (exactly one count per launch) and gives the reference's result; with one base of the insert changed nothing ties and
    the packed-stream kernel's result stands."""
    ctx.set_launch(0, 0)
    base = wide_input()
    ins = np.frombuffer(wide_tie_insert(k), dtype=np.uint8)
    changed = ins.copy()
    changed[5] = ord("C") if changed[5] != ord("C") else ord("G")
    with redone_launches(ctx) as rl:
        for S, p in wide_tie_starts(k):
            for name, insert, redone in (("insert", ins, 1), ("insert with one base changed", changed, 0)):
                a = base.copy()
                a[p: p + k] = insert
                t = to_dev(a.tobytes())
                want = wide_reference(a.tobytes(), k)
                for pre, pname in PRES:
                    launch_and_check(ctx, rl, t, k, pre, want, redone, ("k", k, "seam", S, name, "at", p, pname))
