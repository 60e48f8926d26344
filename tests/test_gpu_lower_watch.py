"""One lower-case byte anywhere in un-normalised byte-path input (PATH_BYTES_CANONICAL with PRE_NONE) must be seen: the speculative builds
of scan2_kernel (k <= 32) and wide_canonical_reduce_kernel with ACCEPT_U = false (k = 33..255) give the packed-value result, which is right
only where no base is lower case, and raise a flag on any byte with bit 5 set so that the byte-walking kernel queued behind them redoes the
launch.  The result is right only if every byte of the input is watched by some tile: halo bytes that are re-read, the lane of tile 0 that
straddles the buffer start, the last 16-byte line, where the padding (lower case here) must not count.  On three tiles of upper-case ACGT
with a few N and line feeds one base at a time turns lower case - every position of the first and the last 48 bytes and of [S - 40, S + 24]
around each seam, every 16th elsewhere; each launch must equal the oracle and count exactly one redone launch (NTK_ACC_REDONE), the
unmodified input none.  test_lower_watch_inputs.py shows that the lower-case base changes the oracle's n_fwd on most positions, so a missed
byte shows in the result as well as in the count.  Run with `pytest -m gpu` on an MI355X."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

import needletail_amd as nt  # noqa: E402
import oracle as O  # noqa: E402  (the checker)
from needletail_amd import _lib as NL  # noqa: E402

import _builds as B  # noqa: E402
from _seams import (LOWER_KS, WIDE_N, WK_ROW, WK_TILE, WK_WAVE, lower_tail_lengths, lower_watch_input, lower_watch_positions, stride_of,  # noqa: E402
                    wide_input)

CUTOFF = 53
PATH, PRE = B.PATH_BYTES_CANONICAL, B.PRE_NONE
LEAD = 1024   # bytes of the allocation in front of the input (the offset-pointer cases read nothing there; it is mapped all the same)


@pytest.fixture(scope="module")
def ctx():
    assert torch.cuda.is_available(), "these tests need a GPU"
    c = nt.Context(0, stream=torch.cuda.current_stream().cuda_stream)
    yield c
    c.set_launch(0, 0)
    c.set_option(NL.OPT_MINIMIZER_ROUTE, 0)
    c.close()


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


def assert_stats_equal(a, b, what=""):
    for key in ("n_total", "n_fwd", "n_rc", "sum", "xor"):
        assert a[key] == b[key], (what, key, a[key], b[key])
    assert np.array_equal(a["hist"], b["hist"]), what


def to_dev(a: np.ndarray, fill: int):
    """LEAD bytes of `fill`, the input (16-byte aligned), `fill` behind it: returns the whole tensor; the input is t[LEAD: LEAD + n]."""
    n = len(a)
    t = torch.full((LEAD + (n + 1023) // 1024 * 1024 + 1024,), fill, dtype=torch.uint8, device="cuda")
    t[LEAD: LEAD + n] = torch.from_numpy(a.copy()).cuda()
    return t


def _wide_reference(recs, k, normalized):
    """CanonicalKmers with 33 <= k <= 255 per record through the oracle's literal iterator: counters + the histogram of the leading six
    bases of every emitted slice (the 2-bit value itself has more than 64 bits: no sum / xor)."""
    code = np.full(256, 255, dtype=np.uint8)
    for i, ch in enumerate(b"ACGT"): code[ch] = i; code[ch | 0x20] = i
    st = {"n_total": 0, "n_fwd": 0, "n_rc": 0, "sum": 0, "xor": 0, "hist": np.zeros(4096, dtype=np.uint64)}
    for r in recs:
        if normalized:
            r = O.normalize(r)[0]
        rc = O.reverse_complement(r)
        pos, flg = O.canonical_kmers_arrays(r, rc, k)
        for p, f in zip(pos.tolist(), flg.tolist()):
            sl = rc[len(rc) - p - k: len(rc) - p] if f else r[p: p + k]
            b = 0
            for ch in sl[:6]: b = b * 4 + int(code[ch])
            st["hist"][b] += 1
        st["n_total"] += len(pos); st["n_rc"] += int(flg.sum()); st["n_fwd"] += len(pos) - int(flg.sum())
    return st


def reference(buf: bytes, k: int):
    if k <= 32:
        return O.reduce_records(buf.split(b"\n"), k, PATH, PRE)
    return _wide_reference(buf.split(b"\n"), k, False)


def assert_speculative(k, quality):
    """The call is a speculative pair: the packed-value build that watches for lower case, the byte-walking kernel behind it."""
    got = B.kernels(B.Call("reduce", k, 0, PATH, PRE, quality, 0))
    first = B.wide_reduce(False, quality) if k > 32 else B.scan2(k, True, False, quality)
    assert got == (first, B.bytes_reduce(k > 32, quality)), got


def sweep_plain(ctx, a, k, positions):
    """One base lower case at a time, no quality stream."""
    n = len(a)
    assert_speculative(k, False)
    t = to_dev(a, 0x61)   # lower-case a in the padding behind byte n (and in front of byte 0)
    seq = t[LEAD:]
    with redone_launches(ctx) as rl:
        ctx.reduce_device(seq, n, k, PATH, PRE, reset=True)
        assert_stats_equal(ctx.accum_read(), reference(a.tobytes(), k), (k, "all upper case"))
        assert rl.count() == 0, (k, "all upper case")
        for p in positions:
            b = a.copy()
            b[p] |= 0x20
            seq[p] = int(b[p])
            ctx.reduce_device(seq, n, k, PATH, PRE, reset=True)
            assert_stats_equal(ctx.accum_read(), reference(b.tobytes(), k), (k, "lower case at", p))
            assert rl.count() == 1, (k, "lower case at", p)
            seq[p] = int(a[p])
        # without the reset flag the count goes up by one per launch
        p = positions[len(positions) // 2]
        ctx.reduce_device(seq, n, k, PATH, PRE, reset=True)
        seq[p] = int(a[p] | 0x20)
        for i in (1, 2, 3):
            ctx.reduce_device(seq, n, k, PATH, PRE)
            assert rl.count() == i, (k, "launch", i)
        seq[p] = int(a[p])
        ctx.reduce_device(seq, n, k, PATH, PRE)
        assert rl.count() == 3, k


def sweep_quality(ctx, a, k, positions):
    """The route rule of test_route_follows_the_masked_watch at every swept position: the lower-case base under a quality below the cutoff
    is masked and not watched (nothing redone), under a high quality it is; both results equal the oracle after quality_mask."""
    n = len(a)
    assert_speculative(k, True)
    t = to_dev(a, 0x61)
    seq = t[LEAD:]
    q = to_dev(np.full(n, 70, dtype=np.uint8), 0)[LEAD:]
    high = np.full(n, 70, dtype=np.uint8).tobytes()
    with redone_launches(ctx) as rl:
        for p in positions:
            b = a.copy()
            b[p] |= 0x20
            seq[p] = int(b[p])
            low = bytearray(high)
            low[p] = CUTOFF - 1
            for name, qual, redone in (("low quality", bytes(low), 0), ("high quality", high, 1)):
                q[p] = qual[p]
                ctx.reduce_device(seq, n, k, PATH, PRE, d_qual=q, quality_cutoff=CUTOFF, reset=True)
                want = reference(O.quality_mask(b.tobytes(), qual, CUTOFF), k)
                assert_stats_equal(ctx.accum_read(), want, (k, "lower case at", p, name))
                assert rl.count() == redone, (k, "lower case at", p, name)
            seq[p] = int(a[p])


def base_positions(a, positions):
    return [p for p in positions if a[p] in b"ACGT"]


@pytest.mark.parametrize("k", LOWER_KS)
def test_one_lower_case_base_is_seen(ctx, k):
    a = lower_watch_input(k)
    s = stride_of(k)
    sweep_plain(ctx, a, k, base_positions(a, lower_watch_positions(len(a), (s, 2 * s))))


@pytest.mark.parametrize("k", LOWER_KS)
def test_one_lower_case_base_under_a_quality_stream(ctx, k):
    a = lower_watch_input(k)
    s = stride_of(k)
    sweep_quality(ctx, a, k, base_positions(a, lower_watch_positions(len(a), (s, 2 * s))))


WIDE_POSITIONS = lower_watch_positions(WIDE_N, (WK_ROW, WK_WAVE, WK_TILE), ends=48, step=WIDE_N)   # around 0, 256, 1024, 4096 and the end


@pytest.mark.parametrize("k", [40, 255])
def test_one_lower_case_base_is_seen_by_the_wide_pair(ctx, k):
    sweep_plain(ctx, wide_input(), k, WIDE_POSITIONS)


@pytest.mark.parametrize("k", [40, 255])
def test_one_lower_case_base_under_a_quality_stream_wide_pair(ctx, k):
    sweep_quality(ctx, wide_input(), k, WIDE_POSITIONS)


@pytest.mark.parametrize("k", [16, 21, 40])
def test_last_line_padding_is_not_watched(ctx, k):
    """The input ends with its last byte at offset 3, 4, 5, 14, 15 and 16 of its 16-byte line (lower_tail_lengths), lower-case bytes behind
    it: all upper case counts no redone launch - the padding is nobody's base, whichever dword of the line it shares with input bytes - and
    with the last byte lower case exactly one.  (The mutation audit's two or_of_input_bytes edits - a dword of exactly four input bytes
    masked to none, a line of 15 input bytes taken whole - passed every sweep before these lengths; profiles/mutation_audit/README.md.)"""
    a = lower_watch_input(k) if k <= 32 else wide_input()
    assert_speculative(k, False)
    t = to_dev(a, 0x61)
    seq = t[LEAD:]
    with redone_launches(ctx) as rl:
        for off, n in lower_tail_lengths(len(a)):
            head = a[:n]
            seq[n:len(a)] = 0x61   # what lay behind byte n is padding now
            ctx.reduce_device(seq, n, k, PATH, PRE, reset=True)
            assert_stats_equal(ctx.accum_read(), reference(head.tobytes(), k), (k, "all upper case, last byte at offset", off))
            assert rl.count() == 0, (k, "all upper case, last byte at offset", off)
            b = head.copy()
            if b[n - 1] not in b"ACGT":
                b[n - 1] = ord("A")
            b[n - 1] |= 0x20
            seq[n - 1] = int(b[n - 1])
            ctx.reduce_device(seq, n, k, PATH, PRE, reset=True)
            assert_stats_equal(ctx.accum_read(), reference(b.tobytes(), k), (k, "last byte lower case at offset", off))
            assert rl.count() == 1, (k, "last byte lower case at offset", off)
            seq[:len(a)] = torch.from_numpy(a.copy()).cuda()


@pytest.mark.parametrize("k", [16, 21, 24, 40])
def test_offset_pointer(ctx, k):
    """The input starts 16 j bytes into a buffer: the lane of tile 0 that straddles the start must not watch what lies in front of it.  A
    lower-case byte just before the pointer and none inside counts nothing and gives the clean result; one at byte 0 of the view counts 1."""
    a = lower_watch_input(k) if k <= 32 else wide_input()
    t = to_dev(a, 0x41)
    with redone_launches(ctx) as rl:
        for j in (1, 3):
            view = a[16 * j:]
            ptr = t.data_ptr() + LEAD + 16 * j
            assert ptr % 16 == 0
            t[LEAD + 16 * j - 1] = int(a[16 * j - 1] | 0x20)
            ctx.reduce_device(ptr, len(view), k, PATH, PRE, reset=True)
            assert_stats_equal(ctx.accum_read(), reference(view.tobytes(), k), (k, j, "lower case before the pointer"))
            assert rl.count() == 0, (k, j, "lower case before the pointer")
            b = view.copy()
            b[0] |= 0x20
            t[LEAD + 16 * j] = int(b[0])
            ctx.reduce_device(ptr, len(view), k, PATH, PRE, reset=True)
            assert_stats_equal(ctx.accum_read(), reference(b.tobytes(), k), (k, j, "lower case at byte 0 of the view"))
            assert rl.count() == 1, (k, j, "lower case at byte 0 of the view")
            t[LEAD + 16 * j - 1] = int(a[16 * j - 1])
            t[LEAD + 16 * j] = int(a[16 * j])
