"""The windowed minimizers at their tile seams on the device, on all three routes: the register-fused builds scan2_kernel<K, ..., W> (tiles
advance 992 bytes where k + w - 1 <= 32, 976 where it is 33..48), the generic minimizer_scan_kernel (run-time stride 992 / 976 / 960 / 944)
and the two-pass route (scan_kernel materialises at 992; window_min_reduce_kernel<W> runs over 2048 positions with up to 256 of halo).  The
inputs of tests/_seams.py - one N at every offset around each seam of a three-tile input, and a reverse-complement palindrome whose two tied
k-mers (one canonical value, opposite strands, the window's minimum) slide across the seam - go through reduce_device(..., w=w, reset=True) on
the byte path (PRE_NORMALIZE: ties count as rc, U accepted) and on PATH_BITS_CANONICAL (PRE_NONE); every result is compared bit for bit (five
scalars, 4096 bins) with the literal minimizer of every window (oracle).  A window that straddles a seam needs its k-mers imported from the
previous tile, the invalid smear over its w window ends, and the leftmost-minimum rule across the import; a tie resolved the wrong way
changes only n_fwd / n_rc, and test_minimizer_seam_inputs.py shows that these inputs notice it.  The same inputs run through the per-lane
source on the CPU in test_minimizer_seams_emu.py: a mismatch here alone is in what the emulator leaves out (work pulls, launch plan, buffer
bounds, the LDS histogram, the asm regions).  Every route is forced through NTK_OPT_MINIMIZER_ROUTE and checked against the build manifest
(tests/_builds.py, which test_build_manifest.py holds to the shipped code object).  Run with `pytest -m gpu` on an MI355X; measured times
and case counts are in profiles/seam_sweeps/README.md."""
from contextlib import contextmanager

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

import needletail_amd as nt  # noqa: E402
import oracle as O  # noqa: E402  (the checker)
from needletail_amd import _lib as NL  # noqa: E402

import _builds as B  # noqa: E402
from _seams import (ACGT, FUSED_PAIRS, FUSED_Q_PAIRS, GENERIC_PAIRS, TWO_PASS_PAIRS, TWO_PASS_SEAMS, map_threads, min_seam_inputs,  # noqa: E402
                    min_stride, thin_far, tie_insert, two_pass_inputs)
from _mutant_inputs import SCAN_STRIDE, palindrome_kmer_inputs, tail_input  # noqa: E402

CUTOFF = 53
MAX_CASES = 1500
# (name, path, pre, the oracle's (accept_u, tie_rc))
BYTE_PATH = ("bytes", B.PATH_BYTES_CANONICAL, B.PRE_NORMALIZE, (True, True))
BIT_PATH = ("bits", B.PATH_BITS_CANONICAL, B.PRE_NONE, (False, False))
ROUTE_BITS = {"fused": 0, "generic": NL.ROUTE_NO_REGFUSED, "two_pass": NL.ROUTE_TWO_PASS}
FAMILY = {"fused": ("scan2_kernel",), "generic": ("minimizer_scan_kernel",), "two_pass": ("scan_kernel", "window_min_reduce_kernel")}


@pytest.fixture(scope="module")
def ctx():
    assert torch.cuda.is_available(), "these tests need a GPU"
    c = nt.Context(0, stream=torch.cuda.current_stream().cuda_stream)
    yield c
    c.set_launch(0, 0)
    for o in (NL.OPT_MINIMIZER_ROUTE, NL.OPT_MINIMIZER_CHUNK_BYTES):
        c.set_option(o, 0)
    c.close()


@contextmanager
def ctx_option(c, option, value):
    """ntk_ctx_set_option for the duration of a block (the module's ctx is shared: the default is restored)."""
    c.set_option(option, value)
    try:
        yield
    finally:
        c.set_option(option, 0)


def to_dev(buf: bytes, fill: int = 0x41):
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


def template_args(symbol: str):
    return symbol[symbol.index("<") + 1: symbol.rindex(">")].split(", ")


def assert_route(k, w, path, route, extra_bits, quality):
    """The call launches the kernels of the route the test names (the manifest's restatement of the dispatch): the family, for the fused
    builds (k, w), for the generic kernel its key form, and the quality build where a quality stream comes along."""
    call = B.Call("minimizers", k, w, path[1], path[2], quality, ROUTE_BITS[route] | extra_bits)
    syms = B.kernels(call)
    assert tuple(B.family(s) for s in syms) == FAMILY[route], (k, w, route, syms)
    args = template_args(syms[0])
    if route == "fused":   # scan2_kernel<K, TIE_RC, ACCEPT_U, QM, HB, W, FWD>
        assert (args[0], args[5], args[3]) == (str(k), str(w), B.b(quality)), syms
    if route == "generic":   # minimizer_scan_kernel<KW, TIE_RC, ACCEPT_U, QM, F64, MODE>
        assert (args[4], args[3]) == (B.b(k <= 25 and not extra_bits & NL.ROUTE_NO_F64), B.b(quality)), syms


def capped(cases, k, w):
    cases = list(cases)
    return list(thin_far(cases, k, w)) if len(cases) > MAX_CASES else cases


def wants_of(cases, k, w, paths):
    return {p[0]: map_threads(lambda c: O.minimizers_reduce(c[1], k, w, accept_u=p[3][0], tie_rc=p[3][1]), cases) for p in paths}


def run_cases(ctx, k, w, cases, wants, runs, stride):
    """cases: (tag, bytes); wants: {path name: [stats per case]}; runs: (route, extra route bits, paths, chunk bytes).  Every launch names
    seam, offset, route and path in its assertion message."""
    devs = [to_dev(buf) for _, buf in cases]
    for route, extra, paths, chunk in runs:
        for path in paths:
            assert_route(k, w, path, route, extra, False)
        with ctx_option(ctx, NL.OPT_MINIMIZER_ROUTE, ROUTE_BITS[route] | extra), ctx_option(ctx, NL.OPT_MINIMIZER_CHUNK_BYTES, chunk):
            for i, (tag, buf) in enumerate(cases):
                for path in paths:
                    if w <= 255:
                        ctx.reduce_device(devs[i], len(buf), k, path[1], path[2], w=w, reset=True)
                    else:   # ntk_params.flags holds the window in eight bits: w = 256 goes through the entry point that takes it as an argument
                        ctx.accum_reset()
                        ctx.minimizers_reduce_device(devs[i], len(buf), k, w, path[1], path[2])
                    assert_stats_equal(ctx.accum_read(), wants[path[0]][i], (k, w, tag, route, extra, path[0], "stride", stride, "chunk", chunk))


def run_quality(ctx, k, w, stride, route, paths):
    """High qualities everywhere and one below the cutoff at the offset of every break case (no N in the sequence)."""
    cases = capped(min_seam_inputs(k, w, stride), k, w)
    base = cases[0][1]
    quals = []
    for tag, _ in cases:
        if tag[0] == "break":
            q = np.full(len(base), 70, dtype=np.uint8)
            q[tag[2]] = CUTOFF - 1
            quals.append((tag, q.tobytes()))
    d_seq = to_dev(base)
    for path in paths:
        assert_route(k, w, path, route, 0, True)
        wants = map_threads(lambda c: O.minimizers_reduce(O.quality_mask(base, c[1], CUTOFF), k, w, accept_u=path[3][0], tie_rc=path[3][1]), quals)
        with ctx_option(ctx, NL.OPT_MINIMIZER_ROUTE, ROUTE_BITS[route]):
            for (tag, q), want in zip(quals, wants):
                ctx.reduce_device(d_seq, len(base), k, path[1], path[2], w=w, d_qual=to_dev(q, 0), quality_cutoff=CUTOFF, reset=True)
                assert_stats_equal(ctx.accum_read(), want, (k, w, tag, route, path[0], "quality-masked", "stride", stride))
    return len(quals)


# ---- the register-fused pairs: on their own build, on the generic kernel, on the two-pass route ---------------------------------------

@pytest.mark.parametrize("k,w", FUSED_PAIRS)
def test_fused_pair_on_every_route(ctx, k, w):
    """The two-pass route's chunk option is left out here: its smallest accepted value (4096 bytes) is larger than the three-tile input (at
    most 2971 bytes), so no chunk cut falls inside it; test_two_pass_only_pair sweeps the cut."""
    ctx.set_launch(0, 0)
    by_stride = {}
    for route in ("fused", "generic", "two_pass"):
        by_stride.setdefault(min_stride(k, w, route), []).append((route, 0, (BYTE_PATH, BIT_PATH), 0))
    for stride, runs in by_stride.items():
        cases = capped(min_seam_inputs(k, w, stride), k, w)
        run_cases(ctx, k, w, cases, wants_of(cases, k, w, (BYTE_PATH, BIT_PATH)), runs, stride)


@pytest.mark.parametrize("k,w", FUSED_Q_PAIRS)
def test_fused_quality_builds(ctx, k, w):
    ctx.set_launch(0, 0)
    assert run_quality(ctx, k, w, min_stride(k, w, "fused"), "fused", (BYTE_PATH, BIT_PATH)) > 0


# ---- the generic pairs -----------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("k,w", GENERIC_PAIRS)
def test_generic_pair(ctx, k, w):
    """Both key forms where k <= 25 (NTK_ROUTE_NO_F64 takes the general keys)."""
    ctx.set_launch(0, 0)
    stride = min_stride(k, w, "generic")
    runs = [("generic", 0, (BYTE_PATH, BIT_PATH), 0)] + ([("generic", NL.ROUTE_NO_F64, (BYTE_PATH, BIT_PATH), 0)] if k <= 25 else [])
    if B.pick_scan_min(B.resolve_mode(k, BYTE_PATH[1], BYTE_PATH[2]), k, w, False) is None:
        for path in (BYTE_PATH, BIT_PATH):   # no register-fused build: the default route is the generic kernel as well
            assert tuple(B.family(s) for s in B.kernels(B.Call("minimizers", k, w, path[1], path[2], False, 0))) == FAMILY["generic"]
    cases = capped(min_seam_inputs(k, w, stride), k, w)
    run_cases(ctx, k, w, cases, wants_of(cases, k, w, (BYTE_PATH, BIT_PATH)), runs, stride)


def test_generic_pair_quality_masked(ctx):
    ctx.set_launch(0, 0)
    assert run_quality(ctx, 24, 11, min_stride(24, 11, "generic"), "generic", (BYTE_PATH,)) > 0


# ---- the two-pass route alone ----------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("seams", [(TWO_PASS_SEAMS[0], TWO_PASS_SEAMS[2]), (TWO_PASS_SEAMS[1], TWO_PASS_SEAMS[3])], ids=["2048+1984", "4096+3968"])
@pytest.mark.parametrize("k,w", TWO_PASS_PAIRS)
def test_two_pass_only_pair(ctx, k, w, seams):
    """Pairs beyond the fused kernels (k = 32, w >= 50), on the byte path: 3 x 2048 - 5 bytes, swept around the 2048-position seams of
    window_min_reduce_kernel and around the 992-byte seams of scan_kernel nearest to them (each pair of seams is one case of this test: the
    oracle walks w k-mers per window).  Once more with NTK_OPT_MINIMIZER_CHUNK_BYTES at its smallest accepted value, 4096: the chunk cut then
    falls on byte 4096 of the input, which the second pair of seams sweeps - the second chunk is scanned from (4096 - (k + w - 2)) & ~15 on, so
    both kernels' seams move with it."""
    ctx.set_launch(0, 0)
    cases = capped(two_pass_inputs(k, w, seams), k, w)
    assert ctx.get_option(NL.OPT_MINIMIZER_CHUNK_BYTES) > len(cases[0][1]) > 4096   # by default one chunk, with the option two
    runs = [("two_pass", 0, (BYTE_PATH,), 0), ("two_pass", 0, (BYTE_PATH,), 4096)]
    run_cases(ctx, k, w, cases, wants_of(cases, k, w, (BYTE_PATH,)), runs, 992)


# ---- the inputs added for the survivors of the mutation audit (tests/_mutant_inputs.py, profiles/mutation_audit/README.md) -----------------

def check_on_route(ctx, buf, k, w, route, extra, paths, what):
    """One input through one forced route, both paths, against the literal minimizer of every window; to_dev pads with 'A'."""
    t = to_dev(buf)
    for path in paths:
        assert_route(k, w, path, route, extra, False)
    with ctx_option(ctx, NL.OPT_MINIMIZER_ROUTE, ROUTE_BITS[route] | extra):
        for path in paths:
            ctx.reduce_device(t, len(buf), k, path[1], path[2], w=w, reset=True)
            want = O.minimizers_reduce(buf, k, w, accept_u=path[3][0], tie_rc=path[3][1])
            assert_stats_equal(ctx.accum_read(), want, (what, k, w, route, extra, path[0]))


@pytest.mark.parametrize("k", [5, 16, 22, 32])
def test_scan_kernel_ignores_a_base_in_the_padding(ctx, k):
    """The two-pass route with w = 1 (every k-mer is its window's minimizer) on a last 16-byte line of 15 input bytes with an 'A' behind them:
    what scan_kernel materialises for the line and what window_min_reduce_kernel takes from it.  The reduce stops at byte n whatever the
    scan marked valid behind it, so this holds the pair and not lane_tile's tail rule alone; the rule itself shows in the materialised
    valid16 word, test_gpu_build_matrix.py::test_materialize_ignores_a_base_in_the_padding."""
    ctx.set_launch(0, 0)
    buf = tail_input(SCAN_STRIDE)
    assert len(buf) % 16 == 15
    check_on_route(ctx, buf, k, 1, "two_pass", 0, (BYTE_PATH, BIT_PATH), "a base in the padding")


@pytest.mark.parametrize("k,w", [(21, 11), (24, 11), (26, 18), (11, 49)])
def test_generic_kernel_ignores_a_base_in_the_padding(ctx, k, w):
    """minimizer_invalid16's tail rule, both smear forms and both key forms."""
    ctx.set_launch(0, 0)
    buf = tail_input(min_stride(k, w, "generic"))
    assert len(buf) % 16 == 15
    for extra in ((0, NL.ROUTE_NO_F64) if k <= 25 else (0,)):
        check_on_route(ctx, buf, k, w, "generic", extra, (BYTE_PATH, BIT_PATH), "a base in the padding")


@pytest.mark.parametrize("k", [18, 22, 32, 4, 16])
def test_scan_kernel_reports_a_self_palindrome_by_the_paths_tie_rule(ctx, k):
    """lane_tile's strand compare on a k-mer equal to its own reverse complement (the byte path reports rc, the bit path forward), ending
    mid-tile, on both sides of the 992-byte seam and of a lane boundary: scan_kernel through the two-pass route with w = 1."""
    ctx.set_launch(0, 0)
    for e, buf in palindrome_kmer_inputs(k):
        check_on_route(ctx, buf, k, 1, "two_pass", 0, (BYTE_PATH, BIT_PATH), ("self-palindrome ending at", e))


# ---- launch shape ----------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("k,w,route", [(21, 11, "fused"), (23, 12, "fused"), (21, 11, "generic"), (26, 18, "generic"), (21, 11, "two_pass")])
def test_64_tiles_under_a_7_block_launch(ctx, k, w, route):
    """Few blocks: every wave pulls several chunks of consecutive tiles, and the shards' edges fall between tiles.  A break right at every
    third seam, a tied pair across every other one."""
    s = min_stride(k, w, route)
    rng = np.random.default_rng(2100 + 37 * k + w + s)
    a = ACGT[rng.integers(0, 4, 64 * s - 3)].copy()
    d = max(x for x in range(1, w) if (k + x) % 2 == 0)
    pal = np.frombuffer(tie_insert(k, d, rng), dtype=np.uint8)
    for t in range(1, 64):
        if t % 2 == 0:   # its first k-mer ends before the seam, its second behind it (behind the break where the seam has one)
            p = t * s + 1 if t % 3 == 0 else t * s - k - d // 2
            a[p: p + len(pal)] = pal
        if t % 3 == 0:
            a[t * s - 1 + (t % 2)] = ord("N")
    buf = a.tobytes()
    t_dev = to_dev(buf)
    ctx.set_launch(7, 0)
    try:
        with ctx_option(ctx, NL.OPT_MINIMIZER_ROUTE, ROUTE_BITS[route]):
            for path in (BYTE_PATH, BIT_PATH):
                assert_route(k, w, path, route, 0, False)
                want = O.minimizers_reduce(buf, k, w, accept_u=path[3][0], tie_rc=path[3][1])
                ctx.reduce_device(t_dev, len(buf), k, path[1], path[2], w=w, reset=True)
                assert_stats_equal(ctx.accum_read(), want, (k, w, route, path[0], "64 tiles, 7 blocks"))
    finally:
        ctx.set_launch(0, 0)
