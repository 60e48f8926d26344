"""Every build of the dispatch matrix (tests/_builds.py) against the oracle, on one adversarial device buffer.

Reduce entries (every reachable (k, path, pre, quality, route) of the k-mer reduce, a covering set of the windowed-minimizer calls) are
compared with the checkers the suite trusts (O.reduce_fused, O.reduce_records, O.minimizers_reduce, the literal iterator for k > 32) under
the default launch and a few-block one.  Speculative entries also assert the route they took (NTK_ACC_REDONE).  Materialise entries are
compared position by position with planes built from the oracle's literal iterators.  Run with `pytest -m gpu` on an MI355X."""

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

import needletail_amd as nt  # noqa: E402
import oracle as O  # noqa: E402  (the checker)
from needletail_amd import _lib as NL  # noqa: E402

import _builds as B  # noqa: E402
from _mutant_inputs import SCAN_STRIDE, pack16, tail_input  # noqa: E402

GEOMETRIES = ((0, 0), (7, 0))   # the library's grid, and a few-block launch (every block pulls many tiles)
CUTOFF = 53                     # Phred+33 Q20: the seeded qualities sit on both sides of it


@pytest.fixture(scope="module")
def ctx():
    assert torch.cuda.is_available(), "these tests need a GPU"
    c = nt.Context(0, stream=torch.cuda.current_stream().cuda_stream)
    yield c
    c.set_launch(0, 0)
    c.set_option(NL.OPT_MINIMIZER_ROUTE, 0)
    c.close()


def _revcomp_ascii(s: bytes) -> bytes:
    return s[::-1].translate(bytes.maketrans(b"ACGT", b"TGCA"))


def adversarial(seed: int = 0xB11D, upper_only: bool = False):
    """(sequence bytes, quality bytes): records of 1..30, 991..993, 1023..1025 bytes and others, '\\n' after each; breaks on lane (16 B) and
    tile (992 B) edges; N runs of every length up to 34 (k - 1, k, k + 1); palindromes (strand ties at even k); lower case, U / u, IUPAC,
    whitespace, CR and high bytes.  upper_only: ACGT, N and the separator alone (no byte with bit 5 set, no planted inverted repeat)."""
    rng = np.random.default_rng(seed)
    acgt = np.frombuffer(b"ACGT", dtype=np.uint8)
    junk = np.frombuffer(b"NnUuRYKMSWBDHVryk -.*\t\r\x00\x7f\x80\xc3\xff0@>", dtype=np.uint8)
    recs = []
    lengths = list(range(1, 31)) + [991, 992, 993, 1023, 1024, 1025, 15, 16, 17, 31, 32, 33, 63, 64, 65] * 4
    lengths += [int(x) for x in rng.integers(34, 700, 700)] + [3000] * 4   # (3000: clean enough for windows of 255 bases)
    rng.shuffle(lengths)
    cur = 0   # bytes so far: every 50th record is cut so that its break byte lands on a tile / lane edge
    for i, n in enumerate(lengths):
        if i % 50 == 0:
            n = [(991 - cur) % 992, (992 - cur) % 992, (15 - cur) % 16, (16 - cur) % 16][(i // 50) % 4] or 992
        cur += n + 1
        a = acgt[rng.integers(0, 4, n)].copy()
        if 40 < n < 3000:
            for _ in range(int(rng.integers(0, 3))):   # an N run
                ln, at = int(rng.integers(1, 35)), int(rng.integers(0, n))
                a[at: at + ln] = ord("N")
            if rng.random() < 0.3 and not upper_only:  # a palindrome (inverted repeat) of even length
                h = int(rng.integers(4, 40))
                s = acgt[rng.integers(0, 4, h)].tobytes()
                pal = np.frombuffer(s + _revcomp_ascii(s), dtype=np.uint8)
                at = int(rng.integers(0, max(1, n - len(pal))))
                a[at: at + len(pal)] = pal[: n - at]
        if not upper_only:
            m = rng.random(n)
            a[m < 0.03] |= 0x20                        # lower case
            if rng.random() < 0.2:                     # a soft-masked stretch
                at = int(rng.integers(0, n)); a[at: at + int(rng.integers(1, 60))] |= 0x20
            j = (m > 0.99) & (n < 3000)
            a[j] = junk[rng.integers(0, len(junk), int(j.sum()))]
        else:
            a[rng.random(n) < 0.004] = ord("N")
        recs.append(a.tobytes())
    seq = b"\n".join(recs) + b"\n"
    q = rng.integers(CUTOFF + 1, 75, len(seq), dtype=np.uint8)   # a good read: most bases above the cutoff
    low = rng.random(len(seq)) < 0.01
    q[low] = rng.integers(33, CUTOFF, int(low.sum()), dtype=np.uint8)
    q[rng.random(len(seq)) < 0.02] = CUTOFF        # on the cutoff: kept
    q[rng.random(len(seq)) < 0.005] = CUTOFF - 1   # one below: masked
    sq = np.frombuffer(seq, dtype=np.uint8)
    q[sq == ord("\n")] = 73                       # the separator's quality is ignored by contract: keep it above the cutoff
    return seq, q.tobytes()


def to_dev(buf: bytes, fill: int = 0x41):
    n = len(buf)
    t = torch.full(((n + 1023) // 1024 * 1024 + 1024,), fill, dtype=torch.uint8, device="cuda")
    t[:n] = torch.frombuffer(bytearray(buf), dtype=torch.uint8).cuda()
    return t


def assert_stats_equal(a, b, what=""):
    for key in ("n_total", "n_fwd", "n_rc", "sum", "xor"):
        assert a[key] == b[key], (what, key, a[key], b[key])
    assert np.array_equal(a["hist"], b["hist"]), what


def _split_masked(seq: bytes, qual: bytes, quality: bool, seps: bytes):
    """The pieces between separator bytes, each quality-masked first when `quality` (per record, as the literal chain does)."""
    cuts = [i for i, c in enumerate(seq) if c in seps]
    out, s0 = [], 0
    for c in cuts + [len(seq)]:
        r = seq[s0:c]
        out.append(O.quality_mask(r, qual[s0:c], CUTOFF) if quality else r)
        s0 = c + 1
    return out


_CODE = np.full(256, 255, dtype=np.uint8)
for _i, _ch in enumerate(b"ACGT"):
    _CODE[_ch] = _i
    _CODE[_ch | 0x20] = _i


def wide_reference(recs, k, normalized):
    """CanonicalKmers with 33 <= k <= 255 per record through the oracle's literal iterator: counters and the histogram of the leading six
    bases of every emitted slice (no sum / xor of values of more than 64 bits)."""
    st = {"n_total": 0, "n_fwd": 0, "n_rc": 0, "sum": 0, "xor": 0, "hist": np.zeros(4096, dtype=np.uint64)}
    for r in recs:
        if normalized:
            r = O.normalize(r)[0]
        if len(r) < k:
            continue
        rc = O.reverse_complement(r)
        pos, flg = O.canonical_kmers_arrays(r, rc, k)
        if not len(pos):
            continue
        pos = pos.astype(np.int64)
        fw, rv = _CODE[np.frombuffer(r, dtype=np.uint8)].astype(np.int64), _CODE[np.frombuffer(rc, dtype=np.uint8)].astype(np.int64)
        start = np.where(flg == 1, len(rc) - pos - k, pos)
        src = np.where(flg == 1, 1, 0)
        b = np.zeros(len(pos), dtype=np.int64)
        for i in range(6):
            b = b * 4 + np.where(src == 1, rv[start + i], fw[start + i])
        st["hist"] += np.bincount(b, minlength=4096).astype(np.uint64)
        st["n_total"] += len(pos); st["n_rc"] += int(flg.sum()); st["n_fwd"] += len(pos) - int(flg.sum())
    return st


class Data:
    """The two device buffers, built once, and the oracle's answers, each computed once."""
    def __init__(self):
        self.seq, self.qual = adversarial()
        self.up, self.up_qual = adversarial(0xB11E, upper_only=True)
        self.masked = O.quality_mask(self.seq, self.qual, CUTOFF)
        self.up_masked = O.quality_mask(self.up, self.up_qual, CUTOFF)
        self.dev = {False: to_dev(self.seq), True: to_dev(self.up)}
        self.dev_q = {False: to_dev(self.qual, 0), True: to_dev(self.up_qual, 0)}
        self.cache = {}

    def text(self, upper):
        return (self.up, self.up_qual, self.up_masked) if upper else (self.seq, self.qual, self.masked)

    def expect(self, c: B.Call, upper=False):
        m = B.resolve_mode(c.k, c.path, c.pre)
        if c.entry == "minimizers":
            key = ("min", c.k, c.w, m.accept_u, m.tie_rc, c.quality, upper)
        elif m.raw_bytes and c.k > 32:
            key = ("wide", c.k, m.accept_u, c.quality, upper)
        elif m.raw_bytes:
            key = ("raw", c.k, c.quality, upper)
        else:
            key = ("fused", c.k, m.canon, m.tie_rc, m.accept_u, c.quality, upper)
        if key not in self.cache:
            seq, qual, masked = self.text(upper)
            src = masked if c.quality else seq
            if key[0] == "min":
                self.cache[key] = O.minimizers_reduce(src, c.k, c.w, m.accept_u, m.tie_rc)
            elif key[0] == "wide":
                self.cache[key] = wide_reference(_split_masked(seq, qual, c.quality, b"\n\r\t " if m.accept_u else b"\n"), c.k, m.accept_u)
            elif key[0] == "raw":
                self.cache[key] = O.reduce_records(_split_masked(seq, qual, c.quality, b"\n"), c.k, B.PATH_BYTES_CANONICAL, B.PRE_NONE)
            else:
                self.cache[key] = O.reduce_fused(src, c.k, m.canon, m.tie_rc, m.accept_u)
        return self.cache[key]


@pytest.fixture(scope="module")
def data():
    return Data()


def _reduce(ctx, data, c: B.Call, upper=False):
    ctx.set_option(NL.OPT_MINIMIZER_ROUTE, c.route)
    seq = data.text(upper)[0]
    ctx.reduce_device(data.dev[upper], len(seq), c.k, c.path, c.pre, w=c.w,
                      d_qual=data.dev_q[upper] if c.quality else None, quality_cutoff=CUTOFF if c.quality else 0, reset=True)
    return ctx.accum_read()


def _redone(acc):
    torch.cuda.synchronize()
    return int(acc[NL.ACC_REDONE])


def test_the_buffer_has_its_edges(data):
    seq = np.frombuffer(data.seq, dtype=np.uint8)
    nl = np.flatnonzero(seq == ord("\n"))
    assert 200_000 < len(seq) < 400_000
    assert any((nl + 1) % 992 == 0) and any(nl % 992 == 0) and any((nl + 1) % 16 == 0) and any(nl % 16 == 0)
    lens = np.diff(np.concatenate([[-1], nl])) - 1
    assert {15, 16, 17, 991, 992, 993, 1023, 1024, 1025} <= set(lens.tolist())
    assert all(ch in data.seq for ch in b"acgtUuRY \t\r\x80\xff")
    assert not any(ch in data.up for ch in b"acgtnuU \t\r")
    q = np.frombuffer(data.qual, dtype=np.uint8)
    assert (q < CUTOFF).any() and (q == CUTOFF).any()


def reduce_calls():
    return [c for c in B.calls() if c.entry == "reduce"]


def minimizer_calls():
    """A covering set: for every minimizer build, the first call (manifest order) that launches it."""
    seen, out = set(), []
    for c in B.calls():
        if c.entry != "minimizers":
            continue
        new = [s for s in B.kernels(c) if s not in seen]
        if new:
            out.append(c)
            seen.update(B.kernels(c))
    return out


def test_reduce_entries_against_the_oracle(ctx, data):
    """Every k-mer reduce entry (k = 1..32 on every (path, pre), k > 32 on the byte path, with and without a quality stream, speculation
    on and off) under both geometries; the route of every speculative entry through NTK_ACC_REDONE."""
    acc = torch.zeros(NL.ACC_WORDS, dtype=torch.int64, device="cuda")
    ctx.accum_bind_device(acc)
    n_runs = 0
    try:
        for c in reduce_calls():
            m = B.resolve_mode(c.k, c.path, c.pre)
            spec = m.raw_bytes and not c.route & B.ROUTE_NO_SPECULATION
            for geometry in GEOMETRIES:
                ctx.set_launch(*geometry)
                got = _reduce(ctx, data, c)
                assert_stats_equal(got, data.expect(c), (c, geometry))
                if m.raw_bytes:
                    # mixed case: lower case with a quality above the cutoff exists, so the byte-walking kernel redid every speculative launch
                    # (normalised k > 32 input redoes only on 32-base ties: not asserted here)
                    if not m.accept_u:
                        assert _redone(acc) == (1 if spec else 0), (c, geometry)
                    got = _reduce(ctx, data, c, upper=True)
                    assert_stats_equal(got, data.expect(c, upper=True), (c, geometry, "upper case"))
                    assert _redone(acc) == 0, (c, geometry, "upper case: the packed-value kernel's result stands")
                n_runs += 1
    finally:
        ctx.accum_bind_device(None)
        ctx.set_launch(0, 0)
        ctx.set_option(NL.OPT_MINIMIZER_ROUTE, 0)
    print(f"reduce entries: {len(reduce_calls())}, runs {n_runs}")


def test_minimizer_entries_against_the_oracle(ctx, data):
    """A call for every fused, generic and two-pass minimizer build, with and without a quality stream, under both geometries."""
    calls = minimizer_calls()
    covered = {s for c in calls for s in B.kernels(c)}
    want = {s for s, cs in B.manifest().items() if any(c.entry == "minimizers" for c in cs)}
    assert covered == want
    try:
        for c in calls:
            for geometry in GEOMETRIES:
                ctx.set_launch(*geometry)
                assert_stats_equal(_reduce(ctx, data, c), data.expect(c), (c, geometry))
    finally:
        ctx.set_launch(0, 0)
        ctx.set_option(NL.OPT_MINIMIZER_ROUTE, 0)
    print(f"minimizer entries: {len(calls)}")


# ---- materialise mode, position by position ------------------------------------------------------------------------------

def _window_values(codes: np.ndarray, starts: np.ndarray, k: int) -> np.ndarray:
    v = np.zeros(len(starts), dtype=np.uint64)
    for i in range(k):
        v = (v << np.uint64(2)) | codes[starts + i].astype(np.uint64)
    return v


def expected_planes(buf: bytes, k: int, path: int, pre: int):
    """(valid, rc, values) per byte of `buf` from the oracle's literal iterators.  Every maximal run of base bytes of the mode (ACGTacgt, and
    U / u under PRE_NORMALIZE*) is a sequence of its own: the runs are laid side by side with one N between them (where the bytes were),
    so one iterator call covers all of them.  The bit paths take O.bit_kmers_arrays; the byte path O.normalize, then
    O.canonical_kmers_arrays, and the 2-bit value of the emitted slice (O.bytes_to_bitmer, vectorised; pinned in the test).  Each k-mer
    sits at its window-end byte."""
    m = B.resolve_mode(k, path, pre)
    a = np.frombuffer(buf, dtype=np.uint8)
    base = _CODE[a] != 255
    if m.accept_u:
        base |= (a == ord("U")) | (a == ord("u"))
    runs = np.where(base, a, ord("N")).astype(np.uint8)
    if m.accept_u:
        runs[(a == ord("U")) | (a == ord("u"))] = ord("T")
    n = len(a)
    valid, rcf, vals = np.zeros(n, dtype=bool), np.zeros(n, dtype=bool), np.zeros(n, dtype=np.uint64)
    if path == B.PATH_BYTES_CANONICAL:
        norm = O.normalize(runs.tobytes())[0]
        assert len(norm) == n
        rc = O.reverse_complement(norm)
        pos, flg = O.canonical_kmers_arrays(norm, rc, k)
        pos = pos.astype(np.int64)
        fw = _CODE[np.frombuffer(norm, dtype=np.uint8)]
        rv = _CODE[np.frombuffer(rc, dtype=np.uint8)]
        val = np.where(flg == 1, _window_values(rv, np.where(flg == 1, n - pos - k, 0), k), _window_values(fw, np.where(flg == 1, 0, pos), k))
    else:
        pos, val, flg = O.bit_kmers_arrays(runs.tobytes(), k, path == B.PATH_BITS_CANONICAL)
        pos = pos.astype(np.int64)
    ends = pos + k - 1
    valid[ends] = True
    rcf[ends] = flg.astype(bool)
    vals[ends] = val
    return valid, rcf, vals


def _planes_stats(valid, rcf, vals, k):
    """The reduction of a set of planes, as the oracle's stats: counters, sum, xor and the histogram of the leading bases."""
    v = vals[valid]
    shift = 2 * k - 12 if k >= 6 else 0
    hist = np.bincount((v >> np.uint64(shift)).astype(np.int64), minlength=4096).astype(np.uint64)
    return {"n_total": int(valid.sum()), "n_rc": int(rcf[valid].sum()), "n_fwd": int(valid.sum() - rcf[valid].sum()),
            "sum": int(v.sum(dtype=np.uint64)), "xor": int(np.bitwise_xor.reduce(v)) if len(v) else 0, "hist": hist}


def test_expected_planes_helper_is_pinned(data):
    """The per-position helper's own reduction equals O.reduce_fused on the same buffer, and its byte-path values are O.bytes_to_bitmer of the
    emitted slices (CPU only: it holds the helper, not the kernels)."""
    seq = data.seq
    for path, pre in ((B.PATH_BITS, B.PRE_NONE), (B.PATH_BITS_CANONICAL, B.PRE_NORMALIZE), (B.PATH_BYTES_CANONICAL, B.PRE_NORMALIZE)):
        for k in (1, 5, 6, 16, 17, 21, 32):
            m = B.resolve_mode(k, path, pre)
            valid, rcf, vals = expected_planes(seq, k, path, pre)
            assert_stats_equal(_planes_stats(valid, rcf, vals, k), O.reduce_fused(seq, k, m.canon, m.tie_rc, m.accept_u), (path, pre, k))
    k = 21
    valid, rcf, vals = expected_planes(seq, k, B.PATH_BYTES_CANONICAL, B.PRE_NORMALIZE)
    ends = np.flatnonzero(valid)
    for e in ends[:: max(1, len(ends) // 300)]:
        rec = seq[e - k + 1: e + 1].upper().replace(b"U", b"T")
        sl = O.reverse_complement(rec) if rcf[e] else rec
        assert O.bytes_to_bitmer(sl) == int(vals[e]), e


def _materialize(ctx, dev, n, k, path, pre, dq=None, with_values=True, guard=1024):
    """Outputs at exactly the documented sizes (round_up(n, 16) values, ceil(n / 16) flag words) with a sentinel guard behind each."""
    nv, nw = (n + 15) // 16 * 16, (n + 15) // 16
    vals = torch.full((nv + guard,), 0x5A5A5A5A5A5A5A5A, dtype=torch.int64, device="cuda")
    v16 = torch.full((nw + guard,), 0x5A5A, dtype=torch.int16, device="cuda")
    r16 = torch.full((nw + guard,), 0x5A5A, dtype=torch.int16, device="cuda")
    ctx.materialize_device(dev, n, k, path, pre, vals if with_values else None, v16, r16,
                           d_qual=dq, quality_cutoff=CUTOFF if dq is not None else 0)
    torch.cuda.synchronize()
    vals, v16, r16 = vals.cpu().numpy().view(np.uint64), v16.cpu().numpy().view(np.uint16), r16.cpu().numpy().view(np.uint16)
    assert (v16[nw:] == 0x5A5A).all() and (r16[nw:] == 0x5A5A).all(), ("flag guard", n, k)
    assert (vals[nv:] == 0x5A5A5A5A5A5A5A5A).all(), ("value guard", n, k)
    if not with_values:
        assert (vals == 0x5A5A5A5A5A5A5A5A).all()
    e = np.arange(n)
    valid = ((v16[e // 16] >> (15 - e % 16)) & 1).astype(bool)
    rcf = ((r16[e // 16] >> (15 - e % 16)) & 1).astype(bool)
    return valid, rcf, vals[:n], v16[:nw].copy(), r16[:nw].copy()


def materialize_calls():
    return [c for c in B.calls() if c.entry == "materialize"]


def test_materialize_entries_position_by_position(ctx, data):
    """k = 1..32 on every reachable (path, pre), with and without a quality stream: the valid plane bit for bit, the rc plane and the values on
    valid positions."""
    n = len(data.seq)
    cache = {}
    calls = materialize_calls()
    assert len(calls) == 10 * 32 * 2
    for c in calls:
        m = B.resolve_mode(c.k, c.path, c.pre)
        key = (c.k, m.canon, m.tie_rc, m.accept_u, c.quality)
        if key not in cache:
            cache[key] = expected_planes(data.masked if c.quality else data.seq, c.k, c.path, c.pre)
        ev, er, evals = cache[key]
        gv, gr, gvals, _, _ = _materialize(ctx, data.dev[False], n, c.k, c.path, c.pre, data.dev_q[False] if c.quality else None)
        assert np.array_equal(gv, ev), (c, "valid plane", np.flatnonzero(gv != ev)[:8])
        assert np.array_equal(gr[ev], er[ev]), (c, "rc plane")
        assert np.array_equal(gvals[ev], evals[ev]), (c, "values")
    print(f"materialise entries: {len(calls)}")


@pytest.mark.parametrize("n", [12_345, 16 * 777 + 1, 992 * 13 + 1, 992 * 40, 1])
def test_materialize_exact_sizes_and_flags_only(ctx, data, n):
    """Outputs of exactly the documented sizes stay inside them (odd n, one past a multiple of 16 and of 992); d_values = NULL writes the same
    flag planes and no value."""
    sub = data.seq[:n]
    for k, path, pre in ((21, B.PATH_BYTES_CANONICAL, B.PRE_NORMALIZE), (7, B.PATH_BITS, B.PRE_NONE), (32, B.PATH_BITS_CANONICAL, B.PRE_NORMALIZE)):
        ev, er, evals = expected_planes(sub, k, path, pre)
        gv, gr, gvals, w16, r16 = _materialize(ctx, data.dev[False], n, k, path, pre)
        assert np.array_equal(gv, ev) and np.array_equal(gr[ev], er[ev]) and np.array_equal(gvals[ev], evals[ev]), (n, k, path)
        fv, fr, _, fw16, fr16 = _materialize(ctx, data.dev[False], n, k, path, pre, with_values=False)
        assert np.array_equal(fw16, w16) and np.array_equal(fr16, r16), (n, k, path, "flags only")


@pytest.mark.parametrize("k", [5, 16, 21, 22, 32])
def test_materialize_ignores_a_base_in_the_padding(ctx, k):
    """lane_tile's tail rule on the device, where it shows: a last 16-byte line of 15 input bytes with an 'A' behind them
    (tests/_mutant_inputs.py), materialised.  MaterializeSink::end_tile stores valid16 = ~inval as lane_tile leaves it, unclipped, so bit 0 of
    the last word is position n: were the line taken whole (keep >= 15 for keep >= 16), that bit would be set - nothing else differs, and no
    reduction over the planes reads it (window_min_reduce_kernel stops at n).  The whole valid16 and rc16 planes, that word included, and the
    values on valid positions against the oracle; k = 21 on the canonical paths is the k-specialised build."""
    ctx.set_launch(0, 0)
    buf = tail_input(SCAN_STRIDE)
    n = len(buf)
    assert n % 16 == 15 and n > SCAN_STRIDE
    dev = to_dev(buf)   # 'A' behind byte n
    for path, pre in ((B.PATH_BYTES_CANONICAL, B.PRE_NORMALIZE), (B.PATH_BITS_CANONICAL, B.PRE_NONE), (B.PATH_BITS, B.PRE_NONE)):
        m = B.resolve_mode(k, path, pre)
        syms = B.kernels(B.Call("materialize", k, 0, path, pre, False, 0))
        assert syms == (B.pick_scan_materialize(m, k, False),) and B.family(syms[0]) == "scan_kernel", syms
        assert ("21, false>" in syms[0]) == (k == 21 and m.canon), syms
        ev, er, evals = expected_planes(buf, k, path, pre)
        assert ev[n - 1] and expected_planes(buf + b"A", k, path, pre)[0][n]   # not vacuous: the reading that takes the byte emits there
        gv, gr, gvals, v16, r16 = _materialize(ctx, dev, n, k, path, pre)
        assert v16[-1] & 1 == 0, ("the window ending on the padding byte is marked valid", k, path, hex(v16[-1]))
        assert np.array_equal(v16, pack16(ev)), (k, path, "valid16", np.flatnonzero(v16 != pack16(ev))[:8])
        assert np.array_equal(r16, pack16(er & ev)), (k, path, "rc16")
        assert np.array_equal(gvals[ev], evals[ev]), (k, path, "values")
