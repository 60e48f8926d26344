"""GPU tests of quality masking on byte-path input that was not normalised (NTK_PATH_BYTES_CANONICAL with pre = NONE / STRIP_RETURNS, any
k <= 255) and at k = 33..255 (normalised or not): `(seq, qual).quality_mask(cutoff)` followed by `canonical_kmers(k, &rc)` (reference
src/sequence.rs:237-239,285-296), against the oracle's literal per-record chain.  Run with `pytest -m gpu` on an MI355X."""
import os
import re

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

import needletail_amd as nt  # noqa: E402
import oracle as O  # noqa: E402  (the checker)
from needletail_amd import _lib as NL  # noqa: E402
from _fastx import fasta_raw_seqs  # noqa: E402


@pytest.fixture(scope="module")
def ctx():
    assert torch.cuda.is_available(), "these tests need a GPU"
    c = nt.Context(0, stream=torch.cuda.current_stream().cuda_stream)
    yield c
    c.set_launch(0, 0)
    c.set_option(NL.OPT_MINIMIZER_ROUTE, 0)
    c.close()


def to_dev(buf: bytes):
    n = len(buf)
    t = torch.full(((n + 1023) // 1024 * 1024 + 1024,), 0x41, dtype=torch.uint8, device="cuda")  # 'A' padding: must be ignored
    if n:
        t[:n] = torch.frombuffer(bytearray(buf), dtype=torch.uint8).cuda()
    return t


def _qual_dev(qual: bytes):
    n = len(qual)
    t = torch.zeros(((n + 1023) // 1024 * 1024 + 1024,), dtype=torch.uint8, device="cuda")  # quality 0 in the padding
    if n:
        t[:n] = torch.frombuffer(bytearray(qual), dtype=torch.uint8).cuda()
    return t


class redone_launches:
    """Binds an accumulator buffer of the test's own and reports NTK_ACC_REDONE (speculative launches since the last reset whose result came
    from the byte-walking kernel queued behind them)."""
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


def _wide_reference(recs, k, normalized):
    """CanonicalKmers with 33 <= k <= 255 per record through the oracle's literal iterator: counters + the histogram of the leading six bases
    of every emitted slice (no sum / xor on values of more than 64 bits)."""
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


def _records(rng, n_rec, lo, hi, p_lower, p_junk):
    """Mixed-case records with N / U / junk bytes (as test_gpu_parity's un-normalised reduce test builds them)."""
    out = []
    for _ in range(n_rec):
        n = int(rng.integers(lo, hi))
        a = np.frombuffer(b"ACGT", dtype=np.uint8)[rng.integers(0, 4, n)].copy()
        m = rng.random(n)
        a[m < p_lower] |= 0x20
        j = m > 1 - p_junk
        a[j] = np.frombuffer(b"NnUuRYKM-.*\x00\xff", dtype=np.uint8)[rng.integers(0, 13, int(j.sum()))]
        out.append(a.tobytes())
    return out


def _phred(rng, n, low=0.03):
    """Phred+33 qualities of a good read: most at or above Q20 ('5' = 53), a few below."""
    q = rng.integers(53, 75, n, dtype=np.uint8)
    bad = rng.random(n) < low
    q[bad] = rng.integers(33, 53, int(bad.sum()), dtype=np.uint8)
    return q.tobytes()


def _batch(recs, quals, sep_qual=0x21):
    """The device batch layout: records back to back, one break byte each; the quality under the break byte is ignored by contract."""
    seq = b"".join(r + b"\n" for r in recs)
    qual = b"".join(q + bytes([sep_qual]) for q in quals)
    return seq, qual


def _masked_bytes(recs, quals, cutoff):
    """What the kernels' bit-5 watch sees: bit 7 set on a masked byte."""
    return [bytes((b | 0x80) if q < cutoff else b for b, q in zip(r, q_)) for r, q_ in zip(recs, quals)]


def _watch_fires(recs, quals, cutoff):
    """Some byte of the input has bit 5 set and was not masked (the only route from a clean speculative launch to the redo)."""
    return any((b & 0xA0) == 0x20 for r in _masked_bytes(recs, quals, cutoff) for b in r)


def _tie32(masked_recs, k, normalized):
    """Some emitted k-mer agrees with its reverse complement over the first 32 bases (the k > 32 kernel's other reason to redo)."""
    comp = bytes.maketrans(b"ACGT", b"TGCA")
    for r in masked_recs:
        r = O.normalize(r)[0] if normalized else r.upper()
        for run in re.findall(rb"[ACGT]{%d,}" % k, r):
            n, rc = len(run), run[::-1].translate(comp)
            # window [i, i + k): its first 32 bases against the reverse complement of its last 32, rc[n - i - k, n - i - k + 32)
            if any(run[i: i + 32] == rc[n - i - k: n - i - k + 32] for i in range(n - k + 1)):
                return True
    return False


# ---- k <= 32: the speculative scan and the byte-walking kernel with a quality stream ----------------------------------------------------

@pytest.mark.parametrize("k", [1, 4, 11, 16, 17, 21, 31, 32])
def test_quality_masked_reduce_on_raw_bytes(ctx, k):
    """Mixed-case records with junk bytes, Phred+33 and arbitrary qualities, every cutoff class; both routes, two launch geometries,
    bit-exact against quality_mask -> CanonicalKmers on the bytes as they are (the oracle's literal chain per record)."""
    rng = np.random.default_rng(7100 + k)
    recs = _records(rng, 300, 0, 400, 0.3, 0.02) + _records(rng, 30, 3000, 6000, 0.5, 0.001) + [b"acgTT", b"", b"A", b"ACGT" * 50, b"acgt" * 50]
    phred = [_phred(rng, len(r), 0.1) for r in recs]
    anyq = [rng.integers(0, 256, len(r), dtype=np.uint8).tobytes() for r in recs]
    try:
        for qname, quals in (("phred", phred), ("arbitrary", anyq)):
            seq, qual = _batch(recs, quals, sep_qual=int(rng.integers(0, 256)))
            t, q = to_dev(seq), _qual_dev(qual)
            for cutoff in (1, 36, 53, 128, 129, 255):
                masked = [O.quality_mask(r, qq, cutoff) for r, qq in zip(recs, quals)]
                for pre in (nt.PRE_NONE, nt.PRE_STRIP_RETURNS):
                    want = O.reduce_records(masked, k, nt.PATH_BYTES_CANONICAL, pre)
                    for route in (0, NL.ROUTE_NO_SPECULATION):
                        ctx.set_option(NL.OPT_MINIMIZER_ROUTE, route)
                        for launch in ((0, 0), (3, 0)):
                            ctx.set_launch(*launch)
                            ctx.reduce_device(t, len(seq), k, nt.PATH_BYTES_CANONICAL, pre, d_qual=q, quality_cutoff=cutoff, reset=True)
                            assert_stats_equal(ctx.accum_read(), want, (qname, k, cutoff, pre, route, launch))
    finally:
        ctx.set_launch(0, 0)
        ctx.set_option(NL.OPT_MINIMIZER_ROUTE, 0)


@pytest.mark.parametrize("k", [21, 40])
def test_route_follows_the_masked_watch(ctx, k):
    """Which kernel's result a launch kept: upper-case input stands; lower case only under masked qualities stands too (the watch skips
    masked bytes); one unmasked lower-case base sends the launch to the byte-walking kernel.  Every result against the literal chain."""
    rng = np.random.default_rng(7200 + k)
    cutoff = 53
    upper = _records(rng, 200, 0, 500, 0.0, 0.0)
    quals = [_phred(rng, len(r)) for r in upper]
    # lower case exactly where the quality is below the cutoff
    hidden = [bytes((b | 0x20) if qq < cutoff else b for b, qq in zip(r, q_)) for r, q_ in zip(upper, quals)]
    assert any(b & 0x20 for r in hidden for b in r)
    # ... and one lower-case base under a good quality
    i = max(range(len(hidden)), key=lambda j: len(hidden[j]))
    pos = next(p for p in range(len(hidden[i]) // 2, len(hidden[i])) if quals[i][p] >= cutoff)
    one = list(hidden)
    one[i] = hidden[i][:pos] + bytes([hidden[i][pos] | 0x20]) + hidden[i][pos + 1:]

    def reference(recs):
        masked = [O.quality_mask(r, q_, cutoff) for r, q_ in zip(recs, quals)]
        if k <= 32:
            return O.reduce_records(masked, k, nt.PATH_BYTES_CANONICAL, nt.PRE_NONE)
        return _wide_reference(masked, k, False)

    for name, recs, redone in (("upper case", upper, 0), ("lower case under masked qualities", hidden, 0), ("one unmasked lower-case base", one, 1)):
        assert _watch_fires(recs, quals, cutoff) == bool(redone), name
        seq, qual = _batch(recs, quals)
        t, q = to_dev(seq), _qual_dev(qual)
        want = reference(recs)
        with redone_launches(ctx) as rl:
            ctx.reduce_device(t, len(seq), k, nt.PATH_BYTES_CANONICAL, nt.PRE_NONE, d_qual=q, quality_cutoff=cutoff, reset=True)
            assert rl.count() == redone, (name, k)
        ctx.reduce_device(t, len(seq), k, nt.PATH_BYTES_CANONICAL, nt.PRE_NONE, d_qual=q, quality_cutoff=cutoff, reset=True)
        got = ctx.accum_read()
        assert_stats_equal(got, want, (name, k))
        assert got["n_undigested"] == (got["n_total"] if k > 32 else 0)
        try:
            ctx.set_option(NL.OPT_MINIMIZER_ROUTE, NL.ROUTE_NO_SPECULATION)
            with redone_launches(ctx) as rl:   # the direct route: nothing speculative to redo
                ctx.reduce_device(t, len(seq), k, nt.PATH_BYTES_CANONICAL, nt.PRE_NONE, d_qual=q, quality_cutoff=cutoff, reset=True)
                assert rl.count() == 0, (name, k)
            ctx.reduce_device(t, len(seq), k, nt.PATH_BYTES_CANONICAL, nt.PRE_NONE, d_qual=q, quality_cutoff=cutoff, reset=True)
            assert_stats_equal(ctx.accum_read(), want, (name, k, "direct route"))
        finally:
            ctx.set_option(NL.OPT_MINIMIZER_ROUTE, 0)


# ---- k = 33..255 ------------------------------------------------------------------------------------------------------------------------

def test_quality_masked_k_above_32(ctx, golden_dir):
    """k = 33..255 with a quality stream, normalised or not: 28S, random mixed-case records, and inverted repeats with and without one masked
    base in the middle; counters + histogram against the literal iterator on the masked records, both routes, the route each launch took."""
    rng = np.random.default_rng(7300)
    cutoff = 40
    recs28 = [r.replace(b"\n", b"").replace(b"\r", b"") for r in fasta_raw_seqs(open(os.path.join(golden_dir, "28S.fasta"), "rb").read())]
    rnd = _records(rng, 60, 0, 900, 0.2, 0.003)
    pal = [b"ACGT" * 80, b"acgt" * 80, b"AT" * 40 + b"at" * 40, b"A" * 300 + b"T" * 300]   # reverse-complement palindromes

    def good(r):
        return rng.integers(cutoff, 75, len(r), dtype=np.uint8).tobytes()

    def with_mid_masked(r):   # one base in the middle of each record below the cutoff
        q = bytearray(good(r))
        if q:
            q[len(q) // 2] = cutoff - 1
        return bytes(q)

    half = rng.integers(0, 4, 32)
    ir64 = bytes(b"ACGT"[x] for x in half) + bytes(b"TGCA"[x] for x in half[::-1])   # a 64-base inverted repeat
    cases = [("28S", recs28, [_phred(rng, len(r), 0.005) for r in recs28]),
             ("random", rnd, [rng.integers(0, 256, len(r), dtype=np.uint8).tobytes() for r in rnd]),
             ("palindromes", pal, [good(r) for r in pal]),
             ("palindromes, middle masked", pal, [with_mid_masked(r) for r in pal]),
             ("inverted repeat", [ir64] * 3, [good(ir64)] * 3),
             ("inverted repeat, middle masked", [ir64] * 3, [with_mid_masked(ir64)] * 3)]
    try:
        for name, recs, quals in cases:
            seq, qual = _batch(recs, quals)
            t, q = to_dev(seq), _qual_dev(qual)
            masked = [O.quality_mask(r, q_, cutoff) for r, q_ in zip(recs, quals)]
            for k in (33, 40, 64, 97, 127, 255):
                for pre, normalized in ((nt.PRE_NONE, False), (nt.PRE_NORMALIZE, True)):
                    want = _wide_reference(masked, k, normalized)
                    for route in (0, NL.ROUTE_NO_SPECULATION):
                        ctx.set_option(NL.OPT_MINIMIZER_ROUTE, route)
                        for launch in ((0, 0), (3, 0)):
                            ctx.set_launch(*launch)
                            ctx.reduce_device(t, len(seq), k, nt.PATH_BYTES_CANONICAL, pre, d_qual=q, quality_cutoff=cutoff, reset=True)
                            got = ctx.accum_read()
                            assert_stats_equal(got, want, (name, k, pre, route, launch))
                            assert got["n_undigested"] == got["n_total"]
                    ctx.set_option(NL.OPT_MINIMIZER_ROUTE, 0)
                    ctx.set_launch(0, 0)
                    redone = 1 if _tie32(masked, k, normalized) or (not normalized and _watch_fires(recs, quals, cutoff)) else 0
                    with redone_launches(ctx) as rl:
                        ctx.reduce_device(t, len(seq), k, nt.PATH_BYTES_CANONICAL, pre, d_qual=q, quality_cutoff=cutoff, reset=True)
                        assert rl.count() == redone, (name, k, pre)
        # the example: a 64-base inverted repeat ties at k = 64; one masked base in its middle leaves no window, so nothing is redone
        assert _tie32([ir64], 64, False)
        with redone_launches(ctx) as rl:
            seq, qual = _batch([ir64], [with_mid_masked(ir64)])
            ctx.reduce_device(to_dev(seq), len(seq), 64, nt.PATH_BYTES_CANONICAL, nt.PRE_NONE, d_qual=_qual_dev(qual), quality_cutoff=cutoff, reset=True)
            assert rl.count() == 0
            assert ctx.accum_read()["n_total"] == 0
    finally:
        ctx.set_launch(0, 0)
        ctx.set_option(NL.OPT_MINIMIZER_ROUTE, 0)


def test_what_stays_an_error(ctx):
    """The quality stream opens the reduce face only: dense values and windowed minimizers on input that was not normalised, and k > 32 with
    w or materialise, keep the status they had."""
    t, q = to_dev(b"ACGT" * 100), _qual_dev(b"I" * 400)
    vals = torch.zeros(512, dtype=torch.int64, device="cuda"); v16 = torch.zeros(64, dtype=torch.int16, device="cuda"); r16 = torch.zeros_like(v16)
    for status, call in ((6, lambda: ctx.reduce_device(t, 400, 21, nt.PATH_BYTES_CANONICAL, nt.PRE_NONE, w=11, d_qual=q, quality_cutoff=40)),
                         (6, lambda: ctx.materialize_device(t, 400, 21, nt.PATH_BYTES_CANONICAL, nt.PRE_NONE, vals, v16, r16, d_qual=q, quality_cutoff=40)),
                         (1, lambda: ctx.reduce_device(t, 400, 33, nt.PATH_BYTES_CANONICAL, nt.PRE_NONE, w=5, d_qual=q, quality_cutoff=40)),
                         (1, lambda: ctx.reduce_device(t, 400, 33, nt.PATH_BYTES_CANONICAL, nt.PRE_NORMALIZE, w=5, d_qual=q, quality_cutoff=40)),
                         (1, lambda: ctx.materialize_device(t, 400, 33, nt.PATH_BYTES_CANONICAL, nt.PRE_NONE, vals, v16, r16, d_qual=q, quality_cutoff=40))):
        with pytest.raises(nt.NtkError) as e:
            call()
        assert e.value.status == status


# ---- the pinned-batch face and the file pipeline --------------------------------------------------------------------------------------

def _chain(recs, k, pre, cutoff):
    """The literal per-record chain: quality_mask -> (strip_returns) -> canonical_kmers."""
    masked = [O.quality_mask(s, q, cutoff) for s, q in recs]
    if k <= 32:
        return O.reduce_records(masked, k, O.PATH_BYTES_CANONICAL, pre)
    if pre == nt.PRE_STRIP_RETURNS:
        masked = [O.strip_returns(s)[0] for s in masked]
    return _wide_reference(masked, k, False)


def _soft_masked_fastq(path, rng, n_rec=400):
    recs = []
    with open(path, "wb") as f:
        for i in range(n_rec):
            n = int(rng.integers(0, 300))
            a = np.frombuffer(b"ACGT", dtype=np.uint8)[rng.integers(0, 4, n)].copy()
            lo = rng.random(n) < 0.15   # soft-masked stretches: lower case in runs
            if n:
                lo = np.convolve(lo, np.ones(6), mode="full")[:n] > 0
            a[lo] |= 0x20
            a[rng.random(n) > 0.995] = ord("N")
            s = a.tobytes()
            q = _phred(rng, n)
            f.write(b"@r%d soft-masked\r\n" % i + s + b"\r\n+\r\n" + q + b"\r\n")
            recs.append((s, q))
    return recs


def test_quality_masked_pipeline_on_raw_bytes(ctx, golden_dir, tmp_path):
    """FASTQ -> parser -> pinned batches carrying the quality lines -> masked scan with PRE_NONE / STRIP_RETURNS and k up to 51, sequential
    and parallel producers, against the literal per-record chain; the reference's FASTQ sample and a soft-masked FASTQ with CR/LF line ends."""
    rng = np.random.default_rng(7400)
    fq = os.path.join(golden_dir, "PRJNA271013_head.fq")
    soft = tmp_path / "soft_masked_crlf.fq"
    soft_recs = _soft_masked_fastq(soft, rng)
    for path in (fq, str(soft)):
        recs = [(r.raw_seq, r.qual.encode()) for r in nt.parse_fastx_file(path)]
        assert len(recs) > 100 and all(len(s) == len(q) for s, q in recs)
        if path == str(soft):
            assert recs == soft_recs   # (the parser drops the CR of each line)
        for k in (21, 51):
            for pre in (nt.PRE_NONE, nt.PRE_STRIP_RETURNS):
                for cutoff in (35, 53):
                    want = _chain(recs, k, pre, cutoff)
                    st = nt.scan_file(ctx, path, k, nt.PATH_BYTES_CANONICAL, pre, batch_bytes=1 << 14, quality_cutoff=cutoff)
                    assert_stats_equal(st, want, (path, k, pre, cutoff))
                    stp = nt.scan_file_parallel(ctx, path, k, nt.PATH_BYTES_CANONICAL, pre, threads=4, batch_bytes=1 << 14, quality_cutoff=cutoff)
                    assert_stats_equal(stp, want, (path, k, pre, cutoff, "parallel"))
    # the batch face directly: ntk_batch_append_quality -> ntk_batch_submit, PRE_NONE, k = 21 and 255
    recs = soft_recs
    for k in (21, 255):
        b = ctx.batch(1 << 20, 4096)
        for s, q in recs:
            assert b.append(s, nt.PRE_NONE, qual=q, quality_cutoff=35)
        ctx.accum_reset()
        b.submit(k, nt.PATH_BYTES_CANONICAL, nt.PRE_NONE, quality_cutoff=35)
        b.wait(); b.release()
        want = _chain(recs, k, nt.PRE_NONE, 35)
        assert want["n_total"] > 0
        assert_stats_equal(ctx.accum_read(), want, ("batch face", k))


# ---- full size ----------------------------------------------------------------------------------------------------------------------------

def test_quality_masked_raw_bytes_full_size(ctx):
    """The config-2 batch (10 M x 150 bp, upper case) with device-random Phred+33 qualities (3 % below Q20) at cutoff 53: at k = 21 PRE_NONE with the quality
    stream equals PRE_NORMALIZE with it and keeps the packed-value scan's result; at k = 64 the two routes agree, normalised or not."""
    n_reads, L = 10_000_000, 150
    nbytes = n_reads * (L + 1)
    t = torch.empty(nbytes + 1024, dtype=torch.uint8, device="cuda")
    ctx.synth_reads_device(0x5EED0002, 0, n_reads, L, 1, t)
    g = torch.Generator(device="cuda"); g.manual_seed(7500)
    q = torch.randint(53, 75, (nbytes + 1024,), dtype=torch.uint8, device="cuda", generator=g)   # Q20 and up, 3 % below
    low = torch.rand(nbytes + 1024, device="cuda", generator=g) < 0.03
    q[low] = torch.randint(33, 53, (int(low.sum()),), dtype=torch.uint8, device="cuda", generator=g)
    path, cutoff = nt.PATH_BYTES_CANONICAL, 53
    try:
        with redone_launches(ctx) as rl:
            ctx.reduce_device(t, nbytes, 21, path, nt.PRE_NONE, d_qual=q, quality_cutoff=cutoff, reset=True)
            assert rl.count() == 0
        ctx.reduce_device(t, nbytes, 21, path, nt.PRE_NONE, d_qual=q, quality_cutoff=cutoff, reset=True)   # (the ctx's own accumulators)
        raw = ctx.accum_read()
        ctx.reduce_device(t, nbytes, 21, path, nt.PRE_NORMALIZE, d_qual=q, quality_cutoff=cutoff, reset=True)
        norm = ctx.accum_read()
        assert_stats_equal(raw, norm, "k = 21, PRE_NONE vs PRE_NORMALIZE")
        ctx.reduce_device(t, nbytes, 21, path, nt.PRE_NORMALIZE, reset=True)
        assert 0 < raw["n_total"] < ctx.accum_read()["n_total"]   # the mask removed k-mers
        ctx.set_option(NL.OPT_MINIMIZER_ROUTE, NL.ROUTE_NO_SPECULATION)
        ctx.reduce_device(t, nbytes, 21, path, nt.PRE_NONE, d_qual=q, quality_cutoff=cutoff, reset=True)
        assert_stats_equal(ctx.accum_read(), raw, "k = 21, direct route")
        got = {}
        for pre in (nt.PRE_NONE, nt.PRE_NORMALIZE):
            for route in (0, NL.ROUTE_NO_SPECULATION):
                ctx.set_option(NL.OPT_MINIMIZER_ROUTE, route)
                ctx.reduce_device(t, nbytes, 64, path, pre, d_qual=q, quality_cutoff=cutoff, reset=True)
                got[(pre, route)] = ctx.accum_read()
        ctx.set_option(NL.OPT_MINIMIZER_ROUTE, 0)
        first = got[(nt.PRE_NONE, 0)]
        assert first["n_total"] > 0 and first["n_undigested"] == first["n_total"]
        for key, st in got.items():
            assert_stats_equal(st, first, ("k = 64", key))
    finally:
        ctx.set_option(NL.OPT_MINIMIZER_ROUTE, 0)
