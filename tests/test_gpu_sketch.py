"""The k-mer sketch (include/needletail_amd_sketch.h, needletail_amd.KmerSketch) on a real MI355X.

Truth for the registers: the host model tests/_sketch_model.py applied to the oracle's literal iterators - `oracle_values`
(tests/_count_helpers.py) for k <= 32, the {hi, lo} words of canonical_kmers_arrays (the wide count tests' oracle_items) for k >= 33.
Registers are compared bit for bit, n_windows exactly.  At size the sketch is held against the exact count tables, which the suite
already holds to the oracle."""
import ctypes as C
import math
import os
import re
import subprocess

import numpy as np
import pytest

torch = pytest.importorskip("torch")

import needletail_amd as nt  # noqa: E402
from needletail_amd import _lib as NL  # noqa: E402
from needletail_amd import sketching  # noqa: E402
import _count_model as CM  # noqa: E402
import _sketch_model as S  # noqa: E402
from _count_helpers import CUTOFF, PATH_PRES, oracle_values, pack, quality_masked, random_records, upload  # noqa: E402
from test_gpu_count import _genome_reads  # noqa: E402
from test_gpu_wide_count import oracle_items as wide_oracle_items  # noqa: E402

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden")
KS = (1, 3, 6, 7, 16, 21, 31, 32)
WIDE_KS = (33, 34, 40, 51, 62, 63)
BYTES = nt.PATH_BYTES_CANONICAL
ERR_BAD_K, ERR_BAD_ARG, ERR_UNSUPPORTED = 1, 2, 6


@pytest.fixture(scope="module")
def ctx():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    c = nt.Context(0)
    yield c
    c.close()


def model(buf: bytes, k: int, path: int, pre: int):
    """(registers, n_windows) of a packed batch: the model on the oracle's k-mers."""
    if k <= 32:
        v = oracle_values(buf, k, path, pre)
        return S.registers(v), int(v.size)
    keys, counts = wide_oracle_items(buf, k)
    return S.registers(keys), int(counts.sum())


def assert_sketch(sk, want, what):
    regs, e = sk.registers(), sk.estimate()
    assert regs.dtype == np.uint8 and regs.shape == (S.M,)
    assert np.array_equal(regs, want[0]), (what, int((regs != want[0]).sum()))
    assert e["n_windows"] == want[1], (what, e["n_windows"], want[1])
    # the estimate and the capacity are the model's on these registers (the same double arithmetic; log may differ in the last place)
    m = S.evaluate(want[0], want[1], sk.k)
    assert e["capacity"] == m["capacity"] and e["zero_registers"] == m["zero_registers"], (what, e, m)
    assert e["distinct"] == pytest.approx(m["distinct"], rel=1e-12), what
    assert (e["k"], e["path"]) == (sk.k, sk.path)
    assert sketching.estimate_from_registers(regs, e["n_windows"], sk.k)["capacity"] == e["capacity"]


# ---- 1. exact against the model on the oracle's k-mers -----------------------------------------------------------------------------

def test_random_records_match_the_model(ctx):
    recs = random_records(0x5C0017)
    buf = pack(recs)
    dev = upload(buf)
    rng = np.random.default_rng(7)
    qual = rng.integers(33, 75, len(buf)).astype(np.uint8)
    dq, masked = upload(qual.tobytes(), fill=0xFF), quality_masked(buf, qual)
    for path, pre in PATH_PRES:
        for k in KS:
            with nt.KmerSketch(k, path, ctx) as sk:
                want = model(buf, k, path, pre)
                sk.add_device(dev, len(buf), pre)
                assert_sketch(sk, want, (path, pre, k))
                if k in (7, 21, 32):
                    # the packer route: the same records through ntk_batch_append
                    sk.reset()
                    sk.add_records(recs, pre)
                    assert_sketch(sk, want, ("records", path, pre, k))
                    # a quality stream and a cutoff mask bases as the tables do
                    sk.reset()
                    sk.add_device(dev, len(buf), pre, d_qual=dq, quality_cutoff=CUTOFF)
                    assert_sketch(sk, model(masked, k, path, pre), ("quality", path, pre, k))


def test_random_records_match_the_model_wide(ctx):
    recs = random_records(0x5D0017, 200)
    buf = pack(recs)
    dev = upload(buf)
    rng = np.random.default_rng(8)
    qual = rng.integers(33, 80, len(buf)).astype(np.uint8)
    dq, masked = upload(qual.tobytes(), fill=0xFF), quality_masked(buf, qual)
    for k in WIDE_KS:
        want = model(buf, k, BYTES, nt.PRE_NORMALIZE)
        assert want[1] > 1000
        for pre in (nt.PRE_NORMALIZE, nt.PRE_NORMALIZE_IUPAC):
            with nt.KmerSketch(k, BYTES, ctx) as sk:
                sk.add_device(dev, len(buf), pre)
                assert_sketch(sk, want, (pre, k))
                if pre == nt.PRE_NORMALIZE_IUPAC:
                    sk.reset()
                    sk.add_records(recs, pre)
                    assert_sketch(sk, want, ("records", pre, k))
                elif k in (40, 63):
                    sk.reset()
                    sk.add_device(dev, len(buf), pre, d_qual=dq, quality_cutoff=CUTOFF)
                    assert_sketch(sk, model(masked, k, BYTES, pre), ("quality", k))
                    sk.reset()   # cutoff 0 or no stream: no mask
                    sk.add_device(dev, len(buf), pre, d_qual=dq, quality_cutoff=0)
                    assert_sketch(sk, want, ("no mask", k))


def _records(name):
    return [r.raw_seq for r in nt.parse_fastx_file(os.path.join(GOLDEN, name))]


def _packed(ctx, recs, pre):
    b = nt.Batch(ctx, sum(len(r) for r in recs) + len(recs), len(recs))
    for r in recs:
        assert b.append(r, pre)
    seq, _ = b.buffers()
    buf = seq.tobytes()
    b.release()
    return buf


def test_golden_28s_and_prjna271013(ctx):
    for name in ("28S.fasta", "PRJNA271013_head.fq"):
        recs = _records(name)
        buf = _packed(ctx, recs, nt.PRE_NORMALIZE)
        for k in (4, 21, 31, 51, 63):
            with nt.KmerSketch(k, BYTES, ctx) as sk:
                sk.add_records(recs, nt.PRE_NORMALIZE)
                assert_sketch(sk, model(buf, k, BYTES, nt.PRE_NORMALIZE), (name, k))
        raw = _packed(ctx, recs, nt.PRE_STRIP_RETURNS)
        with nt.KmerSketch(21, nt.PATH_BITS_CANONICAL, ctx) as sk:
            sk.add_records(recs, nt.PRE_STRIP_RETURNS)
            assert_sketch(sk, model(raw, 21, nt.PATH_BITS_CANONICAL, nt.PRE_STRIP_RETURNS), (name, "bits"))
    with nt.KmerSketch(4, nt.PATH_BITS_CANONICAL, ctx) as sk:   # 136 canonical 4-mers, every one present
        sk.add_records(_records("28S.fasta"), nt.PRE_STRIP_RETURNS)
        assert 136 <= sk.capacity() <= 2 * 136


# ---- 2. a function of the key set: order, splits, repeats, reset, merge ---------------------------------------------------------------

def _cuts(buf: bytes, pieces: int):
    """Record-aligned, 16-byte-aligned cut points that split buf into about `pieces` calls."""
    ends = [i + 1 for i in range(len(buf)) if buf[i:i + 1] == b"\n" and (i + 1) % 16 == 0]
    want = [len(buf) * j // pieces for j in range(1, pieces)]
    cuts = sorted({min(ends, key=lambda e: abs(e - w)) for w in want})
    return [0, *cuts, len(buf)]


@pytest.mark.parametrize("k,path,pre", [(11, nt.PATH_BITS_CANONICAL, nt.PRE_NORMALIZE), (21, BYTES, nt.PRE_NORMALIZE),
                                        (45, BYTES, nt.PRE_NORMALIZE)])
def test_order_and_split_invariance(ctx, k, path, pre):
    recs = random_records(0x5C0019, 400)
    buf = pack(recs)
    dev = upload(buf)
    want = model(buf, k, path, pre)
    with nt.KmerSketch(k, path, ctx) as sk:
        sk.add_device(dev, len(buf), pre)
        assert_sketch(sk, want, "one call")
        order = np.random.default_rng(3).permutation(len(recs))
        shuffled = pack([recs[i] for i in order])
        sk.reset()
        assert not sk.registers().any() and sk.estimate()["n_windows"] == 0 and sk.estimate()["capacity"] == 1
        ds = upload(shuffled)
        sk.add_device(ds, len(shuffled), pre)
        assert_sketch(sk, want, "shuffled")
        for pieces in (2, 7):
            cuts = _cuts(buf, pieces)
            assert len(cuts) == pieces + 1
            sk.reset()
            for a, b in zip(cuts[:-1], cuts[1:]):
                sk.add_device(dev.data_ptr() + a, b - a, pre)
            assert_sketch(sk, want, ("pieces", pieces))
        # the same batch again: the registers stay, the windows double
        sk.add_device(dev, len(buf), pre)
        assert_sketch(sk, (want[0], 2 * want[1]), "twice")
        with nt.KmerSketch(k, path, ctx) as other:   # a second sketch on the same bytes: identical
            other.add_device(dev, len(buf), pre)
            assert np.array_equal(other.registers(), want[0])


@pytest.mark.parametrize("k", [21, 51])
def test_merge(ctx, k):
    lib = sketching.lib()
    ra, rb = random_records(0x5C001A, 300), random_records(0x5C001B, 200)
    a, b = pack(ra), pack(rb)
    pre = nt.PRE_NORMALIZE
    want = model(a + b, k, BYTES, pre)
    with nt.KmerSketch(k, BYTES, ctx) as sa, nt.KmerSketch(k, BYTES, ctx) as sb:
        da, db = upload(a), upload(b)   # both stay alive until the sketches have read them (add_device is asynchronous)
        sa.add_device(da, len(a), pre)
        sb.add_device(db, len(b), pre)
        regs_a, n_a = sa.registers(), sa.estimate()["n_windows"]
        sb.merge(regs_a, n_a)                       # bare registers: how a sketch travels
        assert_sketch(sb, want, "registers of A into B")
        assert np.array_equal(np.maximum(regs_a, model(b, k, BYTES, pre)[0]), want[0])
        sb.merge(sa)                                # a sketch object; idempotent on the registers
        assert_sketch(sb, (want[0], want[1] + n_a), "A again")
        host = sketching.estimate_from_registers(want[0], want[1] + n_a, k)
        assert host["capacity"] == sb.capacity() and host["distinct"] == pytest.approx(sb.estimate()["distinct"], rel=1e-12)
        sb.reset()
        sb.merge(regs_a, n_a)
        assert_sketch(sb, (regs_a, n_a), "into an empty sketch")
        # wrong length, wrong type, a register above the cap, NULL: NTK_ERR_BAD_ARG; n_windows is required with bare registers
        for bad in (regs_a[:-1], regs_a.astype(np.uint16), np.full(S.M, S.RANK_MAX + 1, np.uint8)):
            with pytest.raises(nt.NtkError) as e:
                sb.merge(bad, 5)
            assert e.value.status == ERR_BAD_ARG
        with pytest.raises(TypeError):
            sb.merge(regs_a)
        assert lib.ntk_kmer_sketch_merge(sb._h, None, 5) == ERR_BAD_ARG
        assert lib.ntk_kmer_sketch_registers(sb._h, None) == ERR_BAD_ARG and lib.ntk_kmer_sketch_estimate(sb._h, None) == ERR_BAD_ARG
        with nt.KmerSketch(k - 1, BYTES, ctx) as other, pytest.raises(nt.NtkError):
            sb.merge(other)
        assert_sketch(sb, (regs_a, n_a), "unchanged by the refused merges")


# ---- 3. seams -----------------------------------------------------------------------------------------------------------------------

def test_chunk_boundaries_are_taken_once(ctx):
    """A batch of more than 64 MiB (the sketch's chunk) whose records straddle the chunk boundaries, at halos of 0, 16 and 32 bytes:
    n_windows is the reduce face's n_total, and the registers are those of the same batch added in record-aligned pieces that each
    fit one chunk."""
    n_reads, L = 500_000, 150
    nbytes = n_reads * (L + 1)
    assert nbytes > S.CHUNK and S.CHUNK % (L + 1)
    dev = torch.empty(nbytes + 1024, dtype=torch.uint8, device="cuda")
    ctx.synth_reads_device(0x5EED0007, 0, n_reads, L, 2, dev)
    cut = (n_reads // 2) // 16 * 16 * (L + 1)   # a record boundary and a multiple of 16
    assert cut < S.CHUNK and nbytes - cut < S.CHUNK
    for path, pre, k in ((BYTES, nt.PRE_NORMALIZE, 21), (nt.PATH_BITS, nt.PRE_STRIP_RETURNS, 17),
                         (nt.PATH_BITS_CANONICAL, nt.PRE_NONE, 32), (nt.PATH_BITS_CANONICAL, nt.PRE_NORMALIZE, 1)):
        ctx.accum_reset()
        ctx.reduce_device(dev, nbytes, k, path, pre)
        n_total = ctx.accum_read()["n_total"]
        with nt.KmerSketch(k, path, ctx) as sk:
            sk.add_device(dev, nbytes, pre)
            whole, e = sk.registers(), sk.estimate()
            assert e["n_windows"] == n_total, (k, e["n_windows"], n_total)
            sk.reset()
            sk.add_device(dev, cut, pre)
            sk.add_device(dev.data_ptr() + cut, nbytes - cut, pre)
            assert np.array_equal(sk.registers(), whole) and sk.estimate()["n_windows"] == n_total, k
            assert whole.any()


def test_wide_kernel_seams(ctx):
    """A break (record end, N, masked quality) at every offset -k..k around every lane-run seam (64 bytes) of a batch that spans
    three blocks of the wide walker; then readable padding of A past an n_bytes that is not a multiple of 16."""
    rng = np.random.default_rng(0x5EB)
    span = 2 * S.THREADS * S.LANE_RUN + 3 * S.LANE_RUN + 5
    for k in (33, 63):
        with nt.KmerSketch(k, BYTES, ctx) as sk:
            for d in range(-k, k + 1):
                a = np.frombuffer(b"ACGT", dtype=np.uint8)[rng.integers(0, 4, span)].copy()
                at = np.arange(S.LANE_RUN, span, S.LANE_RUN) + d
                at = at[(at >= 0) & (at < span)]
                qual = np.full(span, 60, dtype=np.uint8)
                kind = (d + k) % 3
                if kind == 0:
                    a[at] = ord("\n")
                elif kind == 1:
                    a[at] = ord("N")
                else:
                    qual[at] = 10
                buf = a.tobytes()
                sk.reset()
                dev, dq = upload(buf), upload(qual.tobytes())
                sk.add_device(dev, len(buf), nt.PRE_NORMALIZE, d_qual=dq, quality_cutoff=CUTOFF)
                assert_sketch(sk, model(quality_masked(buf, qual), k, BYTES, nt.PRE_NORMALIZE), ("seam", k, d))
            for n_bytes in (span - 16 * 3 - 1, 100, k, k - 1, 1):
                buf = bytes(a[:n_bytes])
                sk.reset()
                dev = upload(buf, fill=ord("A"))
                sk.add_device(dev, n_bytes, nt.PRE_NORMALIZE)
                assert_sketch(sk, model(buf, k, BYTES, nt.PRE_NORMALIZE), ("padding", k, n_bytes))


# ---- 4. nothing to add, and one key 2^26 times ------------------------------------------------------------------------------------------

@pytest.mark.parametrize("k,path,pre", [(21, nt.PATH_BITS_CANONICAL, nt.PRE_NONE), (21, BYTES, nt.PRE_NORMALIZE), (51, BYTES, nt.PRE_NORMALIZE)])
def test_inputs_without_a_window(ctx, k, path, pre):
    lib = sketching.lib()
    with nt.KmerSketch(k, path, ctx) as sk:
        p = NL.Params(k, path, pre, 0)
        assert lib.ntk_kmer_sketch_add_device(sk._h, None, None, 0, C.byref(p)) == 0           # empty input
        bufs = (b"ACGTACGTAC", b"A" * (k - 1), b"\n" * 1000, b"N" * 300 + b"\n" + b"-" * 77, (b"A" * (k - 1) + b"\n") * 50)
        devs = [upload(buf, fill=ord("A")) for buf in bufs]   # alive until the sketch has read them (add_device is asynchronous)
        for buf, dev in zip(bufs, devs):
            sk.add_device(dev, len(buf), pre)
        e = sk.estimate()
        assert not sk.registers().any() and e["n_windows"] == 0 and e["distinct"] == 0.0 and e["capacity"] == 1
        assert e["zero_registers"] == S.M


@pytest.mark.parametrize("k,path,pre", [(21, nt.PATH_BITS_CANONICAL, nt.PRE_NONE), (51, BYTES, nt.PRE_NORMALIZE)])
def test_one_key_2_26_times(ctx, k, path, pre):
    """One record of 2^26 A: every window is the key AAA...A, so after the first the register's plain read answers (no time is
    asserted).  Exactly one register is non-zero, with the model's rank."""
    n = 1 << 26
    dev = torch.full((n + 1024,), ord("\n"), dtype=torch.uint8, device="cuda")
    dev[:n] = ord("A")
    torch.cuda.synchronize()
    key = np.zeros(1, np.uint64) if k <= 32 else np.zeros((1, 2), np.uint64)
    want = S.registers(key)
    assert int((want != 0).sum()) == 1
    with nt.KmerSketch(k, path, ctx) as sk:
        sk.add_device(dev, n + 1, pre)
        regs, e = sk.registers(), sk.estimate()
        assert np.array_equal(regs, want) and int((regs != 0).sum()) == 1
        assert e["n_windows"] == n - k + 1 and e["zero_registers"] == S.M - 1 and e["capacity"] == 10   # ceil(1.04 x 1.00003) + 8
    del dev
    torch.cuda.empty_cache()


# ---- 5. error rules -----------------------------------------------------------------------------------------------------------------------

def test_error_cases(ctx):
    lib = sketching.lib()
    for k, path, status in ((0, BYTES, ERR_BAD_K), (64, BYTES, ERR_BAD_K), (255, BYTES, ERR_BAD_K), (0, nt.PATH_BITS, ERR_BAD_K),
                            (33, nt.PATH_BITS, ERR_BAD_K), (40, nt.PATH_BITS_CANONICAL, ERR_BAD_K), (64, nt.PATH_BITS, ERR_BAD_K),
                            (21, 3, ERR_BAD_ARG), (40, 3, ERR_BAD_ARG)):
        with pytest.raises(nt.NtkError) as e:
            nt.KmerSketch(k, path, ctx)
        assert e.value.status == status, (k, path)
    h = C.c_void_p()
    assert lib.ntk_kmer_sketch_create(None, 21, BYTES, C.byref(h)) == ERR_BAD_ARG
    assert lib.ntk_kmer_sketch_create(ctx._h, 21, BYTES, None) == ERR_BAD_ARG
    assert lib.ntk_kmer_sketch_reset(None) == ERR_BAD_ARG
    lib.ntk_kmer_sketch_destroy(None)
    for k in (32, 33, 63):   # the ends of both routes exist
        nt.KmerSketch(k, BYTES, ctx).close()
    buf = pack(random_records(0x5C001C, 40))
    dev, dq = upload(buf), upload(bytes(len(buf)))
    for k in (21, 40):
        with nt.KmerSketch(k, BYTES, ctx) as sk:
            def call(p, seq=dev.data_ptr(), qual=None, n=len(buf)):
                return lib.ntk_kmer_sketch_add_device(sk._h, C.c_void_p(seq), None if qual is None else C.c_void_p(qual), n, C.byref(p))
            for pre in (nt.PRE_NONE, nt.PRE_STRIP_RETURNS):   # un-normalised byte-path input
                with pytest.raises(nt.NtkError) as e:
                    sk.add_device(dev, len(buf), pre)
                assert e.value.status == ERR_UNSUPPORTED
            assert call(NL.Params(k, nt.PATH_BITS_CANONICAL, nt.PRE_NORMALIZE, 0)) == ERR_BAD_ARG   # path mismatch
            for kk, flags in ((k + 1, 0), (k, 11), (k, NL.FLAG_RESET), (k, 1 << 20)):   # k mismatch, window bits, reset flag, high bits
                assert call(NL.Params(kk, BYTES, nt.PRE_NORMALIZE, flags)) == ERR_BAD_ARG, (kk, flags)
            assert call(NL.Params(k, BYTES, 4, 0)) == ERR_BAD_ARG   # no such pre
            p = NL.Params(k, BYTES, nt.PRE_NORMALIZE, NL.flags(0, CUTOFF))
            assert call(p, seq=dev.data_ptr() + 8, n=len(buf) - 8) == ERR_BAD_ARG     # misaligned d_seq
            assert call(p, qual=dq.data_ptr() + 4) == ERR_BAD_ARG                      # misaligned d_qual
            assert lib.ntk_kmer_sketch_add_device(sk._h, None, None, len(buf), C.byref(p)) == ERR_BAD_ARG
            assert lib.ntk_kmer_sketch_add_device(sk._h, C.c_void_p(dev.data_ptr()), None, len(buf), None) == ERR_BAD_ARG
            assert lib.ntk_kmer_sketch_add_device(None, C.c_void_p(dev.data_ptr()), None, len(buf), C.byref(p)) == ERR_BAD_ARG
            assert call(p, n=0) == 0
            assert sk.estimate()["n_windows"] == 0 and not sk.registers().any()
    with nt.KmerSketch(21, nt.PATH_BITS, ctx) as sk:   # the bit paths take un-normalised input, as the table does
        sk.add_device(dev, len(buf), nt.PRE_NONE)
        assert sk.estimate()["n_windows"] > 0


# ---- 6. at size, against the exact tables -------------------------------------------------------------------------------------------

def _sized_by_the_sketch(ctx, dev, nbytes, k, path, pre, what):
    """The two-pass recipe on one batch; returns estimate / exact n_distinct."""
    with nt.KmerSketch(k, path, ctx) as sk:
        sk.add_device(dev, nbytes, pre)
        e = sk.estimate()
        with sk.table() as t:
            assert isinstance(t, nt.KmerTable if k <= 32 else nt.WideKmerTable)
            t.count_device(dev, nbytes, pre)
            st = t.stats()
    ratio = e["distinct"] / st["n_distinct"]
    print(f"\nsketch at size [{what}]: estimate {e['distinct']:.0f}, n_distinct {st['n_distinct']}, estimate / n_distinct {ratio:.5f}, "
          f"n_windows {e['n_windows']}, capacity {e['capacity']}, slots {st['slots']} (exact fit {CM.slots_for(st['n_distinct'])}), "
          f"n_dropped {st['n_dropped']}")
    assert st["n_dropped"] == 0 and st["n_total"] == e["n_windows"], (what, st, e)
    assert st["n_distinct"] <= e["capacity"], (what, st, e)
    assert st["slots"] <= 2 * CM.slots_for(st["n_distinct"]), (what, st)
    assert abs(ratio - 1) <= 5 * 1.04 / math.sqrt(S.M), (what, ratio)
    return ratio


def test_config2_batch_sized_by_the_sketch(ctx):
    """BASELINE configs[1]: 10M x 150 bp, k = 21 on the byte path, about 1.27 G distinct keys."""
    n_reads, L = 10_000_000, 150
    nbytes = n_reads * (L + 1)
    dev = torch.empty(nbytes + 1024, dtype=torch.uint8, device="cuda")
    ctx.synth_reads_device(0x5EED0002, 0, n_reads, L, 1, dev)
    _sized_by_the_sketch(ctx, dev, nbytes, 21, BYTES, nt.PRE_NORMALIZE, "config2 k=21")
    del dev
    torch.cuda.empty_cache()


def test_genome_sampled_reads_sized_by_the_sketch(ctx):
    """~300x error-free coverage of a 1 Mb genome (test_genome_sampled_reads_spectrum's reads): 302 M windows, about 1 M distinct."""
    k, path, pre = 21, nt.PATH_BITS_CANONICAL, nt.PRE_STRIP_RETURNS
    buf = _genome_reads(0x6E0E, 1_000_000, 2_000_000)
    dev = torch.from_numpy(buf).cuda()
    torch.cuda.synchronize()
    _sized_by_the_sketch(ctx, dev, buf.size, k, path, pre, "genome k=21")
    del dev
    torch.cuda.empty_cache()


def test_synthetic_reads_sized_by_the_sketch_wide(ctx):
    """1 M x 150 bp synthetic reads (with N) at k = 51: about 100 M nearly all-distinct keys."""
    n_reads, L = 1_000_000, 150
    nbytes = n_reads * (L + 1)
    dev = torch.empty(nbytes + 1024, dtype=torch.uint8, device="cuda")
    ctx.synth_reads_device(0x5EED0002, 0, n_reads, L, 1, dev)
    _sized_by_the_sketch(ctx, dev, nbytes, 51, BYTES, nt.PRE_NORMALIZE, "synthetic k=51")
    del dev
    torch.cuda.empty_cache()


# ---- 7. the CLI ---------------------------------------------------------------------------------------------------------------------------

def test_count_kmers_sizes_its_table_with_the_sketch(ctx):
    exe = os.path.join(ROOT, "examples", "count_kmers")
    assert os.path.exists(exe), "built by __graft_entry__.build()"
    for name in ("28S.fasta", "PRJNA271013_head.fq"):
        path = os.path.join(GOLDEN, name)
        bases = sum(len(r) for r in _records(name))
        for args in (["-k", "21", "-p", "canonical"], ["-k", "51"]):
            r = subprocess.run([exe, *args, "-v", path], capture_output=True, text=True, timeout=120)
            assert r.returncode == 0, r.stderr
            fixed = subprocess.run([exe, *args, "-c", str(bases), path], capture_output=True, text=True, timeout=120)
            assert fixed.returncode == 0, fixed.stderr
            assert r.stdout == fixed.stdout and len(r.stdout.splitlines()) > 1000, (name, args)
            m = re.fullmatch(r"count_kmers: estimate (\d+) n_windows (\d+) capacity (\d+) n_distinct (\d+) slots (\d+) n_dropped (\d+)\n",
                             r.stderr)
            assert m, r.stderr
            est, n_windows, capacity, n_distinct, slots, n_dropped = map(int, m.groups())
            assert n_dropped == 0 and n_distinct == len(r.stdout.splitlines()) and n_distinct <= capacity <= n_windows
            assert slots <= 2 * CM.slots_for(n_distinct), (name, args, slots, n_distinct)
            assert abs(est / n_distinct - 1) <= 5 * 1.04 / math.sqrt(S.M)
