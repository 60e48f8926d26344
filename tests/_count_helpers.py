"""Helpers of the count-table GPU tests (tests/test_gpu_count.py, tests/test_gpu_count_edges.py) and tools/count_bench.py.

"The oracle's counts": the oracle's literal iterators (bit_kmers_arrays / canonical_kmers_arrays) -> packed values ->
numpy.unique(return_counts=True)."""
import ctypes as C

import numpy as np

import needletail_amd as nt
import oracle as O  # the checker
from needletail_amd import _lib as NL
from needletail_amd import counting

PATH_PRES = [(nt.PATH_BYTES_CANONICAL, p) for p in (nt.PRE_NORMALIZE, nt.PRE_NORMALIZE_IUPAC)] + \
            [(path, p) for path in (nt.PATH_BITS, nt.PATH_BITS_CANONICAL)
             for p in (nt.PRE_NONE, nt.PRE_STRIP_RETURNS, nt.PRE_NORMALIZE, nt.PRE_NORMALIZE_IUPAC)]
CUTOFF = 40
M64 = (1 << 64) - 1

_CODE = np.full(256, 255, dtype=np.uint8)
for _i, _c in enumerate(b"ACGT"):
    _CODE[_c] = _CODE[_c + 32] = _i


def _window_values(codes, starts, k):
    v = np.zeros(len(starts), dtype=np.uint64)
    for i in range(k):
        v = (v << np.uint64(2)) | codes[starts + i].astype(np.uint64)
    return v


def oracle_values(buf: bytes, k: int, path: int, pre: int) -> np.ndarray:
    """Every emitted value of a packed batch (records separated by break bytes) from the oracle's iterators.  Each maximal run of
    base bytes of the mode (ACGTacgt, and U / u after normalize) is a sequence of its own; the runs are laid side by side with an N
    where the other bytes were, so one iterator call covers them all."""
    a = np.frombuffer(buf, dtype=np.uint8)
    accept_u = pre >= nt.PRE_NORMALIZE
    base = _CODE[a] != 255
    isu = (a == ord("U")) | (a == ord("u"))
    if accept_u:
        base |= isu
    runs = np.where(base, a, ord("N")).astype(np.uint8)
    if accept_u:
        runs[isu] = ord("T")
    if path != nt.PATH_BYTES_CANONICAL:
        return O.bit_kmers_arrays(runs.tobytes(), k, path == nt.PATH_BITS_CANONICAL)[1]
    norm = O.normalize(runs.tobytes())[0]
    n = len(norm)
    rc = O.reverse_complement(norm)
    pos, flg = O.canonical_kmers_arrays(norm, rc, k)
    pos = pos.astype(np.int64)
    fw, rv = _CODE[np.frombuffer(norm, dtype=np.uint8)], _CODE[np.frombuffer(rc, dtype=np.uint8)]
    return np.where(flg == 1, _window_values(rv, np.where(flg == 1, n - pos - k, 0), k), _window_values(fw, np.where(flg == 1, 0, pos), k))


def oracle_items(buf, k, path, pre):
    return np.unique(oracle_values(buf, k, path, pre), return_counts=True)


def quality_masked(buf: bytes, qual: np.ndarray, cutoff: int = CUTOFF) -> bytes:
    """QualitySequence::quality_mask on a packed batch: a base byte whose quality is < cutoff becomes N (break bytes stay)."""
    a = np.frombuffer(buf, dtype=np.uint8)
    return np.where((qual < cutoff) & (a != ord("\n")), ord("N"), a).astype(np.uint8).tobytes()


def random_records(seed, n=160):
    """Random records with N runs, U / u, IUPAC letters and lower case."""
    rng = np.random.default_rng(seed)
    out = []
    for _ in range(n):
        L = int(rng.integers(0, 400))
        r = np.frombuffer(b"ACGT", dtype=np.uint8)[rng.integers(0, 4, L)].copy()
        if L:
            for _ in range(int(rng.integers(0, 4))):
                s = int(rng.integers(0, L))
                r[s:s + int(rng.integers(1, 12))] = ord("N")
            extra = np.frombuffer(b"UuacgtRYKMnSW", dtype=np.uint8)
            m = rng.random(L) < 0.02
            r[m] = extra[rng.integers(0, extra.size, int(m.sum()))]
        if rng.random() < 0.1:   # a low-complexity record: long runs of one key
            r = np.frombuffer(b"ACGT", dtype=np.uint8)[np.full(L, rng.integers(0, 4))].copy()
        out.append(r.tobytes())
    return out


def pack(records):
    return b"".join(r + b"\n" for r in records)


def upload(buf: bytes, fill=ord("\n"), device="cuda"):
    import torch
    n = len(buf)
    t = torch.full(((n + 15) // 16 * 16 + 64,), fill, dtype=torch.uint8, device=device)
    if n:
        t[:n] = torch.from_numpy(np.frombuffer(buf, dtype=np.uint8).copy()).to(t.device)
    torch.cuda.synchronize(t.device)
    return t


def assert_items(table, want, what):
    keys, counts = table.items()
    assert np.array_equal(keys, want[0]) and np.array_equal(counts, want[1].astype(np.uint64)), what
    st = table.stats()
    assert st["n_distinct"] == len(want[0]) and st["n_total"] == int(want[1].sum()) and st["n_dropped"] == 0, (what, st)


def device_items(table, min_count=1):
    """(keys, counts) as device tensors (for tables too large for the host)."""
    import torch
    lib = counting.lib()
    n = C.c_uint64(0)
    rc = lib.ntk_kmer_table_extract_device(table._h, min_count, None, None, 0, C.byref(n))
    assert rc in (0, 5), rc
    keys = torch.empty(max(n.value, 1), dtype=torch.int64, device=f"cuda:{table.ctx.device}")
    counts = torch.empty_like(keys)
    NL.check(lib.ntk_kmer_table_extract_device(table._h, min_count, C.c_void_p(keys.data_ptr()), C.c_void_p(counts.data_ptr()),
                                               n.value, C.byref(n)), "extract")
    return keys[: n.value], counts[: n.value]
