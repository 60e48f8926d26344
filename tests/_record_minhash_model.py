"""A host model of the per-record MinHash library (include/needletail_amd_record_minhash.h), written from the header's text: record r's
sketch is the MinHash sketch (tests/_minhash_model.py) of the k-mers that record emits on its own (the oracle's iterators on
record + break byte, tests/_count_helpers.oracle_values), n_windows[r] their number, and the result a CSR.  Independent of
needletail_amd/record_minhashing.py; nothing here calls the library under test."""
import numpy as np

import _minhash_model as M
from _count_helpers import CUTOFF, oracle_values, quality_masked

ALLPASS = 4                       # NTK_RECORD_MINHASH_ALLPASS
BUFFER_DEFAULT, BUFFER_MIN, BUFFER_MAX = 1 << 24, 256, 1 << 30
MAX_NUM = 1 << 20


def record_values(record: bytes, k, path, pre, qual=None, cutoff=None):
    """The k-mers record r emits.  qual: its quality bytes (masked at `cutoff` first)."""
    buf = bytes(record) + b"\n"
    if qual is not None:
        buf = quality_masked(buf, np.append(np.asarray(qual, dtype=np.uint8), 0xFF), CUTOFF if cutoff is None else cutoff)
    return oracle_values(buf, k, path, pre)


def csr(values_per_record, num: int = 0, scaled: int = 0):
    """(offsets, n_windows, hashes, counts) of the records' k-mers."""
    sk = [M.sketch(v, num, scaled) for v in values_per_record]
    offsets = np.concatenate([[0], np.cumsum([h.size for h, _ in sk])]).astype(np.uint64)
    windows = np.array([len(v) for v in values_per_record], dtype=np.uint64)
    cat = lambda parts: np.concatenate(parts).astype(np.uint64) if parts else np.zeros(0, dtype=np.uint64)
    return offsets, windows, cat([h for h, _ in sk]), cat([c for _, c in sk])


def sketches(records, k, path, pre, num: int = 0, scaled: int = 0, quals=None, cutoff=None):
    return csr([record_values(r, k, path, pre, None if quals is None else quals[i], cutoff) for i, r in enumerate(records)], num, scaled)


def offsets(records) -> np.ndarray:
    """The packer's offsets of records it copies unchanged: record r = [off[r], off[r + 1]), the last byte its break byte."""
    return np.concatenate([[0], np.cumsum([len(r) + 1 for r in records])]).astype(np.uint64)
