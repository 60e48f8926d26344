"""A host model of the MinHash library (include/needletail_amd_minhash.h): the sketch of a multiset of keys, the merge of two sketches
and the comparison, restated in numpy / plain Python from the header's text.  Independent of needletail_amd/minhashing.py: the tests
compare the two, and hold the device's hashes and counts with array_equal to this model applied to the oracle's k-mers.  The hash is
tests/_sketch_model.py's (the k-mer sketch's)."""
import numpy as np

import _sketch_model as S

ALL = (1 << 64) - 1
XOR = S.XOR                       # NTK_MINHASH_XOR = NTK_SKETCH_XOR
CHUNK = S.CHUNK                   # kChunkBases of ntk_minhash.hip
LANE_RUN, PRIME = S.LANE_RUN, S.PRIME
MAX_NUM = 1 << 20
BUFFER_DEFAULT, BUFFER_MIN, BUFFER_MAX = 1 << 22, 64, 1 << 28

_E = np.zeros(0, dtype=np.uint64)


def max_hash(scaled: int) -> int:
    return ALL // scaled


def cut(u, c, num: int = 0, scaled: int = 0):
    """Sorted distinct hashes with counts, cut by the rule: the first `num`, or those <= max_hash(scaled)."""
    assert (num == 0) != (scaled == 0)
    if num:
        return u[:num].copy(), c[:num].astype(np.uint64)
    keep = u <= np.uint64(max_hash(scaled))
    return u[keep], c[keep].astype(np.uint64)


def sketch(keys, num: int = 0, scaled: int = 0):
    """(hashes, counts) of a multiset of keys: narrow values (1-d) or [hi, lo] rows."""
    keys = np.asarray(keys, dtype=np.uint64)
    if keys.shape[0] == 0:
        return _E.copy(), _E.copy()
    u, c = np.unique(S.hash_keys(keys), return_counts=True)
    return cut(u, c, num, scaled)


def threshold(hashes, num: int = 0, scaled: int = 0) -> int:
    if scaled:
        return max_hash(scaled)
    return int(hashes[num - 1]) if len(hashes) >= num else ALL


def merge(a, b, num: int = 0, scaled: int = 0):
    """Two sketches (hashes, counts) into one: counts of equal hashes add, then the cut."""
    h = np.concatenate([a[0], b[0]])
    c = np.concatenate([a[1], b[1]]).astype(np.uint64)
    if h.size == 0:
        return _E.copy(), _E.copy()
    u, inv = np.unique(h, return_inverse=True)
    s = np.zeros(u.size, dtype=np.uint64)
    np.add.at(s, inv, c)
    return cut(u, s, num, scaled)


def compare(a, ca, b, cb, num: int = 0, max_hash: int = ALL) -> dict:
    """The header's comparison with sets and dicts.  None counts mean 1."""
    da = {int(h): (1 if ca is None else int(ca[i])) for i, h in enumerate(a) if int(h) <= max_hash}
    db = {int(h): (1 if cb is None else int(cb[i])) for i, h in enumerate(b) if int(h) <= max_hash}
    union = sorted(set(da) | set(db))
    if num:
        union = union[:num]
    shared = [h for h in union if h in da and h in db]
    dot = norm2_a = norm2_b = 0.0
    for h in union:                     # ascending hash order
        if h in da and h in db:
            dot += float(da[h]) * float(db[h])
        if h in da:
            norm2_a += float(da[h]) ** 2
        if h in db:
            norm2_b += float(db[h]) ** 2
    return {"n_a": len(da), "n_b": len(db), "n_shared": len(shared), "n_union": len(union), "dot": dot, "norm2_a": norm2_a,
            "norm2_b": norm2_b}
