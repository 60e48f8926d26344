"""A host model of the sketch-set library (include/needletail_amd_minhash_set.h): the expected block of a compare, built by calling
tests/_minhash_model.py's compare pair by pair (or any other pairwise compare handed in), and the rank rule of
needletail_amd/csrc/ntk_mhset_rank.hpp restated in numpy."""
import numpy as np

import _minhash_model as M

ALL = M.ALL
BLOCK_DEFAULT, BLOCK_MIN, BLOCK_MAX = 1 << 20, 1, 1 << 26
STAGE = 2048
MATRICES = ("n_shared", "n_union", "dot", "norm2_a", "norm2_b")
DTYPES = {"n_shared": np.uint32, "n_union": np.uint32, "dot": np.float64, "norm2_a": np.float64, "norm2_b": np.float64}


def block(rows, cols, num=0, max_hash=ALL, abundance=True, compare=M.compare) -> dict:
    """The matrices and vectors of comparing every (hashes, counts) of `rows` with every one of `cols`.  Without abundance every count
    is 1."""
    out = {name: np.zeros((len(rows), len(cols)), dtype=DTYPES[name]) for name in MATRICES}
    out["n_a"], out["n_b"] = np.zeros(len(rows), dtype=np.uint64), np.zeros(len(cols), dtype=np.uint64)
    for r, (a, ca) in enumerate(rows):
        for c, (b, cb) in enumerate(cols):
            got = compare(a, ca if abundance else None, b, cb if abundance else None, num, max_hash)
            for name in MATRICES:
                out[name][r, c] = got[name]
            out["n_a"][r], out["n_b"][c] = got["n_a"], got["n_b"]
    return out


def rank_rule(a, ca, b, cb, num=0, max_hash=ALL) -> dict:
    """The comparison without a union: element i of A (after the cut) is member i + p - s of the ascending union, p = B's elements
    below it, s = the shared elements among A[0..i); it counts iff num == 0 or that position is below num."""
    a, b = np.asarray(a, dtype=np.uint64), np.asarray(b, dtype=np.uint64)
    na, nb = int(np.searchsorted(a, np.uint64(max_hash), side="right")), int(np.searchsorted(b, np.uint64(max_hash), side="right"))
    a, b = a[:na], b[:nb]
    ca = np.ones(na) if ca is None else np.asarray(ca[:na], dtype=np.uint64).astype(np.float64)
    cb = np.ones(nb) if cb is None else np.asarray(cb[:nb], dtype=np.uint64).astype(np.float64)

    def side(x, cx, y, cy):
        p = np.searchsorted(y, x, side="left")
        shared = np.zeros(x.size, dtype=bool)
        inside = p < y.size
        shared[inside] = y[p[inside]] == x[inside]
        s = np.cumsum(shared) - shared                      # shared elements before i
        position = np.arange(x.size) + p - s
        counted = np.ones(x.size, dtype=bool) if num == 0 else position < num
        both = counted & shared
        dot = float(np.sum(cx[both] * cy[p[both]])) if both.any() else 0.0
        return int(both.sum()), int(shared.sum()), dot, float(np.sum(cx[counted] ** 2))

    n_shared, S, dot, norm2_a = side(a, ca, b, cb)
    norm2_b = side(b, cb, a, ca)[3]
    everything = na + nb - S
    return {"n_a": na, "n_b": nb, "n_shared": n_shared, "n_union": everything if num == 0 else min(num, everything), "dot": dot,
            "norm2_a": norm2_a, "norm2_b": norm2_b}
