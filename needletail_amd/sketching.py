"""How many distinct k-mers does a batch hold?  ctypes binding of libneedletail_amd_sketch.so (include/needletail_amd_sketch.h).

KmerSketch is a HyperLogLog sketch (2^14 one-byte registers) of the keys a count table of the same k and path would insert, made in a
first pass over the same device batches: sketch -> capacity() -> KmerTable / WideKmerTable -> count.  The capacity is never too small
(five standard errors above the estimate) and at most one doubling too big.  Sketches of several batches, GPUs or processes merge by
element-wise max of their registers.  There is no fallback: without a gfx950 device every call raises; only
estimate_from_registers(), which evaluates registers that travelled, needs none."""
from __future__ import annotations

import ctypes as C
import math
import os

import numpy as np

from . import _lib as L
from .counting import KmerTable, upload_records
from .engine import Context, _ptr, default_context
from .wide_counting import WideKmerTable

LIB_PATH = os.path.join(L._HERE, "libneedletail_amd_sketch.so")
PREFIX = "ntk_kmer_sketch_"

P = 14                        # NTK_SKETCH_P
REGISTERS = 1 << P            # NTK_SKETCH_REGISTERS
MAX_RANK = 64 - P + 1         # NTK_SKETCH_MAX_RANK
SIGMA = 1.04 / math.sqrt(REGISTERS)   # the estimator's relative standard error


class Estimate(C.Structure):
    _fields_ = [("distinct", C.c_double), ("n_windows", C.c_uint64), ("capacity", C.c_uint64), ("zero_registers", C.c_uint32),
                ("k", C.c_uint32), ("path", C.c_uint32)]


_vp, _u64, _u32 = C.c_void_p, C.c_uint64, C.c_uint32
# the calls of the sketch library (after its symbol prefix) and their argument types
CALLS = {
    "create": [_vp, _u32, _u32, C.POINTER(_vp)], "destroy": [_vp], "reset": [_vp],
    "add_device": [_vp, _vp, _vp, _u64, C.POINTER(L.Params)], "registers": [_vp, _vp], "merge": [_vp, _vp, _u64],
    "estimate": [_vp, C.POINTER(Estimate)],
}

# every symbol include/needletail_amd_sketch.h declares
SYMBOLS = [PREFIX + c for c in CALLS]


def lib() -> C.CDLL:
    """The sketch library with its calls typed; loaded once."""
    return L.load(LIB_PATH, PREFIX, CALLS)


def _checked_registers(regs) -> np.ndarray:
    regs = np.ascontiguousarray(regs)
    if regs.dtype != np.uint8 or regs.shape != (REGISTERS,):
        raise L.NtkError(2, f"a sketch is {REGISTERS} uint8 registers, not {regs.dtype}{list(regs.shape)}")   # NTK_ERR_BAD_ARG
    return regs


def estimate_from_registers(regs, n_windows: int, k: int) -> dict:
    """The estimator and the capacity rule of ntk_kmer_sketch_estimate, restated on the host: registers that travelled (merged by
    np.maximum, say) are evaluated without a device.  `n_windows` is the exact number of k-mers behind them."""
    regs = _checked_registers(regs)
    m = float(REGISTERS)
    c = np.bincount(regs, minlength=MAX_RANK + 1)
    if c.size > MAX_RANK + 1:
        raise L.NtkError(2, f"a register above {MAX_RANK}")
    z = 0.0
    for r in range(MAX_RANK, -1, -1):   # every term exact; this order is the definition
        z += math.ldexp(float(c[r]), -r)
    e = 0.7213 / (1.0 + 1.079 / m) * m * m / z
    if e <= 2.5 * m and c[0]:
        e = m * math.log(m / float(c[0]))
    cap = int(math.ceil(e * (1.0 + 5.0 * 1.04 / math.sqrt(m)))) + 8
    cap = min(cap, int(n_windows))
    if k < 32:
        cap = min(cap, 1 << (2 * k))
    return {"distinct": e, "n_windows": int(n_windows), "capacity": max(cap, 1), "zero_registers": int(c[0])}


class KmerSketch(L.Handle):
    """A sketch of the distinct k-mers of `path` (a PATH_* constant): k = 1..32 on any path, k = 33..63 on PATH_BYTES_CANONICAL."""

    _lib, _prefix = staticmethod(lib), PREFIX

    def __init__(self, k: int, path: int, ctx: Context = None):
        self.ctx = ctx if ctx is not None else default_context()
        self.k, self.path = k, path
        self._h = C.c_void_p()
        self._check("create", self.ctx._h, k, path, C.byref(self._h))

    def reset(self):
        self._check("reset", self._h)

    def add_device(self, d_seq, n_bytes: int, pre: int, d_qual=None, quality_cutoff: int = 0):
        """Add the k-mers of a device batch (the layout and rules of CountTable.count_device; async on the context's stream)."""
        p = L.Params(self.k, self.path, pre, L.flags(0, quality_cutoff))
        q = None if d_qual is None else C.c_void_p(_ptr(d_qual))
        self._check("add_device", self._h, C.c_void_p(_ptr(d_seq)), q, n_bytes, C.byref(p))

    def add_records(self, records, pre: int):
        """Pack the records with the batch packer (the route of CountTable.count_records), upload and add them."""
        up = upload_records(self.ctx, records, pre)
        if up is not None:
            self.add_device(up[0], up[1], pre)
            self.ctx.synchronize()

    def registers(self) -> np.ndarray:
        regs = np.zeros(REGISTERS, dtype=np.uint8)
        self._check("registers", self._h, regs.ctypes.data)
        return regs

    def merge(self, other, n_windows: int = None):
        """Fold in another KmerSketch of the same k and path, or bare registers with the exact number of k-mers behind them
        (`n_windows` is required then: the capacity is clamped to the total, which is only safe when the total is complete)."""
        if isinstance(other, KmerSketch):
            if (other.k, other.path) != (self.k, self.path):
                raise L.NtkError(2, "merging sketches of different k or path")
            regs, n_windows = other.registers(), other.estimate()["n_windows"]
        else:
            if n_windows is None:
                raise TypeError("merge(registers, n_windows): n_windows is required with bare registers")
            if other is None:
                raise L.NtkError(2, PREFIX + "merge")
            regs = _checked_registers(other)
        self._check("merge", self._h, regs.ctypes.data, n_windows)

    def estimate(self) -> dict:
        e = Estimate()
        self._check("estimate", self._h, C.byref(e))
        return {name: (float if name == "distinct" else int)(getattr(e, name)) for name, _ in Estimate._fields_}

    def capacity(self) -> int:
        return self.estimate()["capacity"]

    def table(self, ctx: Context = None):
        """A count table for what was sketched: a KmerTable (k <= 32) or WideKmerTable (k >= 33) created with capacity()."""
        cls = KmerTable if self.k <= 32 else WideKmerTable
        return cls(self.k, self.path, self.capacity(), ctx if ctx is not None else self.ctx)
