"""Inputs around the tile seams of the k-mer builds of scan2_kernel, shared by the emulator test (test_exact_stride_emu.py) and the device
test (test_gpu_exact_stride.py)."""
import numpy as np


def stride_of(k: int) -> int:
    """Bytes a tile of the k-mer build of k advances by: 1008 for k <= 16 (one halo lane), else 1024 - (k - 1) rounded down to a multiple
    of 4 (ntk_tile.hpp Sv2Geom<K, true>; restated here, the tests hold the library to it)."""
    return 1008 if k <= 16 else (1024 - (k - 1)) & ~3


def seam_inputs(k: int, seed: int = 0):
    """A random 3-tile input of the build of k (the third tile holds the end of the input) and, on it, a break at every offset of
    [stride - 24, stride + 24] around each of the two seams, one at a time; and no break at all.  Yields (tag, bytes)."""
    s = stride_of(k)
    rng = np.random.default_rng(0xE4AC7 + 131 * k + seed)
    base = np.frombuffer(b"ACGT", dtype=np.uint8)[rng.integers(0, 4, 3 * s - 5)].copy()
    yield "none", base.tobytes()
    for seam in (s, 2 * s):
        for d in range(-24, 25):
            a = base.copy()
            a[seam + d] = ord("N")
            yield (seam, d), a.tobytes()
