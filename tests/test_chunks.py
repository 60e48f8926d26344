"""The chunk geometry of csrc/ntk_chunks.hpp, which every library that materialises a batch piece by piece walks (for_each_chunk of
csrc/ntk_consumer.hpp), compiled here with g++ and swept against a restatement: the chunks tile the batch in order, every chunk after
the first starts a halo early, the halo keeps the batch pointers 16-byte aligned and every window whole, and the scratch holds the
longest chunk."""
import ctypes as C
import os
import re
import subprocess

import pytest

import _count_model as CM

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CHUNKS_HPP = os.path.join(ROOT, "needletail_amd", "csrc", "ntk_chunks.hpp")
CHUNK = CM.CHUNK

KS = (1, 2, 16, 17, 18, 32, 33, 63)
SIZES = (1, 15, 16, 17, CHUNK - 1, CHUNK, CHUNK + 1, CHUNK + 15, CHUNK + 16, CHUNK + 17, CHUNK + 33, 2 * CHUNK, 3 * CHUNK + 12345, 1 << 40)

SHIM = r"""
#include "ntk_chunks.hpp"
extern "C" {
uint64_t chunks_length(void) { return kChunkBases; }
uint64_t chunks_halo(uint32_t k) { return chunk_halo(k); }
uint64_t chunks_bases(uint64_t n_bytes) { return chunk_bases(n_bytes); }
uint64_t chunks_scratch_bases(uint64_t n_bytes, uint32_t k) { return chunk_scratch_bases(n_bytes, k); }
// the walk of for_each_chunk: {start, end, base, len, skip} of every chunk, at most `cap` of them; the number of chunks
uint64_t chunks_walk(uint64_t n_bytes, uint32_t k, uint64_t *out, uint64_t cap)
{
    uint64_t n = 0;
    for (uint64_t start = 0; start < n_bytes; start += kChunkBases, n++) {
        const Chunk c = chunk_at(n_bytes, k, start);
        if (n < cap) { out[5 * n] = c.start; out[5 * n + 1] = c.end; out[5 * n + 2] = c.base; out[5 * n + 3] = c.len(); out[5 * n + 4] = c.skip(); }
    }
    return n;
}
}
"""


@pytest.fixture(scope="module")
def chunks_lib(tmp_path_factory):
    td = tmp_path_factory.mktemp("chunks")
    src, so = td / "shim.cpp", td / "libshim.so"
    src.write_text(SHIM)
    r = subprocess.run(["g++", "-std=c++17", "-O2", "-Wall", "-Werror", "-fPIC", "-shared", "-I" + os.path.dirname(CHUNKS_HPP), "-o", str(so),
                        str(src)], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    lib = C.CDLL(str(so))
    u64, u32 = C.c_uint64, C.c_uint32
    for name, argtypes in (("chunks_length", []), ("chunks_halo", [u32]), ("chunks_bases", [u64]), ("chunks_scratch_bases", [u64, u32]),
                           ("chunks_walk", [u64, u32, C.POINTER(u64), u64])):
        getattr(lib, name).argtypes = argtypes
        getattr(lib, name).restype = u64
    return lib


def test_the_header_is_plain_cpp_and_states_the_models_chunk(chunks_lib):
    text = open(CHUNKS_HPP).read()
    assert not re.search(r"hip/|__device__|__global__|__host__", text), "the chunk header is plain C++"
    assert chunks_lib.chunks_length() == CHUNK


def _round_up16(x):
    return (x + 15) // 16 * 16


@pytest.mark.parametrize("k", KS)
def test_chunks_tile_the_batch_with_whole_windows(chunks_lib, k):
    halo = _round_up16(k - 1)
    assert chunks_lib.chunks_halo(k) == halo
    for n in SIZES:
        want_chunks = (n + CHUNK - 1) // CHUNK
        out = (C.c_uint64 * (5 * want_chunks))()
        assert chunks_lib.chunks_walk(n, k, out, want_chunks) == want_chunks, (k, n)
        assert chunks_lib.chunks_bases(n) == min(n, CHUNK)
        scratch = chunks_lib.chunks_scratch_bases(n, k)
        assert scratch == min(n, CHUNK) + (halo if n > CHUNK else 0), (k, n)
        at = 0
        for i in range(want_chunks):
            start, end, base, length, skip = out[5 * i: 5 * i + 5]
            # the [start, end) ranges tile [0, n_bytes) in order, each at most CHUNK
            assert start == at == i * CHUNK and start < end <= n and end - start <= CHUNK, (k, n, i)
            assert end == min(n, start + CHUNK), (k, n, i)
            at = end
            # base is 0 for the first chunk and start - round_up(k - 1, 16) after it
            assert base == (0 if i == 0 else start - halo), (k, n, i)
            assert length == end - base and skip == start - base, (k, n, i)
            assert base % 16 == 0, (k, n, i)
            # every window that ends in the chunk is whole: k - 1 bytes before its start (the first chunk starts at the batch's first byte)
            assert start - base >= k - 1 or (i == 0 and start == base == 0), (k, n, i)
            assert end - base <= scratch, (k, n, i)
        assert at == n, (k, n)
