"""The model of the compacted de Bruijn graph of a k-mer list (include/needletail_amd_dbg.h): strings, a set of keys and one walk per
unitig.  No directory, no search, no pointer doubling: the oracle of tests/test_dbg_rule.py and tests/test_gpu_dbg.py."""
import numpy as np

TOTALS = ("n_half_edges", "deg_hist", "n_isolated", "n_tips", "n_branching", "n_self", "n_links")
COMP = {"A": "T", "C": "G", "G": "C", "T": "A"}
CODE = {"A": 0, "C": 1, "G": 2, "T": 3}


def rc(s: str) -> str:
    return "".join(COMP[c] for c in reversed(s))


def canon(s: str) -> str:
    r = rc(s)
    return s if s < r else r


def encode(s: str) -> int:
    v = 0
    for c in s:
        v = v << 2 | CODE[c]
    return v


def decode(v: int, k: int) -> str:
    return "".join("ACGT"[(v >> (2 * (k - 1 - j))) & 3] for j in range(k))


def keys_of(seqs, k: int, circular: bool = False) -> np.ndarray:
    """The ascending canonical keys of the k-mers of the sequences (each read around its end when circular)."""
    out = set()
    for s in seqs:
        t = s + s[: k - 1] if circular else s
        for i in range(len(t) - k + 1):
            out.add(encode(canon(t[i:i + k])))
    return np.array(sorted(out), dtype=np.uint64)


def all_canonical(k: int) -> np.ndarray:
    return np.array(sorted({encode(canon(decode(v, k))) for v in range(4 ** k)}), dtype=np.uint64)


class Graph:
    """Everything the library answers for the list `keys` (ascending canonical values) with `counts`."""

    def __init__(self, keys, counts, k: int):
        self.k = k
        self.strings = [decode(int(v), k) for v in keys]
        self.index = {s: i for i, s in enumerate(self.strings)}
        self.counts = [int(c) for c in counts]
        n = len(self.strings)
        self.n = n
        # half-edges: target[(i, side, c)] = (j, side', c') for every set bit
        self.mate = {}
        self.edges = np.zeros(n, dtype=np.uint8)
        for i, s in enumerate(self.strings):
            for side in (0, 1):
                u = s if side == 0 else rc(s)
                for c in range(4):
                    t = u[1:] + "ACGT"[c]
                    y = canon(t)
                    if y in self.index:
                        self.edges[i] |= 1 << (4 * side + c)
                        self.mate[(i, side, c)] = (self.index[y], 1 if t == y else 0, CODE[COMP[u[0]]])
        for he, m in self.mate.items():
            assert self.mate[m] == he, "a bit is set iff its mate's is"
        self.link = {}   # (i, side) -> (j, side')
        for (i, side, c), (j, side2, c2) in self.mate.items():
            if self._nib(i, side) == 1 << c and j != i and bin(self._nib(j, side2)).count("1") == 1:
                self.link[(i, side)] = (j, side2)
        for a, b in self.link.items():
            assert self.link[b] == a, "links pair up"
        self._walk()

    def _nib(self, i, side):
        return (int(self.edges[i]) >> (4 * side)) & 15

    def totals(self) -> dict:
        pop = lambda v: bin(v).count("1")
        hist = np.zeros((5, 5), dtype=np.uint64)
        for i in range(self.n):
            hist[pop(self._nib(i, 0)), pop(self._nib(i, 1))] += 1
        a, b = np.meshgrid(np.arange(5), np.arange(5), indexing="ij")
        return {"n_half_edges": len(self.mate), "deg_hist": hist, "n_isolated": int(hist[0, 0]),
                "n_tips": int(hist[0, 1:].sum() + hist[1:, 0].sum()), "n_branching": int(hist[(a > 1) | (b > 1)].sum()),
                "n_self": sum(1 for (i, _, _), (j, _, _) in self.mate.items() if i == j), "n_links": len(self.link)}

    def _follow(self, i, out):
        """The (k-mer, out side) states from (i, out) on, until the links end or come back to i."""
        states = [(i, out)]
        while (i, out) in self.link:
            j, side2 = self.link[(i, out)]
            i, out = j, 1 - side2
            if i == states[0][0]:
                return states, True
            states.append((i, out))
        return states, False

    def _walk(self):
        n, pop = self.n, lambda v: bin(v).count("1")
        self.kmer_rows = np.zeros((n, 2), dtype=np.uint32)
        rows, spelled, seen = [], [], [False] * n
        for i in range(n):   # ascending key: the first unseen k-mer of a unitig that may start it does
            if seen[i]:
                continue
            has = [(i, 0) in self.link, (i, 1) in self.link]
            if has[0] and has[1]:
                states, cycle = self._follow(i, 0)
                if not cycle:
                    continue   # an inner k-mer of a path: its smaller end comes by itself
            else:
                states, cycle = self._follow(i, 0 if has[0] or not has[1] else 1)
                assert not cycle
                if states[-1][0] < i:
                    continue   # the other end is smaller, and was not seen: cannot happen in ascending order
            u = len(rows)
            for pos, (j, out) in enumerate(states):
                assert not seen[j]
                seen[j] = True
                self.kmer_rows[j] = (u, pos << 1 | out)
            first, last = states[0], states[-1]
            flags = (1 if cycle else 0) | pop(self._nib(first[0], 1 - first[1])) << 8 | pop(self._nib(last[0], last[1])) << 12
            rows.append((i, len(states), sum(self.counts[j] for j, _ in states) & (2 ** 64 - 1), flags))
            orient = [self.strings[j] if out == 0 else rc(self.strings[j]) for j, out in states]
            for a, b in zip(orient, orient[1:]):
                assert a[1:] == b[:-1]
            spelled.append("".join(s[0] for s in orient[:-1]) + orient[-1])
        assert all(seen) and sum(r[1] for r in rows) == n
        self.unitig_rows = np.array(rows, dtype=np.uint64).reshape(-1, 4)
        self.spelled = spelled
        self.n_unitigs = len(rows)
        self.n_bases = sum(len(s) for s in spelled)

    def batch(self):
        """(bytes, offsets) of the spelled unitigs in the device-batch layout: one break byte per record, padded to 16."""
        body = "".join(s + "\n" for s in self.spelled).encode()
        off = np.cumsum([0] + [len(s) + 1 for s in self.spelled]).astype(np.uint64)
        return np.frombuffer(body + b"\n" * (-len(body) % 16), dtype=np.uint8), off


class ArrayGraph:
    """Graph on arrays, for lists of a million keys: the same attributes but `strings`, `mate`, `link` and `spelled`.  Adjacency is a
    binary search for the eight neighbours of every key, the links follow from the edge nibbles, and the walk is a plain loop that
    takes every k-mer once: from the ends of the paths first (the states that lack a link on one side), then around what is left,
    which lies on cycles.  tests/test_dbg_array_model.py holds it to Graph on every small case; it is trusted through that alone.
    walk=False stops after the adjacency and the links: `edges` and `totals()` only."""

    def __init__(self, keys, counts, k: int, walk: bool = True):
        U = np.uint64
        keys = np.ascontiguousarray(keys, dtype=np.uint64)
        self.k, self.n = k, int(keys.size)
        n, mask = self.n, U((1 << (2 * k)) - 1)
        self.keys, self.counts = keys, np.ascontiguousarray(counts, dtype=np.uint64)
        # tgt[side][c], flip[side][c]: the k-mer the half-edge (i, side, c) reaches (-1: none) and the side of that k-mer it enters
        tgt = np.full((2, 4, n), -1, dtype=np.int64)
        flip = np.zeros((2, 4, n), dtype=np.int64)
        if n:
            for side, u in enumerate((keys, _rc_values(keys, k))):
                for c in range(4):
                    t = ((u << U(2)) & mask) | U(c)
                    y = np.minimum(t, _rc_values(t, k))
                    by_value = np.argsort(y)   # ascending queries walk the list once: several times faster than in the keys' order
                    at = np.empty(n, dtype=np.int64)
                    at[by_value] = np.minimum(np.searchsorted(keys, y[by_value]), n - 1)
                    tgt[side, c] = np.where(keys[at] == y, at, -1)
                    flip[side, c] = t == y
        have = tgt >= 0
        self.edges = np.zeros(n, dtype=np.uint8)
        for side in range(2):
            for c in range(4):
                self.edges |= (have[side, c].astype(np.uint8) << np.uint8(4 * side + c))
        self.deg = have.sum(axis=1)                                      # [side, i]
        self.n_self = int((tgt == np.arange(n)[None, None, :]).sum())
        # links: the one half-edge of a side, to another k-mer, entering a side that has one half-edge too
        only = np.argmax(have, axis=1)                                   # [side, i]: the c of the first set bit
        idx = np.arange(n)
        self.link_to = np.full((2, n), -1, dtype=np.int64)               # the state 2 j + side' entered
        for side in range(2):
            j, s2 = tgt[side, only[side], idx], flip[side, only[side], idx]
            ok = (self.deg[side] == 1) & (j != idx) & (j >= 0)
            jj = np.where(ok, j, 0)
            ok &= self.deg[s2, jj] == 1
            self.link_to[side] = np.where(ok, 2 * j + s2, -1)
        if walk:
            self._walk()

    def totals(self) -> dict:
        hist = np.zeros((5, 5), dtype=np.uint64)
        np.add.at(hist, (self.deg[0], self.deg[1]), 1)
        a, b = np.meshgrid(np.arange(5), np.arange(5), indexing="ij")
        return {"n_half_edges": int(self.deg.sum()), "deg_hist": hist, "n_isolated": int(hist[0, 0]),
                "n_tips": int(hist[0, 1:].sum() + hist[1:, 0].sum()), "n_branching": int(hist[(a > 1) | (b > 1)].sum()),
                "n_self": self.n_self, "n_links": int((self.link_to >= 0).sum())}

    def _walk(self):
        n, k = self.n, self.k
        has = self.link_to >= 0                                          # [side, i]
        # the state after (i, out): leave through `out`, enter (j, side'), go on through the other side of j
        nxt = np.where(self.link_to >= 0, self.link_to ^ 1, -1).T.reshape(-1).tolist()   # by state 2 i + out
        seen = (~has[0] & ~has[1]).tolist()                              # a k-mer without a link is a unitig by itself, below
        starts, lengths, cyclic, order = [], [], [], []                  # per unitig; `order`: the states of all of them, in a row
        ends = np.flatnonzero(has[0] != has[1])
        for i, out in zip(ends.tolist(), has[1][ends].tolist()):         # out = 1 only where side 1 has the link
            if seen[i]:
                continue   # the larger end of a path already walked
            d, at = 2 * i + out, len(order)
            while d >= 0:
                seen[d >> 1] = True
                order.append(d)
                d = nxt[d]
            starts.append(i); lengths.append(len(order) - at); cyclic.append(0)
        for i in np.flatnonzero(~np.array(seen, dtype=bool) if n else np.zeros(0, bool)).tolist():
            if seen[i]:
                continue
            d, at = 2 * i, len(order)                                    # ascending: i is the cycle's smallest k-mer
            while not seen[d >> 1]:
                seen[d >> 1] = True
                order.append(d)
                d = nxt[d]
            assert d == 2 * i, "what no path reaches closes on itself"
            starts.append(i); lengths.append(len(order) - at); cyclic.append(1)
        self.walk_steps = len(order)                                     # passes of the two loops' bodies: one per k-mer with a link
        lone = np.flatnonzero(~has[0] & ~has[1])
        starts = np.concatenate([np.array(starts, dtype=np.int64), lone])
        lengths = np.concatenate([np.array(lengths, dtype=np.int64), np.ones(lone.size, dtype=np.int64)])
        cyclic = np.concatenate([np.array(cyclic, dtype=np.int64), np.zeros(lone.size, dtype=np.int64)])
        first = np.concatenate([[0], np.cumsum(lengths)])[:-1]           # of each unitig in `order`
        order = np.concatenate([np.array(order, dtype=np.int64), 2 * lone])
        assert order.size == n and np.array_equal(np.sort(order >> 1), np.arange(n)), "every k-mer once"
        # unitigs are numbered by their first k-mer, ascending
        by_start = np.argsort(starts, kind="stable")
        starts, lengths, cyclic, first = starts[by_start], lengths[by_start], cyclic[by_start], first[by_start]
        U = len(starts)
        new_first = np.concatenate([[0], np.cumsum(lengths)])[:-1].astype(np.int64)
        take = np.repeat(first - new_first, lengths) + np.arange(n)      # `order` with the unitigs in their final order
        order = order[take]
        unit = np.repeat(np.arange(U), lengths)
        pos = np.arange(n) - np.repeat(new_first, lengths)
        km, out = order >> 1, order & 1
        self.kmer_rows = np.zeros((n, 2), dtype=np.uint32)
        self.kmer_rows[km, 0] = unit
        self.kmer_rows[km, 1] = pos << 1 | out
        sums = np.add.reduceat(self.counts[km], new_first) if U else np.zeros(0, dtype=np.uint64)   # (uint64 sums wrap)
        last = new_first + lengths - 1
        flags = cyclic | self.deg[1 - out[new_first], km[new_first]] << 8 | self.deg[out[last], km[last]] << 12 if U else np.zeros(0, np.int64)
        self.unitig_rows = np.stack([starts.astype(np.uint64), lengths.astype(np.uint64), sums.astype(np.uint64),
                                     flags.astype(np.uint64)], axis=1).reshape(-1, 4)
        self.n_unitigs, self.n_bases = U, int((lengths + k - 1).sum())
        # the spelled batch: the first base of every k-mer as the walk reads it, the whole of a unitig's last one, a break byte
        v = np.where(out == 1, _rc_values(self.keys[km], k), self.keys[km]) if n else np.zeros(0, dtype=np.uint64)
        self._off = np.concatenate([[0], np.cumsum(lengths + k)]).astype(np.uint64)
        text = np.full(int(self._off[-1]) + (-int(self._off[-1]) % 16), ord("\n"), dtype=np.uint8)
        letters = np.frombuffer(b"ACGT", dtype=np.uint8)
        at = self._off[:-1].astype(np.int64)[unit] + pos
        text[at] = letters[((v >> np.uint64(2 * (k - 1))) & np.uint64(3)).astype(np.intp)]
        for j in range(1, k):
            text[at[last] + j] = letters[((v[last] >> np.uint64(2 * (k - 1 - j))) & np.uint64(3)).astype(np.intp)]
        self._text = text

    def batch(self):
        return self._text, self._off


def _rc_values(x, k: int) -> np.ndarray:
    """Reverse complement of packed k-mers (complement = 3 - code; the 2-bit groups reversed)."""
    x = ~np.asarray(x, dtype=np.uint64)
    for shift, m in ((2, 0x3333333333333333), (4, 0x0F0F0F0F0F0F0F0F), (8, 0x00FF00FF00FF00FF), (16, 0x0000FFFF0000FFFF)):
        x = ((x >> np.uint64(shift)) & np.uint64(m)) | ((x & np.uint64(m)) << np.uint64(shift))
    x = (x >> np.uint64(32)) | (x << np.uint64(32))
    return x >> np.uint64(64 - 2 * k)


def kmers_of_codes(codes, k: int) -> np.ndarray:
    """The canonical values of every k-mer of one sequence given as base codes 0 .. 3 (not distinct, in the sequence's order)."""
    codes = np.asarray(codes, dtype=np.uint64)
    m = codes.size - k + 1
    if m <= 0:
        return np.zeros(0, dtype=np.uint64)
    v = np.zeros(m, dtype=np.uint64)
    for j in range(k):
        v = (v << np.uint64(2)) | codes[j:j + m]
    return np.minimum(v, _rc_values(v, k))


# ---- the cases both suites run ----------------------------------------------------------------------------------------------------------

# canonical 3-mers: AAA (a self loop), ACG (targets its own reverse complement), ACA and CAC (linked on both sides: the cycle ACAC), the
# cycles of three AAC - ACA - CAA and AAG - AGA - GAA, and neighbours that make tips and branches of them
UNIVERSE_3 = ("AAA", "AAC", "AAG", "AAT", "ACA", "ACC", "ACG", "AGA", "ATC", "CAC", "CAA", "CCA", "GAA", "TCA")


def universe_keys() -> np.ndarray:
    keys = sorted({encode(canon(s)) for s in UNIVERSE_3})
    assert len(keys) == 14
    return np.array(keys, dtype=np.uint64)


def random_sequence(rng, length: int) -> str:
    return "".join("ACGT"[c] for c in rng.integers(0, 4, length))


def subset_cases(seed: int = 0xDB6):
    """(name, k, keys): random subsets of all canonical 3-mers and 5-mers at densities 0.05 .. 1.0."""
    rng = np.random.default_rng(seed)
    for k in (3, 5):
        full = all_canonical(k)
        for density in (0.05, 0.2, 0.5, 0.8, 1.0):
            for rep in range(3 if density < 1.0 else 1):
                keep = rng.random(full.size) < density if density < 1.0 else np.ones(full.size, bool)
                yield f"k{k}-d{density}-{rep}", k, full[keep]


def sequence_cases(seed: int = 0x5E0):
    """(name, k, keys): the k-mers of random sequences at k = 15 and 31: plain, circularised, with a planted repeat, and n = 0 and 1."""
    rng = np.random.default_rng(seed)
    for k in (15, 31):
        s = random_sequence(rng, 300)
        yield f"k{k}-path", k, keys_of([s], k)
        yield f"k{k}-cycle", k, keys_of([s], k, circular=True)
        rep = random_sequence(rng, 2 * k)
        t = random_sequence(rng, 100) + rep + random_sequence(rng, 100) + rep + random_sequence(rng, 100)
        yield f"k{k}-repeat", k, keys_of([t], k)
        yield f"k{k}-several", k, keys_of([random_sequence(rng, int(L)) for L in rng.integers(k, 80, 12)], k)
        yield f"k{k}-empty", k, np.zeros(0, dtype=np.uint64)
        yield f"k{k}-one", k, keys_of([s[:k]], k)


def counts_for(keys, seed: int = 7) -> np.ndarray:
    """Counts for a list: small ones and, on its first keys, values near 2^64 (the sums wrap)."""
    rng = np.random.default_rng(seed + len(keys))
    c = rng.integers(1, 1000, len(keys)).astype(np.uint64)
    c[:2] = np.uint64(2 ** 64 - 3)
    return c
