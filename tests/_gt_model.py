"""The key half of aggregate verification in GT as plain Python
integers: what every GT table entry and every fold value must be, word for
word, and a restatement of the fold's plan that proves which shapes a corpus
reaches (test infrastructure; tests/test_gt_model.py proves the model itself on
the CPU, tests/test_gpu_gt_values.py holds the kernels to it).

Registry keys in the tests are k_i G2Base with known k_i. With
g = FE(Miller(G2Base, H)) (oracle.final_exponentiation_fc) every table value is
g^(sum of the k_i it covers), and the fold's Y is conj(g^K), K the sum over a
request's set bits. Table products are built by the kernels' own recurrences
(one product per entry), never by powers; only the keys and the fold's
expectations are powers of g.
"""

from __future__ import annotations

import functools

import numpy as np

from oracle import bn256_oracle as O

R_MONT = 1 << 286
R_INV = pow(R_MONT, -1, O.P)
LIMB = (1 << 26) - 1
HG_OK, HG_ERR_LEVEL, HG_ERR_EMPTY_AGG = 0, 3, 6
CHUNKS = (1, 2, 3, 8, 13, 16)
MASK64 = (1 << 64) - 1


# ------------------------------------------------------------------ encoding
def _limbs(v):
    m = v * R_MONT % O.P
    return [(m >> (26 * j)) & LIMB for j in range(9)] + [m >> 234]


def fe_words(f) -> np.ndarray:
    """A GT value as the kernels store it: 120 words, element 2k + c of
    coefficient k of w (c = 0: x), ten 26-bit limbs of the Montgomery
    representative each."""
    out = np.zeros((12, 10), dtype=np.uint32)
    for k, (x, y) in enumerate(f):
        out[2 * k] = _limbs(x)
        out[2 * k + 1] = _limbs(y)
    return out.reshape(-1)


def fe_bytes(f) -> np.ndarray:
    """fe_words as the 480 bytes of a Gt."""
    return fe_words(f).view(np.uint8)


def element(words, e) -> int:
    """The integer of element e of an entry's 120 words (any limbs: no reduction)."""
    return sum(int(words[10 * e + j]) << (26 * j) for j in range(10))


def fe_decode(words):
    """The Fp12 value of 120 stored words."""
    v = [element(words, e) * R_INV % O.P for e in range(12)]
    return [(v[2 * k], v[2 * k + 1]) for k in range(6)]


def canonical(words) -> bool:
    """Every limb below 2^26 (the top one included) and every element below p."""
    return all(int(w) <= LIMB for w in words) and all(element(words, e) < O.P for e in range(12))


# ------------------------------------------------------------------ values
@functools.lru_cache(maxsize=None)
def generator_value(msg: bytes):
    """g = FE(Miller(G2Base, H(msg))), as a tuple."""
    h, err = O.hashed_message(msg)
    assert err is None
    return tuple(O.final_exponentiation_fc(O.miller(O.G2_GEN, h)))


def torus_alpha(v):
    """alpha = (1 + a) / b of a unitary v = a + b w, b != 0: three Fp2."""
    a, b = O._f6_from_flat(v, 0), O._f6_from_flat(v, 1)
    a = [O.f2_add(a[0], O.F2_ONE), a[1], a[2]]
    return O._f6_mul(a, O._f6_inv(b))


def torus_words(v) -> np.ndarray:
    """A converted entry: alpha's three Fp2 in elements 0..5, sixty zero words after."""
    al = torus_alpha(v)
    return fe_words(list(al) + [O.F2_ZERO] * 3)


def alpha_plus_w(al, sign=1):
    """alpha + w (sign = -1: alpha - w) as an Fp12 value."""
    one = O.F2_ONE if sign > 0 else O.f2_neg(O.F2_ONE)
    return [al[0], one, al[1], O.F2_ZERO, al[2], O.F2_ZERO]


def skipped(nreg: int, w: int, s: int) -> bool:
    """16-key entry 65536 w + s names none of the registry's keys: the
    conversion leaves it as the Fp12 bytes of 1."""
    have = min(16, nreg - 16 * w)
    return s & ((1 << have) - 1) == 0


class TableModel:
    """The table set of the registry k_i G2Base under g."""

    def __init__(self, ks, g):
        self.ks, self.g, self.nreg = list(ks), list(g), len(ks)
        self.nwin8, self.nwin16 = (self.nreg + 7) // 8, (self.nreg + 15) // 16
        self.levels = 0  # the registry's block levels: ceil(log2 nreg)
        while (1 << self.levels) < self.nreg:
            self.levels += 1
        self.keys = [O.f12_pow(self.g, k) for k in self.ks]
        self._w8 = {}
        self._blk = {}

    def win8(self, w):
        """The 256 subset products of window w: P(s) = P(s without its lowest bit) * key(lowest bit)."""
        if w not in self._w8:
            t = [O.F12_ONE] * 256
            for s in range(1, 256):
                lo = s & -s
                i = 8 * w + lo.bit_length() - 1
                key = self.keys[i] if i < self.nreg else O.F12_ONE
                t[s] = key if s == lo else O.f12_mul(t[s ^ lo], key)
            self._w8[w] = t
        return self._w8[w]

    def win16(self, w, s):
        """Entry 65536 w + s: w8[2w][low byte] * w8[2w + 1][high byte], an absent upper window counting as 1."""
        lo = self.win8(2 * w)[s & 255]
        if 2 * w + 1 >= self.nwin8 or s >> 8 == 0:
            return lo
        hi = self.win8(2 * w + 1)[s >> 8]
        return hi if s & 255 == 0 else O.f12_mul(lo, hi)

    def block_count(self, k):
        return (self.nreg + (1 << k) - 1) >> k

    def block(self, k, j):
        """The product over [j 2^k, (j + 1) 2^k) within the registry, from the level below (level 4 from the
        8-key windows' full entries); an absent partner counts as 1."""
        if (k, j) not in self._blk:
            if k == 4:
                a = self.win8(2 * j)[255]
                v = O.f12_mul(a, self.win8(2 * j + 1)[255]) if 2 * j + 1 < self.nwin8 else a
            else:
                a = self.block(k - 1, 2 * j)
                v = O.f12_mul(a, self.block(k - 1, 2 * j + 1)) if 2 * j + 1 < self.block_count(k - 1) else a
            self._blk[(k, j)] = v
        return self._blk[(k, j)]

    def sum_value(self, idx):
        """g^(sum of k_i over idx): the definition the recurrences are proven against."""
        return O.f12_pow(self.g, sum(self.ks[i] for i in idx) % O.ORDER)


def sampled_subsets(seed: int, extra: int = 4096):
    """The 16-key subsets compared per window: every s whose low or high byte
    is in {0x00, 0x01, 0x80, 0xFF}, plus `extra` from a seeded generator."""
    edge = (0x00, 0x01, 0x80, 0xFF)
    s = {(h << 8) | lo for h in edge for lo in range(256)} | {(h << 8) | lo for h in range(256) for lo in edge}
    rng = np.random.default_rng(seed)
    s |= {int(x) for x in rng.integers(0, 65536, size=extra)}
    return sorted(s)


# ------------------------------------------------------------------ requests, the fold's value and its plan
def request_bits(req, words):
    """The set bits of a request (offset, bitlen, level_size, word_offset) as registry indices."""
    off, bitlen, _, wo = (int(x) for x in req)
    return [off + i for i in range(bitlen) if (int(words[wo + (i >> 6)]) >> (i & 63)) & 1]


def fold_code(req, words, nreg):
    off, bitlen, level_size, _ = (int(x) for x in req)
    if bitlen != level_size or off + bitlen > nreg:
        return HG_ERR_LEVEL
    return HG_OK if request_bits(req, words) else HG_ERR_EMPTY_AGG


def fold_scalar(ks, req, words):
    return sum(ks[i] for i in request_bits(req, words)) % O.ORDER


def fold_value(g, K):
    """Y = conj(g^K)."""
    return O.f12_conj(O.f12_pow(list(g), K))


def _mask_word(req, words, wi, comp):
    _, bitlen, _, wo = (int(x) for x in req)
    if wi < 0 or wi >= (bitlen + 63) // 64:
        return 0
    w = int(words[wo + wi])
    if comp:
        w = ~w & MASK64
    if 64 * wi + 64 > bitlen:
        w &= (1 << (bitlen - 64 * wi)) - 1
    return w


def _rword(req, words, v, comp, W):
    sh = int(req[0]) & (W - 1)
    hi = _mask_word(req, words, v, comp)
    if sh == 0:
        return hi
    return ((hi << sh) & MASK64) | (_mask_word(req, words, v - 1, comp) >> (64 - sh))


def _nz_units(x, W):
    return sum(1 for j in range(64 // W) if (x >> (W * j)) & ((1 << W) - 1))


def fold_plan(req, words, nreg, levels, W, chunk):
    """agg_plan and k_gt_plan's chunk split restated for window width W: aligned, k, comp, m (terms, the block
    term included), chunks, and whether the tail chunk is short (at most half a chunk) or long (None: no tail).
    Proves coverage only; no value assertion depends on it."""
    off, bitlen = int(req[0]), int(req[1])
    nrw = (bitlen + (off & (W - 1)) + 63) // 64
    nzs = sum(_nz_units(_rword(req, words, v, False, W), W) for v in range(nrw))
    nzu = sum(_nz_units(_rword(req, words, v, True, W), W) for v in range(nrw))
    k = 0
    while k < 31 and (1 << k) < bitlen:
        k += 1
    aligned = bitlen > 0 and k <= levels and off & ((1 << k) - 1) == 0 and (bitlen == 1 << k or off + bitlen == nreg)
    comp = aligned and k > 0 and nzu < nzs
    m = (nzu if comp else nzs) + (1 if comp else 0)
    tail = m % chunk
    return {"aligned": aligned, "k": k, "comp": comp, "m": m, "chunks": (m + chunk - 1) // chunk,
            "tail": None if tail == 0 else ("short" if 2 * tail <= chunk else "long")}


# ------------------------------------------------------------------ the fold corpus (224 keys)
FOLD_NREG = 224
# k and r - k in different 16-key windows: no entry is degenerate, the set stays converted
ZERO_PAIRS = ((5, 40), (21, 60), (70, 90), (100, 120), (130, 150), (170, 200))


def fold_scalars(base, degenerate=False):
    """The 224 secret keys: `base` with the zero pairs put in; degenerate: also
    ks[3] = r - ks[2] (one pair inside window 0: the set stays in Fp12 form)."""
    ks = list(base)
    assert len(ks) == FOLD_NREG
    for a, b in ZERO_PAIRS:
        ks[b] = O.ORDER - ks[a]
    if degenerate:
        ks[3] = O.ORDER - ks[2]
    return ks


def _ones(size, unset=()):
    bits = [True] * size
    for i in unset:
        bits[i] = False
    return bits


def _only(size, set_):
    bits = [False] * size
    for i in set_:
        bits[i] = True
    return bits


def fold_corpus():
    """(reqs, words, labels): the requests of the fold tests over 224 keys,
    every request at an odd word offset (a word of ones between requests, which
    no request may read). Labels name the class of each request."""
    n = FOLD_NREG
    rng = np.random.default_rng(224)
    items = [
        # five neighbours of 1, 2, 3, 7 and 8 terms (16-key windows): the padding restore in one wave
        ("one-term", (1, 5), _ones(5)),
        ("two-terms", (10, 12), _ones(12)),
        ("three-terms", (10, 30), _ones(30)),
        ("seven-terms", (1, 110), _ones(110)),
        ("eight-terms", (1, 126), _ones(126)),
        # complemented blocks inside one window: the window-subset term
        ("comp-k1", (6, 2), _ones(2)),
        ("comp-k2", (20, 4), _ones(4)),
        ("comp-k3", (24, 8), _ones(8)),
        # the block table's levels
        ("k4-full", (32, 16), _ones(16)),
        ("k4-unset", (48, 16), _ones(16, (5,))),
        ("k5", (64, 32), _ones(32, (9,))),
        ("k6", (64, 64), _ones(64, (1, 2, 35))),
        ("k7", (0, 128), _ones(128, (7, 100))),
        ("k7-sparse", (0, 128), _only(128, (3, 64))),
        # the clipped last block and the whole registry
        ("clipped", (128, 96), _ones(96, (50,))),
        ("last-k5", (192, 32), _ones(32, (31,))),
        ("full-3-unset", (0, n), _ones(n, (7, 120, n - 1))),
        ("full", (0, n), _ones(n)),
        # off the grid, every window nonzero: exact term counts
        ("nine-terms", (1, 142), _ones(142)),
        ("twelve-terms", (1, 190), _ones(190, range(0, 190, 3))),
        ("thirteen-terms", (1, 206), _ones(206)),
        ("fourteen-terms", (1, 222), _ones(222, range(5, 222, 7))),
        ("alternating", (1, 222), [i % 2 == 0 for i in range(222)]),
        ("alternating-odd", (3, 219), [i % 2 == 1 for i in range(219)]),
        # sets that sum to zero: one pair across two windows, six pairs across twelve windows (two chunks of 8)
        ("zero-two-windows", (1, 60), _only(60, (5 - 1, 40 - 1))),
        ("zero-two-chunks", (1, 222), _only(222, [i - 1 for p in ZERO_PAIRS for i in p])),
        ("zero-aligned", (0, 64), _only(64, (5, 40, 21, 60))),
        # the two error cases: an empty bitset, a range that leaves the registry
        ("empty", (2, 9), [False] * 9),
        ("level-error", (200, 32), _ones(32)),
        ("last-key", (n - 1, 1), _ones(1)),
        ("shift-15", (15, 130), _ones(130, (0, 64, 129))),
        ("shift-9", (57, 97), _ones(97, range(1, 97, 2))),
    ]
    for i in range(9):  # random sets on ranges off every grid
        off = int(rng.integers(1, 100)) | 1
        size = int(rng.integers(65, n - off))
        size += 1 if size % 64 == 0 else 0
        bits = [bool(b) for b in rng.random(size) < (0.15 if i % 3 == 0 else 0.7)]
        bits[int(rng.integers(size))] = True
        items.append(("random", (off, size), bits))
    reqs, words, labels = [], [], []
    for label, (off, size), bits in items:
        if len(words) % 2 == 0:
            words.append(MASK64)
        assert size == len(bits)
        reqs.append((off, size, size, len(words)))
        words.extend(O.bitset_words(bits))
        labels.append(label)
    return reqs, np.array(words, dtype=np.uint64), labels


# ------------------------------------------------------------------ the table registries (17, 25, 33 keys)
TABLE_REGISTRIES = (17, 25, 33)


def table_scalars(base, degenerate):
    """A table registry's secret keys: `base`, and with degenerate also
    ks[3] = r - ks[2] (a window-0 subset sums to zero, so the scan keeps the
    whole set in Fp12 form): the 33-key registry is always built that way, the
    17- and 25-key ones as the Fp12 twin of their converted set."""
    ks = list(base)
    if degenerate:
        ks[3] = O.ORDER - ks[2]
    return ks


def window_samples(nreg, w):
    """The subsets of 16-key window w the table test compares: sampled_subsets,
    which in a ragged window holds skipped entries (every s with none of the
    window's keys) among them."""
    return sampled_subsets(1600 + 16 * nreg + w)
