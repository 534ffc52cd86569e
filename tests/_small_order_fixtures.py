"""Registries and requests built from twist points of order 13 (test
infrastructure for tests/test_small_order_keys.py and its GPU counterpart).

Keys k * T13 live in a 13-element group, so partial sums of a fold coincide or
cancel all the time, and the aggregate of any request is known in closed form:
(sum of the set k mod 13) * T13 plus the sum of the set honest keys."""

from __future__ import annotations

from typing import NamedTuple

import numpy as np

from oracle import bn256_oracle as O
from oracle import ref_lib as R
from tests import _fixtures as F

N13 = 40                                        # order-13 entries of the mixed registry
K13 = [(7 * i + 3) % 13 for i in range(N13)]    # 3 10 4 11 5 12 6 0 | 7 1 8 2 9 3 10 4 | ...: infinity at 7, 20, 33
N_MIXED, N_PURE = 64, 32
HONEST_SEED = b"small-order"


class Req(NamedTuple):
    what: str
    off: int
    size: int     # level_size; len(bits) is the bitlen
    bits: tuple


class Registry(NamedTuple):
    n: int
    ks13: list      # multiplier of T13 per entry, None for an honest key
    sks: list       # secret key per entry, None for an order-13 entry
    mult: list      # mult[k] = k * T13 (None at 0)
    reg: bytes

    def part13(self, q: Req) -> int:
        return sum(self.ks13[q.off + i] for i, b in enumerate(q.bits) if b and self.ks13[q.off + i] is not None) % 13

    def honest(self, q: Req) -> list:
        return [q.off + i for i, b in enumerate(q.bits) if b and self.sks[q.off + i] is not None]

    def signature(self, q: Req, msg: bytes) -> bytes:
        """The set honest keys' sum signature; infinity when there is none."""
        idx = self.honest(q)
        if not idx:
            return bytes(64)
        return R.sign(msg, (sum(self.sks[i] for i in idx) % O.ORDER).to_bytes(32, "big"))

    def closed_form(self, q: Req) -> bytes:
        """(sum k_i mod 13) T13 + (honest sum), straight from the group law."""
        idx = self.honest(q)
        pt = self.mult[self.part13(q)]
        if idx:
            pt = O.g2_add(pt, O.g2_mul(O.G2_GEN, sum(self.sks[i] for i in idx) % O.ORDER))
        return O.g2_marshal(pt)


def multiples13() -> list:
    t13 = F.small_order_points()[13]
    return [O.g2_mul(t13, k) for k in range(13)]


def mixed_registry() -> Registry:
    """64 keys: 0..39 are K13[i] * T13 (the infinity key where K13[i] = 0), 40..63 honest."""
    mult = multiples13()
    sks = F.scalars(N_MIXED - N13, seed=HONEST_SEED)
    reg = b"".join(O.g2_marshal(mult[k]) for k in K13) + R.g2_scalar_base(F.scalar_bytes(sks))
    return Registry(N_MIXED, K13 + [None] * len(sks), [None] * N13 + sks, mult, reg)


def pure_registry() -> Registry:
    """32 keys, every one a multiple of T13."""
    mult = multiples13()
    ks = K13[:N_PURE]
    return Registry(N_PURE, list(ks), [None] * N_PURE, mult, b"".join(O.g2_marshal(mult[k]) for k in ks))


def window_subset(ks, target: int, avoid_full: bool = True):
    """The first (in counting order) non-empty subset of the 8 multipliers ks
    whose sum is target mod 13, as 8 bits."""
    for s in range(1, 255 if avoid_full else 256):
        if sum(k for j, k in enumerate(ks) if (s >> j) & 1) % 13 == target % 13:
            return tuple(bool((s >> j) & 1) for j in range(8))
    raise AssertionError("no subset of %r sums to %d" % (ks, target))


def _bits(n, idx) -> tuple:
    s = set(idx)
    return tuple(i in s for i in range(n))


def _half(rng, n) -> tuple:
    b = rng.random(n) < 0.5
    b[int(rng.integers(n))] = True  # never empty
    return tuple(bool(x) for x in b)


def _windows(ks, first, targets) -> tuple:
    """Consecutive 8-key windows from window `first`, window j's set keys summing to targets[j] mod 13."""
    out = ()
    for j, t in enumerate(targets):
        w = first + j
        out += window_subset(ks[8 * w:8 * w + 8], t)
    return out


def mixed_requests(seed: int = 13) -> list:
    """The requests on the mixed registry (what each is for is its name)."""
    rng = np.random.default_rng(seed)
    n = N_MIXED
    out = [Req("full range, every bit", 0, n, (True,) * n)]
    # the 40 multipliers sum to 3 mod 13: without key 0 (k = 3) the order-13 part cancels
    for drop in ((0,), (3, 50), (0, 7, 9, 20, 33, 39, 40, 41, 63)):
        out.append(Req("full range minus %d" % len(drop), 0, n, _bits(n, set(range(n)) - set(drop))))
    for size in (8, 16, 32):
        for off in range(0, n, size):
            out.append(Req("block %d+%d, every bit" % (off, size), off, size, (True,) * size))
            out.append(Req("block %d+%d, random half" % (off, size), off, size, _half(rng, size)))
    for off, size in ((5, 40), (33, 20)):
        out.append(Req("unaligned %d+%d, every bit" % (off, size), off, size, (True,) * size))
        out.append(Req("unaligned %d+%d, random half" % (off, size), off, size, _half(rng, size)))
    for w in range(N13 // 8):
        out.append(Req("window %d, zero sum" % w, 8 * w, 8, window_subset(K13[8 * w:8 * w + 8], 0)))
    # window 0 whole and key 9 (k = 1): 51 + 1 = 0 mod 13. One unset window
    # byte against two set ones, so the fold takes the 7 unset keys of window
    # 1 and subtracts them from the block sum, which they equal
    out.append(Req("block minus fold is infinity", 0, 16, _bits(16, list(range(8)) + [9])))
    # one table point per window on one lane: 3 T13, then 10 T13 = -(3 T13)
    out.append(Req("window sum cancels the partial", 0, 16, _bits(16, [0, 14])))
    # four windows with one sum each, and with alternating opposite sums:
    # however the four table points are dealt to lanes, partials meet as
    # equal points (a doubling) or as opposite ones
    out.append(Req("four windows of sum 5", 0, 32, _windows(K13, 0, (5, 5, 5, 5))))
    out.append(Req("four windows of sums 5, -5, 5, -5", 0, 32, _windows(K13, 0, (5, 8, 5, 8))))
    out.append(Req("four windows of sum 3, off the block grid", 8, 32, _windows(K13, 1, (3, 3, 3, 3))))
    out.append(Req("five windows of sum 2, unaligned", 0, 40, _windows(K13, 0, (2, 2, 2, 2, 2))))
    for i in (0, 5, 7, 12, 20, 39, 40):  # 7 and 20 are the infinity key, 40 is honest
        out.append(Req("one key %d" % i, i, 1, (True,)))
    return out


def pure_requests(seed: int = 31) -> list:
    rng = np.random.default_rng(seed)
    n = N_PURE
    ks = K13[:n]
    out = []
    for size in (8, 16, 32):
        for off in range(0, n, size):
            out.append(Req("block %d+%d, every bit" % (off, size), off, size, (True,) * size))
    for _ in range(20):
        out.append(Req("random bitset", 0, n, _half(rng, n)))
    out.append(Req("four windows of sum 5", 0, 32, _windows(ks, 0, (5, 5, 5, 5))))
    out.append(Req("four windows of sums 5, -5, 5, -5", 0, 32, _windows(ks, 0, (5, 8, 5, 8))))
    out.append(Req("four windows of sums 1, 2, 4, 6", 0, 32, _windows(ks, 0, (1, 2, 4, 6))))
    for w in range(n // 8):
        out.append(Req("window %d, zero sum" % w, 8 * w, 8, window_subset(ks[8 * w:8 * w + 8], 0)))
    return out


def pack(reqs):
    """-> (offset, bitlen, level_size, word_offset) tuples and the words array."""
    return F.pack_requests([(q.off, q.size) for q in reqs], [list(q.bits) for q in reqs])


def oracle_aggregate(registry: Registry, reqs, msgs, sigs: bytes, fast: bool = False):
    """The C oracle's codes and aggregate-key bytes, request by request on its
    own message (msgs: one message, or one per request)."""
    if isinstance(msgs, bytes):
        msgs = [msgs] * len(reqs)
    codes, aggs = [], []
    for i, q in enumerate(reqs):
        w = np.array(O.bitset_words(list(q.bits)), dtype=np.uint64)
        c, a = R.verify_aggregate(msgs[i], registry.reg, [q.off], [len(q.bits)], [q.size], w, [0],
                                  sigs[64 * i:64 * i + 64], fast=fast, want_agg=True)
        codes.append(int(c[0]))
        aggs.append(a)
    return codes, b"".join(aggs)


# ---------------------------------------------------------------- single checks
OFF_CURVE_G1 = (1).to_bytes(32, "big") + (1).to_bytes(32, "big")
BATCH_N = 13                       # four waves of four 16-lane teams, the last with one check
BATCH_HONEST = (0, 2, 4, 7, 9)     # valid checks: each shares its wave with an order-13 key
BATCH_ORDER13 = (1, 5, 10, 12)     # order-13 keys whose pairing runs
BATCH_OFF_CURVE_SIG = 8            # an order-13 key whose signature does not decode
BATCH_OTHER = (3, 6, 11)           # T7369, T95797, a large-order point outside G2


def small_order_batch(msgs, seed: bytes = b"small-order-batch"):
    """13 checks (pks, sigs), honest ones interleaved with small-order keys;
    msgs: one message, or one per check (a check's honest signature is made
    on its own message).
       0 honest   1 T13, honest sig       2 honest       3 T7369
       4 honest   5 5 T13, infinity sig   6 T95797       7 honest
       8 T13, off-curve sig   9 honest   10 2 T13, honest sig   11 large-order non-G2
      12 12 T13, honest sig"""
    if isinstance(msgs, bytes):
        msgs = [msgs] * BATCH_N
    pts = F.small_order_points()
    ks = F.scalars(BATCH_N, seed)
    pks = R.g2_scalar_base(F.scalar_bytes(ks))
    pk = [pks[128 * i:128 * i + 128] for i in range(BATCH_N)]
    sg = [R.sign(msgs[i], ks[i].to_bytes(32, "big")) for i in range(BATCH_N)]
    t13 = pts[13]
    for i, k in ((1, 1), (5, 5), (8, 1), (10, 2), (12, 12)):
        pk[i] = O.g2_marshal(O.g2_mul(t13, k))
    sg[5] = bytes(64)
    sg[8] = OFF_CURVE_G1
    pk[3] = O.g2_marshal(pts[7369])
    pk[6] = O.g2_marshal(pts[95797])
    pk[11] = O.g2_marshal(F.non_g2_points(1, seed=5)[0])
    return b"".join(pk), b"".join(sg)
