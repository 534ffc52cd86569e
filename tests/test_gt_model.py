"""CPU suite: the model tests/test_gpu_gt_values.py holds the GT tables and the
fold to (tests/_gt_model.py) is right, and its corpora reach what they claim.

The model's values against the oracle's pairing itself (Miller loop and final
exponentiation of k G2Base, a two-key sum), its table recurrences against
powers of g, the torus form against its defining identity, the encoder against
its decoder; then, with the restatement of agg_plan and of k_gt_plan's chunk
split, that the fold corpus holds every class of request and gives every chunk
count, tail kind and chunk length the GPU test's chunk values are there for.
"""

import numpy as np
import pytest

from oracle import bn256_oracle as O
from tests import _fixtures as F
from tests import _gt_model as M

MSG = F.LIB_MESSAGE


@pytest.fixture(scope="module")
def g():
    return list(M.generator_value(MSG))


@pytest.fixture(scope="module")
def model17(g):
    return M.TableModel(M.table_scalars(F.scalars(17, seed=b"gt-values-17"), False), g)


def test_bilinearity_against_the_pairing(g):
    """FE(Miller(k G2Base, H)) == g^k for three keys, and the product of two
    keys' values is the value of their sum's key."""
    h, _ = O.hashed_message(MSG)
    ks = F.scalars(3, seed=b"gt-model-bilinear")
    vals = []
    for k in ks:
        v = O.final_exponentiation_fc(O.miller(O.g2_mul(O.G2_GEN, k), h))
        assert v == O.f12_pow(g, k)
        vals.append(v)
    both = O.final_exponentiation_fc(O.miller(O.g2_mul(O.G2_GEN, (ks[0] + ks[2]) % O.ORDER), h))
    assert both == O.f12_mul(vals[0], vals[2])
    assert O.f12_is_one(O.f12_mul(g, O.f12_conj(g))) and not O.f12_is_one(g)
    assert O.f12_is_one(O.f12_pow(g, O.ORDER))


def test_recurrences_equal_powers(model17):
    m = model17
    assert (m.nwin8, m.nwin16, m.levels) == (3, 2, 5)
    for w, s in [(0, 0x01), (0, 0xFF), (0, 0xA5), (1, 0x80), (1, 0x3C), (2, 0x01), (2, 0xFF), (2, 0x00)]:
        idx = [8 * w + j for j in range(8) if s >> j & 1 and 8 * w + j < 17]
        assert m.win8(w)[s] == m.sum_value(idx), (w, hex(s))
    for w, s in [(0, 0xFFFF), (0, 0x8001), (0, 0x0100), (1, 0x0001), (1, 0xFFFF), (1, 0xFFFE), (1, 0x0100)]:
        idx = [16 * w + j for j in range(16) if s >> j & 1 and 16 * w + j < 17]
        assert m.win16(w, s) == m.sum_value(idx), (w, hex(s))
    assert [m.block_count(k) for k in (4, 5)] == [2, 1]
    assert m.block(4, 0) == m.sum_value(range(16)) and m.block(4, 1) == m.keys[16]
    assert m.block(5, 0) == m.sum_value(range(17))


def test_torus_form_and_the_ragged_rule(model17):
    m = model17
    for w, s in [(0, 0x0001), (0, 0xFFFF), (0, 0x5A00), (1, 0x0001), (1, 0xABCD)]:
        v = m.win16(w, s)
        al = M.torus_alpha(v)
        assert M.alpha_plus_w(al) == O.f12_mul(v, M.alpha_plus_w(al, -1)), (w, hex(s))  # (alpha + w) == v (alpha - w)
        words = M.torus_words(v)
        assert not words[60:].any() and words[:60].any() and M.canonical(words)
        # the conjugate's alpha is -alpha
        assert M.torus_alpha(O.f12_conj(v)) == [O.f2_neg(c) for c in al]
    # window 1 has one key: every even s is skipped (it names no key) and is 1
    assert all(M.skipped(17, 1, s) == (s % 2 == 0) for s in range(0, 65536, 251))
    assert all(M.skipped(17, 0, s) == (s == 0) for s in range(0, 65536, 251))
    assert O.f12_is_one(m.win16(1, 0xFFFE)) and m.win16(1, 0xFFFF) == m.keys[16]
    assert M.skipped(25, 1, 0xFE00) and not M.skipped(25, 1, 0x0100) and not M.skipped(33, 2, 1)


def test_encoder_round_trip(g):
    rng = np.random.default_rng(5)
    vals = [g, O.F12_ONE, O.f12_conj(g),
            [(int.from_bytes(rng.bytes(32), "big") % O.P, int.from_bytes(rng.bytes(32), "big") % O.P) for _ in range(6)],
            [(O.P - 1, 0), (0, O.P - 1), (1, 1), (O.P - 1, O.P - 1), (0, 0), (2, 3)]]
    for v in vals:
        words = M.fe_words(v)
        assert words.dtype == np.uint32 and words.shape == (120,) and M.canonical(words)
        assert M.fe_decode(words) == [tuple(c) for c in v]
        assert M.fe_bytes(v).tobytes() == words.tobytes() and len(M.fe_bytes(v)) == 480
    # the stored one: R mod p in element 1 (the real part of coefficient 0), zeros elsewhere
    one = M.fe_words(O.F12_ONE)
    assert M.element(one, 1) == M.R_MONT % O.P and not one[:10].any() and not one[20:].any()
    bad = one.copy()
    bad[9] = 1 << 26
    assert not M.canonical(bad)
    bad = one.copy()
    bad[0:10] = [(O.P >> (26 * j)) & M.LIMB for j in range(9)] + [O.P >> 234]
    assert not M.canonical(bad)


@pytest.mark.parametrize("nreg", M.TABLE_REGISTRIES)
def test_sampled_entries_per_window(nreg):
    """How many distinct subsets of its keys each window's sample holds: all of
    them in a window of at most eight keys, more than 5000 in a full window; in
    a ragged window skipped entries are among the sampled."""
    for w in range((nreg + 15) // 16):
        have = min(16, nreg - 16 * w)
        S = M.window_samples(nreg, w)
        assert len(set(S)) == len(S) >= 5000
        distinct = {s & ((1 << have) - 1) for s in S}
        if have <= 9:
            assert len(distinct) == 1 << have  # every subset of the window's keys
        else:
            assert len(distinct) >= 5000
        nskip = sum(M.skipped(nreg, w, s) for s in S)
        assert nskip == 1 if have == 16 else nskip >= 16
        for b in (0x00, 0x01, 0x80, 0xFF):
            assert all(((h << 8) | b) in S and ((b << 8) | h) in S for h in range(256))


# ------------------------------------------------------------------ the fold corpus
@pytest.fixture(scope="module")
def corpus():
    return M.fold_corpus()


def _plans(corpus, W, chunk):
    reqs, words, labels = corpus
    out = {}
    for i, (r, lab) in enumerate(zip(reqs, labels)):
        if M.fold_code(r, words, M.FOLD_NREG) == M.HG_OK:
            out[i] = M.fold_plan(r, words, M.FOLD_NREG, 8, W, chunk)
    return out


def test_corpus_shape(corpus):
    reqs, words, labels = corpus
    n = len(reqs)
    assert n > 16 and n % 16 != 0 and 36 <= n <= 48
    assert all(r[3] % 2 == 1 for r in reqs)  # odd word offsets
    assert all(r[1] % 64 != 0 for r in reqs if r[0] % 16)  # but for the aligned blocks, whose sizes are powers of two
    # ranges longer than 64 bits at offsets off the 16-grid: the shift across words, every shift class odd and even
    shifted = {r[0] % 16 for r in reqs if r[1] > 64 and r[0] % 16}
    assert {1, 15, 9} <= shifted
    # no request reads a neighbour's words: the filler words are all ones and every request's last word is its own
    ends = {r[3] + (r[1] + 63) // 64 for r in reqs}
    assert all(int(words[r[3] - 1]) == M.MASK64 or r[3] in ends for r in reqs)
    codes = [M.fold_code(r, words, M.FOLD_NREG) for r in reqs]
    assert codes.count(M.HG_ERR_LEVEL) == 1 and codes.count(M.HG_ERR_EMPTY_AGG) == 1
    assert labels[codes.index(M.HG_ERR_LEVEL)] == "level-error" and labels[codes.index(M.HG_ERR_EMPTY_AGG)] == "empty"


def test_corpus_holds_every_class(corpus):
    reqs, words, labels = corpus
    p16 = _plans(corpus, 16, 8)
    by = {lab: p16[i] for i, lab in enumerate(labels) if i in p16 and lab != "random"}
    terms = {lab: p["m"] for lab, p in by.items()}
    # the five neighbours of the padding restore, in this order at the head of the batch
    assert labels[:5] == ["one-term", "two-terms", "three-terms", "seven-terms", "eight-terms"]
    assert [terms[lab] for lab in labels[:5]] == [1, 2, 3, 7, 8]
    assert not any(by[lab]["comp"] for lab in labels[:5])
    # complemented blocks inside one window: the window-subset term alone
    for lab, k in (("comp-k1", 1), ("comp-k2", 2), ("comp-k3", 3)):
        assert by[lab]["comp"] and by[lab]["k"] == k and by[lab]["m"] == 1, lab
    # the block table's levels, complemented
    for lab, k in (("k4-full", 4), ("k5", 5), ("k6", 6), ("k7", 7), ("clipped", 7), ("last-k5", 5), ("full-3-unset", 8),
                   ("full", 8)):
        assert by[lab]["comp"] and by[lab]["k"] == k and by[lab]["aligned"], lab
    assert by["k4-full"]["m"] == 1 and by["full"]["m"] == 1 and by["full-3-unset"]["m"] == 4
    # aligned but folded plainly (fewer set windows than unset ones)
    assert by["k7-sparse"]["aligned"] and not by["k7-sparse"]["comp"]
    assert by["k4-unset"]["aligned"] and not by["k4-unset"]["comp"]  # one 16-key window either way
    assert _plans(corpus, 8, 8)[labels.index("k4-unset")]["comp"]    # two 8-key windows against one
    # clipped: offset + bitlen is the registry's end and the block is shorter than 2^k
    c = reqs[labels.index("clipped")]
    assert c[0] + c[1] == M.FOLD_NREG and c[1] < 1 << by["clipped"]["k"]
    f = reqs[labels.index("full")]
    assert (f[0], f[1]) == (0, M.FOLD_NREG) and f[1] < 1 << 8
    # off the grid, every window nonzero
    for lab, m in (("nine-terms", 9), ("twelve-terms", 12), ("thirteen-terms", 13), ("fourteen-terms", 14),
                   ("alternating", 14), ("alternating-odd", 14)):
        assert terms[lab] == m and not by[lab]["aligned"], lab
    # the zero sums: two windows; twelve windows, so two chunks of the default 8; no pair inside one window
    ks = M.fold_scalars(F.scalars(M.FOLD_NREG, seed=b"gt-values-224"))
    for lab in ("zero-two-windows", "zero-two-chunks", "zero-aligned"):
        r = reqs[labels.index(lab)]
        assert M.fold_scalar(ks, r, words) == 0 and M.request_bits(r, words), lab
    assert terms["zero-two-windows"] == 2 and terms["zero-two-chunks"] == 12 and by["zero-two-chunks"]["chunks"] == 2
    assert all(a // 16 != b // 16 for a, b in M.ZERO_PAIRS)
    zero = sum(1 for r in reqs if M.fold_code(r, words, M.FOLD_NREG) == 0 and M.fold_scalar(ks, r, words) == 0)
    assert zero == 3
    # the Fp12 twin differs from the converted registry by one key, which requests name
    kd = M.fold_scalars(F.scalars(M.FOLD_NREG, seed=b"gt-values-224"), degenerate=True)
    assert [i for i in range(M.FOLD_NREG) if ks[i] != kd[i]] == [3] and (kd[2] + kd[3]) % O.ORDER == 0
    # the 8-key fold of the same corpus reaches up to 28 terms
    assert max(p["m"] for p in _plans(corpus, 8, 8).values()) == 28


@pytest.mark.parametrize("W", [16, 8])
def test_chunk_values_reach_every_fold_shape(corpus, W):
    """Over the corpus the chunk values 1, 2, 3, 8, 13, 16 give requests of 1,
    2, 3, 4, 5, 8 and 9 or more chunks (one chunk: finished by the chunk
    kernel; 2: one tree level of k_gt_combine; 3..4: two levels; 5 and more:
    rounds above 1), short and long tails, and chunks longer than the twelve
    terms a team's lanes hold."""
    seen, tails, longest = set(), set(), 0
    per_chunk = {}
    for chunk in M.CHUNKS:
        plans = _plans(corpus, W, chunk)
        counts = {p["chunks"] for p in plans.values()}
        per_chunk[chunk] = counts
        seen |= counts
        tails |= {(chunk, p["tail"]) for p in plans.values()}
        longest = max([longest] + [min(chunk, p["m"]) for p in plans.values()])
    assert {1, 2, 3, 4, 5, 8} <= seen and max(seen) >= 9
    assert 1 in per_chunk[16] and {2, 3, 4, 5} <= per_chunk[3] and max(per_chunk[1]) >= 14
    assert per_chunk[8] >= {1, 2} and (W == 16 or {3, 4} <= per_chunk[8])
    for chunk in (2, 3, 8, 13, 16):
        assert (chunk, "short") in tails, chunk
        # a request of whole chunks (14 sixteen-key windows hold no 16 terms; the 8-key fold does)
        assert (chunk, None) in tails or (chunk, W) == (16, 16), chunk
    for chunk in (3, 8, 13, 16):
        assert (chunk, "long") in tails, chunk
    assert longest >= (14 if W == 16 else 16)
    # every wave of the plan kernel but the last is full, and the batch is not a multiple of it
    assert len(corpus[0]) % 16 not in (0, 1)
