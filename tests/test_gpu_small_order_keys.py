"""GPU suite: public keys of small order on the twist (go flavor unless said).

x/crypto's G2.Unmarshal accepts them like any twist point; the reference pairs
a key of order 13 to ZERO (tests/test_small_order_keys.py pins that on the
CPU), so such a key makes every check invalid, and keys of order 7369 and
95797 pair to ordinary values. Here the kernels meet them: a zero Miller value
in the final exponentiations and in the split form's batched norm inversion
(k_sig12_ninv's zero guard, with honest checks in the same block), and
registries drawn from the 13-element group, where the G2 fold's partial sums
coincide and cancel at every stage (g2_madd, k_window_sums, k_block_sums,
g2_add_pair, the block complement of k_agg_finish).

Every expectation is the C oracle's or the Python oracle's, check by check and
bit for bit; nothing is compared with another GPU path's output."""

import numpy as np
import pytest

from handel_amd.engine import REQ_DTYPE
from oracle import bn256_oracle as O
from oracle import ref_lib as R
from tests import _fixtures as F
from tests import _small_order_fixtures as S

pytestmark = pytest.mark.gpu

MSG = F.LIB_MESSAGE
HG_OK, SIG_INVALID, SIG_UNMARSHAL, CF_PK_MALFORMED, CF_SIG_MALFORMED = 0, 1, 5, 8, 11


@pytest.fixture(scope="module")
def pts():
    return F.small_order_points()


def _own_messages(n):
    """n distinct messages that hash (about 44 % of all messages are "EOF")."""
    msgs = [m for m in (MSG + b" #%d" % i for i in range(4 * n)) if O.hash_scalar(m)[1] is None][:n]
    assert len(set(msgs)) == n
    return msgs


# ---------------------------------------------------------------- 1. hg_pair
def test_pair_of_small_order_keys_matches_reference_bytes(engine, pts):
    t13 = pts[13]
    g2 = [O.g2_mul(t13, k) for k in (1, 2, 5, 12)] + [pts[7369], O.g2_mul(pts[95797], 2),
                                                       O.g2_mul(O.G2_GEN, 11), F.non_g2_points(1, seed=5)[0]]
    g1 = [O.hashed_message(MSG)[0], O.g1_mul(O.G1_GEN, 7)]
    g1b = b"".join(O.g1_marshal(g1[i % 2]) for i in range(len(g2)))
    g2b = b"".join(O.g2_marshal(q) for q in g2)
    gt, codes = engine.pair(g1b, g2b)
    assert list(codes) == [0] * len(g2)
    for i in range(len(g2)):
        want = R.pair(g1b[64 * i:64 * i + 64], g2b[128 * i:128 * i + 128])
        assert gt[384 * i:384 * i + 384] == want, i
    assert gt[:4 * 384] == bytes(4 * 384)  # the four order-13 rows, literally
    assert all(gt[384 * i:384 * i + 384] != bytes(384) for i in range(4, len(g2)))


# ---------------------------------------------------------------- 2. one-kernel form
def _check_batch_oracle(want):
    """On the oracle's output: what the 13-check batch is meant to mix."""
    want = [int(c) for c in want]
    valid = [i for i, c in enumerate(want) if c == HG_OK]
    assert valid == list(S.BATCH_HONEST) and len(valid) >= 5
    assert all(want[i] == SIG_INVALID for i in S.BATCH_ORDER13 + S.BATCH_OTHER)
    assert want[S.BATCH_OFF_CURVE_SIG] == SIG_UNMARSHAL  # the decode error comes first
    # every valid check shares a wave of four teams with an order-13 key whose pairing runs
    assert all(any(j // 4 == i // 4 for j in S.BATCH_ORDER13) for i in valid)


def test_verify_batch_one_kernel_form(engine):
    pks, sigs = S.small_order_batch(MSG)
    want = R.verify_batch(MSG, pks, sigs, nthreads=4)
    _check_batch_oracle(want)
    assert engine.set_message(MSG) == 0
    engine.set_verify_split(False)
    assert list(engine.verify_batch(pks, sigs)) == list(want)


# ---------------------------------------------------------------- 3. split form
SPLIT_ORDER13 = (0, 100, 101, 255, 256, 299)   # first / last slot of an inversion block, two adjacent, the last check
SPLIT_TAMPERED = (50, 280)                     # one per block
SPLIT_T7369 = 200


@pytest.fixture(scope="module")
def split_batch(pts):
    n = 300
    _, pks, sigs = F.keys_and_sigs(n, msg=MSG, seed=b"small-order-split")
    pks, sigs = bytearray(pks), bytearray(sigs)
    mult = S.multiples13()
    for j, i in enumerate(SPLIT_ORDER13):
        pks[128 * i:128 * i + 128] = O.g2_marshal(mult[1 + (5 * j) % 12])
    pks[128 * SPLIT_T7369:128 * SPLIT_T7369 + 128] = O.g2_marshal(pts[7369])
    g1 = O.g1_marshal(O.G1_GEN)
    for i in SPLIT_TAMPERED:
        sigs[64 * i:64 * i + 64] = R.g1_add(bytes(sigs[64 * i:64 * i + 64]), g1)
    pks, sigs = bytes(pks), bytes(sigs)
    want = R.verify_batch(MSG, pks, sigs, nthreads=8)
    planted = sorted(SPLIT_ORDER13 + SPLIT_TAMPERED + (SPLIT_T7369,))
    # exactly the planted checks are invalid: every other check of both blocks must stay valid
    assert [int(i) for i in np.flatnonzero(want)] == planted
    assert all(want[i] == SIG_INVALID for i in planted)
    return pks, sigs, want


@pytest.mark.parametrize("n", [300, 5, 1], ids=["n300_two_blocks", "n5", "n1_alone"])
def test_verify_batch_split_form_keeps_the_honest_neighbours(engine, split_batch, n):
    """k_verify_ml's Miller value of an order-13 key is zero, so k_sig12_norm
    hands k_sig12_ninv a zero norm: the other checks of its 256-check
    inversion block keep their verdicts."""
    pks, sigs, want = split_batch
    if n == 300:
        idx = list(range(300))
    elif n == 5:
        idx = [1, 2, 100, 3, 4]   # the order-13 key at index 2
    else:
        idx = [255]
    p = b"".join(pks[128 * i:128 * i + 128] for i in idx)
    s = b"".join(sigs[64 * i:64 * i + 64] for i in idx)
    expect = [int(want[i]) for i in idx]
    if n == 5:
        assert expect == [0, 0, 1, 0, 0]
    if n == 1:
        assert expect == [1]
    assert engine.set_message(MSG) == 0
    engine.set_verify_split(True)
    try:
        got = engine.verify_batch(p, s)
    finally:
        engine.set_verify_split(False)
    assert list(got) == expect, [(i, int(g), e) for i, g, e in zip(idx, got, expect) if g != e]


# ---------------------------------------------------------------- 4. per-check messages
@pytest.mark.parametrize("split", [False, True], ids=["one_kernel", "split"])
def test_verify_batch_msgs_each_check_on_its_own_message(engine, split):
    msgs = _own_messages(S.BATCH_N)
    pks, sigs = S.small_order_batch(msgs)
    # the C oracle, once per check with that check's message
    want = [int(R.verify_batch(m, pks[128 * i:128 * i + 128], sigs[64 * i:64 * i + 64])[0])
            for i, m in enumerate(msgs)]
    _check_batch_oracle(want)
    engine.set_verify_split(split)
    try:
        got = engine.verify_batch_msgs(msgs, pks, sigs)
    finally:
        engine.set_verify_split(False)
    assert list(got) == want


# ---------------------------------------------------------------- 5. cf flavor
def test_cf_answers_malformed_point(engine_cf):
    """cloudflare's unmarshal multiplies by the group order, so every
    small-order key is "bn256: malformed point", ahead of a signature error
    on the same check."""
    pks, sigs = S.small_order_batch(MSG)
    rejected = S.BATCH_ORDER13 + S.BATCH_OTHER + (S.BATCH_OFF_CURVE_SIG,)
    for i in range(S.BATCH_N):
        err = O.g2_unmarshal(pks[128 * i:128 * i + 128], "cf")[1]
        assert err == (O.ERR_CF_MALFORMED if i in rejected else None)
    assert O.g1_unmarshal(sigs[64 * S.BATCH_OFF_CURVE_SIG:64 * S.BATCH_OFF_CURVE_SIG + 64], "cf")[1] is not None
    assert engine_cf.set_message(MSG) == 0
    engine_cf.set_verify_split(False)
    got = [int(c) for c in engine_cf.verify_batch(pks, sigs)]
    for i in range(S.BATCH_N):
        if i in rejected:
            assert engine_cf.code_string(got[i]) == O.ERR_CF_MALFORMED, i
        else:
            assert got[i] == HG_OK, i
    # the C restatement names unmarshal failures coarsely (4: the pk)
    want = R.verify_batch(MSG, pks, sigs, nthreads=4, flavor=1)
    assert [4 if c == CF_PK_MALFORMED else c for c in got] == [int(c) for c in want]


def test_cf_registry_load_rejects_exactly_the_order_13_keys(engine_cf):
    registry = S.mixed_registry()
    codes = engine_cf.registry_load(registry.reg)
    for i in range(registry.n):
        err = O.g2_unmarshal(registry.reg[128 * i:128 * i + 128], "cf")[1]
        assert err == (O.ERR_CF_MALFORMED if registry.ks13[i] else None), i  # the infinity key decodes
        if err is None:
            assert codes[i] == HG_OK, i
        else:
            assert engine_cf.code_string(int(codes[i])) == err, i
    assert int(np.count_nonzero(codes)) == sum(1 for k in registry.ks13 if k)


# ---------------------------------------------------------------- 6. order-13 registry through the fold
class _Fold:
    def __init__(self, registry, reqs, sigs):
        self.registry, self.cases, self.sigs = registry, reqs, sigs
        tuples, self.words = S.pack(reqs)
        self.reqs = np.array(tuples, dtype=REQ_DTYPE)
        self.want, self.want_agg = S.oracle_aggregate(registry, reqs, MSG, sigs, fast=False)

    def agg(self, j):
        return self.want_agg[128 * j:128 * j + 128]


@pytest.fixture(scope="module")
def mixed():
    registry = S.mixed_registry()
    reqs = S.mixed_requests()
    f = _Fold(registry, reqs, b"".join(registry.signature(q, MSG) for q in reqs))
    # on the oracle's output, before the GPU is asked
    assert f.want.count(HG_OK) >= 6 and f.want.count(SIG_INVALID) >= 6
    assert set(f.want) == {HG_OK, SIG_INVALID}
    assert sum(f.agg(j) == bytes(128) for j in range(len(reqs))) >= 3
    for j, q in enumerate(reqs):
        assert f.want[j] == (HG_OK if registry.part13(q) == 0 else SIG_INVALID), q.what
    # infinity aggregates with the infinity signature are valid (not the empty-aggregate code)
    assert sum(f.agg(j) == bytes(128) and f.sigs[64 * j:64 * j + 64] == bytes(64) and f.want[j] == HG_OK
               for j in range(len(reqs))) >= 3
    return f


def _load(engine, registry):
    assert list(engine.registry_load(registry.reg)) == [0] * registry.n
    # k_g2_subgroup's scalar multiplication by n walks a 13-cycle for each of them
    assert engine.registry_non_g2() == sum(1 for k in registry.ks13 if k)
    assert engine.set_message(MSG) == 0
    assert engine.prepare_aggregate() == 0
    assert engine.aggregate_tables() == 0  # level 2 is pinned, the registry stays on the G2 fold


def _mismatches(f, codes, agg):
    return [(q.what, int(codes[j]), f.want[j], agg[128 * j:128 * j + 128] == f.agg(j))
            for j, q in enumerate(f.cases) if int(codes[j]) != f.want[j] or agg[128 * j:128 * j + 128] != f.agg(j)]


def test_order_13_registry_aggregates_and_verdicts(engine, mixed):
    _load(engine, mixed.registry)
    codes, agg = engine.verify_aggregate(mixed.reqs, mixed.words, mixed.sigs, want_agg=True)
    assert _mismatches(mixed, codes, agg) == []
    assert list(engine.verify_aggregate(mixed.reqs, mixed.words, mixed.sigs)) == mixed.want


def test_order_13_registry_aggregate_pk(engine, mixed):
    _load(engine, mixed.registry)
    agg, codes = engine.aggregate_pk(mixed.reqs, mixed.words)
    assert list(codes) == [0] * len(mixed.cases)
    assert [q.what for j, q in enumerate(mixed.cases) if agg[128 * j:128 * j + 128] != mixed.agg(j)] == []


def test_order_13_registry_multisig_form(engine, mixed):
    _load(engine, mixed.registry)
    full = [j for j, q in enumerate(mixed.cases) if (q.off, q.size) == (0, mixed.registry.n)]
    assert len(full) == 4 and {mixed.want[j] for j in full} == {HG_OK, SIG_INVALID}
    got = engine.verify_multisig(mixed.reqs["bitlen"][full], mixed.reqs["word_offset"][full], mixed.words,
                                 b"".join(mixed.sigs[64 * j:64 * j + 64] for j in full))
    assert list(got) == [mixed.want[j] for j in full]


def test_order_13_registry_requests_on_two_messages(engine, mixed):
    _load(engine, mixed.registry)
    two = (F.TEST_MESSAGES[0], F.TEST_MESSAGES[1])
    msgs = [two[j % 2] for j in range(len(mixed.cases))]
    sigs = b"".join(mixed.registry.signature(q, m) for q, m in zip(mixed.cases, msgs))
    want, want_agg = S.oracle_aggregate(mixed.registry, mixed.cases, msgs, sigs, fast=False)
    assert want == mixed.want and want_agg == mixed.want_agg  # the same keys, each signature on its message
    codes, agg = engine.verify_aggregate_msgs(msgs, mixed.reqs, mixed.words, sigs, want_agg=True)
    assert _mismatches(mixed, codes, agg) == []


# ---------------------------------------------------------------- 7. nothing but order-13 keys
def test_registry_entirely_of_order_13_multiples(engine):
    """32 multiples of T13: every lane partial, every tree level and every
    window sum of the fold lies in a 13-element set."""
    registry = S.pure_registry()
    reqs = S.pure_requests()
    zero = [q for q in reqs if registry.part13(q) == 0]
    assert len(zero) >= 4
    # every request with the infinity signature, the zero-sum ones with a real one as well
    reqs = reqs + zero
    sigs = bytes(64) * (len(reqs) - len(zero)) + R.sign(MSG, (1).to_bytes(32, "big")) * len(zero)
    f = _Fold(registry, reqs, sigs)
    for j, q in enumerate(reqs):
        r = registry.part13(q)
        assert f.agg(j) == O.g2_marshal(registry.mult[r]) == registry.closed_form(q), q.what
        assert (f.agg(j) == bytes(128)) == (r == 0)
        inf_sig = sigs[64 * j:64 * j + 64] == bytes(64)
        assert f.want[j] == (HG_OK if r == 0 and inf_sig else SIG_INVALID), q.what
    _load(engine, registry)
    codes, agg = engine.verify_aggregate(f.reqs, f.words, sigs, want_agg=True)
    assert _mismatches(f, codes, agg) == []


# ---------------------------------------------------------------- 8. the plugin mirror
def test_plugin_mirror_takes_and_refuses_like_the_reference(pts):
    from handel_amd import bn256 as BN

    t13 = O.g2_marshal(pts[13])
    pk = BN.PublicKey()
    pk.UnmarshalBinary(t13)
    assert pk.MarshalBinary() == t13
    honest = R.sign(MSG, F.scalar_bytes(F.scalars(1, seed=b"plugin")))
    for sig in (honest, bytes(64)):
        assert O.verify_signature(pts[13], MSG, O.g1_unmarshal(sig)[0]) == O.ERR_SIG_INVALID
        err = pk.VerifySignature(MSG, BN.SigBLS(sig))
        assert err is not None and str(err) == O.ERR_SIG_INVALID
    other = BN.PublicKey()
    other.UnmarshalBinary(O.g2_marshal(O.g2_mul(pts[13], 12)))
    assert pk.Combine(other).MarshalBinary() == bytes(128) == O.g2_marshal(O.g2_add(pts[13], O.g2_mul(pts[13], 12)))
