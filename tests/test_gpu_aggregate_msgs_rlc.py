"""GPU suite of the per-message random linear combination
(hg_verify_aggregate_msgs_rlc, hg_verify_aggregate_msgs_rlc_device,
hg_verify_multisig_msgs_rlc and the probes hg_debug_msgs_rlc_groups,
hg_debug_msgs_rlc_points). The expectation everywhere is the C
oracle called once per request with that request's message, as
tests/test_gpu_aggregate_msgs.py builds it, and hg_verify_aggregate_msgs on the
same batch: the bar is equal codes, request by request, and hg_rlc_stats equal
to the counts the planted errors give.

One 67-key registry per flavor and one pool of 150 valid requests, each on its
own message (lengths around SHA-256's padding boundaries); every batch is a
prefix of the pool with requests replaced: tampered or undecodable signatures,
level errors, empty bitsets, messages that cannot be hashed. The oracle's code
of a request is computed once and kept."""

from typing import NamedTuple

import numpy as np
import pytest

from oracle import bn256_oracle as O
from oracle import ref_lib as R
from tests import _fixtures as F
from tests import _msgs_fixtures as M
from tests import test_gpu_aggregate_msgs as A

pytestmark = pytest.mark.gpu

HG_OK, SIG_INVALID, HASH_EOF, LEVEL, SIG_UNMARSHAL, EMPTY_AGG, MULTI_SIZES = 0, 1, 2, 3, 5, 6, 13
PHASE_VERIFY, PHASE_AGGREGATE, PHASE_SUBMIT = 0, 1, 2  # enum hg_phase
N = 67
POOL = 150
SEED = bytes(range(7, 39))
INFINITY = bytes(64)
G1 = O.g1_marshal(O.G1_GEN)
NEG_G1 = O.g1_marshal(O.g1_neg(O.G1_GEN))
Case = A.Case


@pytest.fixture(scope="module", autouse=True)
def torch_first():
    """torch's HIP runtime before the engines' (the device form moves tensors)."""
    import torch

    if torch.cuda.is_available():
        torch.cuda.set_device(0)
        torch.zeros(1, device="cuda")


def _messages(count, hashes, first_seed):
    out, seed = [], first_seed
    while len(out) < count:
        m = M.message(M.LENGTHS[seed % len(M.LENGTHS)], seed)
        seed += 1
        if M.hashable(m) == hashes and m not in out:
            out.append(m)
    return out


def _pool_cases():
    rng = np.random.default_rng(N)
    ranges = A._level_ranges(N)
    cases = []
    for i, m in enumerate(_messages(POOL, True, 100)):
        o, s = ranges[(3 * i) % len(ranges)]
        bits = rng.random(s) < 0.6
        bits[int(rng.integers(s))] = True
        cases.append(Case("valid", m, o, s, tuple(bool(b) for b in bits), "valid", m, HG_OK))
    assert len({c.msg for c in cases}) == POOL and {len(c.msg) for c in cases} == set(M.LENGTHS)
    return cases


EOF_MSGS = _messages(4, False, 500)


# the planted errors: what replaces a valid request of the pool
def tampered(c):
    return c._replace(what="tampered", sig="tamper", expect=SIG_INVALID)


def undecodable(c):
    return c._replace(what="undecodable", sig="undecodable", expect=SIG_UNMARSHAL)


def level_error(c):
    return c._replace(what="level", off=0, size=16, bits=(True,) * 15, expect=LEVEL)


def empty_bitset(c):
    return c._replace(what="empty", bits=(False,) * len(c.bits), expect=EMPTY_AGG)


def eof_message(c, k=0):
    return c._replace(what="eof", msg=EOF_MSGS[k], expect=HASH_EOF)


class Ctx(NamedTuple):
    eng: object
    ks: list
    reg: bytes
    pool: list
    sigs: bytes  # of the pool


_CODES = {}  # (msg, off, size, bits, sig) -> the oracle's code: both flavors and every test share it


def _oracle(reg, cases, sigs):
    out = []
    for i, c in enumerate(cases):
        sig = sigs[64 * i:64 * i + 64]
        key = (c.msg, c.off, c.size, c.bits, sig)
        if key not in _CODES:
            _CODES[key] = int(A._oracle(reg, [c], sig)[0][0])
        out.append(_CODES[key])
    return np.array(out, dtype=np.int32)


@pytest.fixture(scope="module", params=["go", "cf"])
def ctx(request, torch_first):
    from handel_amd.engine import Engine

    eng = Engine(device=0, flavor=request.param)
    ks = F.scalars(N, seed=b"agg-msgs-%d" % N)
    reg = R.g2_scalar_base(F.scalar_bytes(ks))
    assert not eng.registry_load(reg).any()
    assert eng.registry_non_g2() == 0
    pool = _pool_cases()
    yield Ctx(eng, ks, reg, pool, A._sign(eng, ks, pool))
    eng.close()


def _batch(c, n, planted):
    """The pool's first n requests with planted[i](case) in place of request i:
    (cases, sigs), signed in one launch for the replaced requests."""
    cases = list(c.pool[:n])
    for i, f in planted.items():
        cases[i] = f(cases[i])
    idx = sorted(planted)
    new = A._sign(c.eng, c.ks, [cases[i] for i in idx]) if idx else b""
    sigs = bytearray(c.sigs[:64 * n])
    for j, i in enumerate(idx):
        sigs[64 * i:64 * i + 64] = new[64 * j:64 * j + 64]
    return cases, bytes(sigs)


def _stats(cases, group, failing):
    """(groups with a live member, groups holding a failing live member, live
    members of those groups) from the planted kinds alone."""
    live = [k.expect in (HG_OK, SIG_INVALID) for k in cases]
    groups = failed = rechecked = 0
    for g in range(0, len(cases), group):
        members = range(g, min(len(cases), g + group))
        cnt = sum(live[i] for i in members)
        groups += cnt > 0
        if any(i in failing for i in members):
            failed += 1
            rechecked += cnt
    return groups, failed, rechecked


def _check(c, cases, sigs, group, failing, seed=SEED):
    """rlc codes == exact codes == oracle codes == planted codes, and the statistics."""
    e = c.eng
    want = _oracle(c.reg, cases, sigs)
    assert [int(w) for w in want] == [k.expect for k in cases], [(i, k.what, int(w)) for i, (k, w) in
                                                                   enumerate(zip(cases, want)) if w != k.expect]
    reqs, words = A._pack(cases)
    msgs = [k.msg for k in cases]
    exact = e.verify_aggregate_msgs(msgs, reqs, words, sigs)
    got = e.verify_aggregate_msgs_rlc(msgs, reqs, words, sigs, seed=seed, group=group)
    stats = e.rlc_stats()
    assert np.array_equal(got, exact), [(i, int(g), int(x)) for i, (g, x) in enumerate(zip(got, exact)) if g != x]
    assert np.array_equal(A._fold_cf(e, got, sigs), want)
    assert stats == _stats(cases, group, failing), (stats, _stats(cases, group, failing))
    return got


# ---------------------------------------------------------------- 1. r_i H_i
def test_scaled_points_match_the_oracle(ctx):
    top, full = 1 << 63, (1 << 64) - 1

    def hashing(length, count):  # the first `count` messages of this length that hash
        out, seed = [], 0
        while len(out) < count:
            m = M.message(length, seed)
            seed += 1
            if M.hashable(m):
                out.append(m)
        return out

    # the empty message cannot be hashed: zeros; the others can
    msgs = [b""] + hashing(1, 1) + [m for n in (32, 55, 56, 64, 200) for m in hashing(n, 2)]
    coeffs = [5, 1, full, 1, top, full, 2, 0x0123456789abcdef, top + 1, full, 3, 0xdeadbeefcafef00d]
    assert [len(m) for m in msgs] == [0, 1, 32, 32, 55, 55, 56, 56, 64, 64, 200, 200] and not M.hashable(b"")
    got = ctx.eng.debug_msgs_rlc_points(msgs, coeffs)
    assert got[:64] == bytes(64) and O.hashed_message(b"")[1] is not None
    for i, (m, r) in enumerate(zip(msgs, coeffs)):
        if i:
            h, err = O.hashed_message(m)
            assert err is None
            assert got[64 * i:64 * i + 64] == O.g1_marshal(O.g1_mul(h, r)), (i, len(m), hex(r))
    assert got[64:128] == O.g1_marshal(O.hashed_message(msgs[1])[0])  # the coefficient 1


# ---------------------------------------------------------------- 2. end to end
# (n, group, tampered signatures): a group's first member, a middle member, a
# group's last member, one inside the ragged last group, two in one group
E2E = [
    (1, 1, (0,)),
    (13, 5, (0, 7, 9, 11)),      # groups 0..4, 5..9, 10..12: 7 and 9 share a group
    (70, 64, (0, 30, 63, 66)),   # 0, 30 and 63 share group 0; 66 in the last group of 6
    (150, 4096, (0, 75, 149)),   # one group, every team's chain longer than one
]


@pytest.mark.parametrize("n,group,bad", E2E, ids=["%d-%d" % (n, g) for n, g, _ in E2E])
def test_end_to_end_matches_exact_path_and_oracle(ctx, n, group, bad):
    cases, sigs = _batch(ctx, n, {})
    got = _check(ctx, cases, sigs, group, ())
    assert not got.any()
    cases, sigs = _batch(ctx, n, {i: tampered for i in bad})
    got = _check(ctx, cases, sigs, group, bad)
    assert [i for i in range(n) if got[i] == SIG_INVALID] == list(bad)
    # another seed: the same codes
    _check(ctx, cases, sigs, group, bad, seed=bytes(32))


def test_end_to_end_with_mixed_errors(ctx):
    n, group = 131, 16
    bad = (16, 24, 47, 129)  # first and middle of group 1 (two in one group), last of group 2, the last group of 3
    planted = {i: tampered for i in bad}
    planted.update({3: undecodable, 40: level_error, 41: empty_bitset, 100: eof_message, 17: undecodable,
                    130: level_error})
    cases, sigs = _batch(ctx, n, planted)
    got = _check(ctx, cases, sigs, group, bad)
    assert {int(x) for x in A._fold_cf(ctx.eng, got, sigs)} == {HG_OK, SIG_INVALID, HASH_EOF, LEVEL, SIG_UNMARSHAL,
                                                               EMPTY_AGG}


def test_multisig_form(ctx):
    e = ctx.eng
    full, part = (True,) * N, tuple(i % 3 != 1 for i in range(N))
    msgs = [k.msg for k in ctx.pool[:7]]
    items = [(msgs[0], full, "valid", HG_OK), (msgs[1], part, "tamper", SIG_INVALID), (msgs[2], part, "valid", HG_OK),
             (msgs[3], full[:-1], "valid", MULTI_SIZES), (EOF_MSGS[0], part, "valid", HASH_EOF),
             (msgs[4], part[:-1], "undecodable", SIG_UNMARSHAL), (msgs[5], (False,) * N, "valid", EMPTY_AGG),
             (msgs[6], full, "valid", HG_OK)]
    cases = [Case("multisig", m, 0, N, b, s, m if M.hashable(m) else msgs[0], x) for m, b, s, x in items]
    sigs = A._sign(e, ctx.ks, cases)
    want = _oracle(ctx.reg, cases, sigs)
    want[want == LEVEL] = MULTI_SIZES
    assert [int(w) for w in want] == [x for _, _, _, x in items]
    reqs, words = A._pack(cases)
    exact = e.verify_multisig_msgs([k.msg for k in cases], reqs["bitlen"], reqs["word_offset"], words, sigs)
    got = e.verify_multisig_msgs_rlc([k.msg for k in cases], reqs["bitlen"], reqs["word_offset"], words, sigs,
                                     seed=SEED, group=3)
    assert np.array_equal(got, exact) and np.array_equal(A._fold_cf(e, got, sigs), want)
    # groups {0, 1, 2}, {3, 4, 5}, {6, 7}: the second has no live member
    assert e.rlc_stats() == (2, 1, 3)


# ---------------------------------------------------------------- 3. liveness
def test_liveness(ctx):
    e, n, group = ctx.eng, 40, 8
    planted = {0: undecodable,                                            # the carrier of group 0 is member 1
               9: level_error, 10: empty_bitset, 11: eof_message,        # group 1
               24: undecodable, 25: level_error, 26: empty_bitset, 27: eof_message, 28: undecodable,
               29: lambda k: eof_message(k, 1), 30: level_error, 31: empty_bitset}  # group 3: no live member
    cases, sigs = _batch(ctx, n, planted)
    sigs = bytearray(sigs)
    sigs[64 * 18:64 * 19] = INFINITY  # a live infinity signature on a non-empty set: group 2 fails
    sigs = bytes(sigs)
    cases[18] = cases[18]._replace(what="infinity signature", expect=SIG_INVALID)
    got = _check(ctx, cases, sigs, group, (18,))
    assert e.rlc_stats() == (4, 1, 8)  # the all-dead group is not counted
    assert got[18] == SIG_INVALID and not got[16:18].any() and not got[19:24].any()
    # the same through the probe, with the call's coefficients
    coeffs = [int(x) for x in e.debug_rlc_coeffs(SEED, 0, n)]
    reqs, words = A._pack(cases)
    codes, gcodes, glive = e.debug_msgs_rlc_groups([k.msg for k in cases], reqs, words, sigs, coeffs, group)
    assert list(glive) == [7, 5, 8, 0, 8] and list(gcodes) == [HG_OK, HG_OK, SIG_INVALID, HG_OK, HG_OK]
    # the codes decided before the pairing: the verdicts' places are still HG_OK
    before = np.where(got == SIG_INVALID, HG_OK, got)
    assert np.array_equal(codes, before)


# ---------------------------------------------------------------- 4. secrecy matters
def test_cancelling_pair_needs_secret_coefficients(ctx):
    e, n, group = ctx.eng, 6, 6
    cases, sigs = _batch(ctx, n, {})
    assert cases[0].msg != cases[1].msg
    pair = bytearray(sigs)
    pair[0:64] = R.g1_add(sigs[0:64], G1)          # sig_a + D
    pair[64:128] = R.g1_add(sigs[64:128], NEG_G1)  # sig_b - D
    pair = bytes(pair)
    reqs, words = A._pack(cases)
    msgs = [k.msg for k in cases]
    _, gcodes, glive = e.debug_msgs_rlc_groups(msgs, reqs, words, pair, [1] * n, group)
    assert list(gcodes) == [HG_OK] and list(glive) == [n]  # equal coefficients cannot see it
    _, gcodes, _ = e.debug_msgs_rlc_groups(msgs, reqs, words, pair, [7] * n, group)
    assert list(gcodes) == [HG_OK]
    _, gcodes, _ = e.debug_msgs_rlc_groups(msgs, reqs, words, pair, [1, 2, 1, 1, 1, 1], group)
    assert list(gcodes) == [SIG_INVALID]
    cases[0] = cases[0]._replace(expect=SIG_INVALID)
    cases[1] = cases[1]._replace(expect=SIG_INVALID)
    got = _check(ctx, cases, pair, group, (0, 1))
    assert list(got) == [SIG_INVALID, SIG_INVALID, HG_OK, HG_OK, HG_OK, HG_OK]


# ---------------------------------------------------------------- 5. every group fails
def test_all_groups_fail(ctx):
    bad = (3, 8, 23)
    cases, sigs = _batch(ctx, 24, {i: tampered for i in bad})
    got = _check(ctx, cases, sigs, 8, bad)
    assert ctx.eng.rlc_stats() == (3, 3, 24)
    assert [i for i in range(24) if got[i]] == list(bad)


# ---------------------------------------------------------------- 6. the device form
def test_device_form_on_a_stream_with_overlap_on_and_off(ctx):
    import torch

    e, n, group = ctx.eng, 21, 8
    bad = (5, 16)
    cases, sigs = _batch(ctx, n, {5: tampered, 16: tampered, 2: undecodable, 9: eof_message})
    want = _check(ctx, cases, sigs, group, bad)
    dev = torch.device("cuda:0")
    pool, off, ln = e.pack_messages([k.msg for k in cases])
    reqs, words = A._pack(cases)
    t = lambda a, dt: torch.frombuffer(bytearray(a), dtype=dt).to(dev)  # noqa: E731
    d_pool, d_sigs, d_reqs = t(pool.tobytes(), torch.uint8), t(sigs, torch.uint8), t(reqs.tobytes(), torch.uint8)
    d_words = t(words.tobytes(), torch.uint8)
    d_off, d_len = t(off.tobytes(), torch.int32), t(ln.tobytes(), torch.int32)
    try:
        for overlap in (False, True):
            e.set_fold_overlap(overlap)
            d_codes = torch.full((n,), -1, dtype=torch.int32, device=dev)
            s = torch.cuda.Stream(dev)
            torch.cuda.synchronize()
            e.verify_aggregate_msgs_rlc_device(d_pool.data_ptr(), len(pool), d_off.data_ptr(), d_len.data_ptr(),
                                               d_reqs.data_ptr(), n, d_words.data_ptr(), d_sigs.data_ptr(),
                                               d_codes.data_ptr(), seed=SEED, group=group, stream=s.cuda_stream)
            s.synchronize()
            assert np.array_equal(d_codes.cpu().numpy(), want), overlap
            assert e.rlc_stats() == _stats(cases, group, bad)
    finally:
        e.set_fold_overlap(True)


# ---------------------------------------------------------------- 7. a key outside G2
def test_non_g2_registry_runs_the_exact_path(torch_first):
    """The crafted go-flavor registry of tests/test_gpu_gt_scope.py (keys 10, 11,
    12 = A, B, -(A + B) outside G2): no combination, the exact call's codes."""
    from handel_amd.engine import Engine

    good = _messages(7, True, 100)
    ks = F.scalars(64, seed=b"non-g2")
    pts = [O.g2_mul(O.G2_GEN, k) for k in ks]
    a, b = F.non_g2_points(2, seed=3)
    pts[10], pts[11], pts[12] = a, b, O.g2_neg(O.g2_add(a, b))
    for i in (10, 11, 12):
        ks[i] = None
    reg = b"".join(O.g2_marshal(p) for p in pts)
    bits = lambda off, size, idx: tuple(off + i in idx for i in range(size))  # noqa: E731
    cases = [
        Case("A + B + C = inf, sig inf", good[0], 8, 8, bits(8, 8, (10, 11, 12)), "valid", good[0], HG_OK),
        Case("... any other sig", good[1], 8, 8, bits(8, 8, (10, 11, 12)), "tamper", good[1], SIG_INVALID),
        Case("honest sum + (A + B + C)", good[2], 0, 64, (True,) * 64, "valid", good[2], HG_OK),
        Case("A alone, sig inf", good[4], 8, 8, bits(8, 8, (10,)), "valid", good[4], SIG_INVALID),
        Case("honest keys only", good[5], 0, 8, bits(0, 8, (0, 3, 5)), "valid", good[5], HG_OK),
        Case("honest, another message", good[6], 32, 32, (True,) * 32, "valid", good[5], SIG_INVALID),
    ]
    e = Engine(device=0, flavor="go")
    try:
        assert list(e.registry_load(reg)) == [0] * 64
        sigs = A._sign(e, ks, cases)
        want, _ = A._oracle(reg, cases, sigs, fast=False)
        assert [int(c) for c in want] == [c.expect for c in cases]
        reqs, words = A._pack(cases)
        msgs = [c.msg for c in cases]
        exact = e.verify_aggregate_msgs(msgs, reqs, words, sigs)
        got = e.verify_aggregate_msgs_rlc(msgs, reqs, words, sigs, seed=SEED, group=4)
        assert list(got) == list(exact) == list(want)
        assert e.rlc_stats() == (0, 0, 0) and e.registry_non_g2() == 3
    finally:
        e.close()


# ---------------------------------------------------------------- 8. the context is untouched
def test_context_state_is_untouched(torch_first):
    """A context with a message and level-2 torus tables on a 64-key registry
    gives the same answers, at the same level, after combined calls on other messages."""
    from handel_amd.engine import REQ_DTYPE, Engine

    e = Engine(device=0, flavor="go")
    try:
        msg = F.LIB_MESSAGE
        ks, reg, _ = F.keys_and_sigs(64, msg=msg, seed=b"aggmsgs-ctx")
        assert not e.registry_load(reg).any()
        assert e.set_message(msg) == 0
        e.set_aggregate_level(2)
        assert e.prepare_aggregate() == 0
        agg = R.sign(msg, (sum(ks[i] for i in (0, 2, 5, 33)) % O.ORDER).to_bytes(32, "big"))
        reqs = np.array([(0, 64, 64, 0), (0, 64, 64, 1), (0, 64, 64, 2)], dtype=REQ_DTYPE)
        words = np.array([0b100101 | 1 << 33, 0b100111 | 1 << 33, 0], dtype=np.uint64)

        def state():
            return (e.aggregate_tables(), e.aggregate_tables_torus(), list(e.verify_aggregate(reqs, words, agg * 3)))

        before = state()
        assert before[0] == 2 and before[2] == [0, 1, 6]
        others = _messages(2, True, 100) + [F.REJECT_MESSAGES[0]]
        assert not M.hashable(others[2])
        cases = [Case("other", m, 0, 64, tuple(i in (0, 2, 5, 33) for i in range(64)), "valid",
                      m if M.hashable(m) else others[0], 0) for m in others]
        got = e.verify_aggregate_msgs_rlc(others, reqs, np.array([words[0]] * 3, dtype=np.uint64),
                                          A._sign(e, ks, cases), seed=SEED, group=2)
        assert list(got) == [HG_OK, HG_OK, HASH_EOF] and e.rlc_stats() == (1, 0, 0)
        # the context's own message, given per request, gives its own verdicts
        assert list(e.verify_aggregate_msgs_rlc([msg] * 3, reqs, words, agg * 3, seed=SEED, group=2)) == before[2]
        assert e.rlc_stats() == (1, 1, 2)
        assert state() == before
    finally:
        e.close()


# ---------------------------------------------------------------- 9. phase intervals
def test_phase_interval_counts(ctx):
    """What hg_timing_read_phase reports for one combined call: 13 requests in
    groups of 4 (three full groups and a ragged one), request 5 with an invalid
    signature, so the recheck runs inside the intervals. One submission, one
    aggregate interval (the G2 fold), one verify interval (the combination and
    the recheck)."""
    e = ctx.eng
    cases, sigs = _batch(ctx, 13, {5: tampered})
    reqs, words = A._pack(cases)
    e.timing_enable(True)
    try:
        for ph in range(3):
            e.timing_read_phase(ph)
        got = e.verify_aggregate_msgs_rlc([k.msg for k in cases], reqs, words, sigs, seed=SEED, group=4)
        read = [e.timing_read_phase(ph) for ph in (PHASE_SUBMIT, PHASE_AGGREGATE, PHASE_VERIFY)]
    finally:
        e.timing_enable(False)
    print("submit, aggregate, verify (ms, intervals):", read)
    assert [i for i in range(13) if got[i]] == [5] and got[5] == SIG_INVALID and e.rlc_stats() == (4, 1, 4)
    assert [k for _, k in read] == [1, 1, 1]
    assert all(ms > 0 for ms, _ in read)
