"""GPU suite of the random linear combination of independent checks on
arbitrary keys (hg_verify_batch_rlc*, hg_verify_batch_msgs_rlc*,
hg_batch_rlc_stats and the probes hg_debug_g2_member,
hg_debug_batch_rlc_groups). The expectation everywhere is the C
oracle's R.verify_batch called once per check with that check's message and the
exact call (hg_verify_batch, hg_verify_batch_msgs) on the same batch: the bar is
equal codes, check for check, and statistics equal to the counts the planted
errors give.

One pool of 150 valid checks per form: the one-message form's on one message,
the per-message form's each on its own message (lengths around SHA-256's padding
boundaries). Every batch is a prefix of the pool (taken twice over where a test
needs more) with checks replaced. The oracle's code of a check is computed once
and kept."""

import ctypes

import numpy as np
import pytest

from oracle import bn256_oracle as O
from oracle import ref_lib as R
from tests import _fixtures as F
from tests import _msgs_fixtures as M

pytestmark = pytest.mark.gpu

HG_OK, SIG_INVALID, HASH_EOF, PK_UNMARSHAL, SIG_UNMARSHAL, CF_MALFORMED, HG_ERR_ARG = 0, 1, 2, 4, 5, 8, 100
PHASE_VERIFY, PHASE_AGGREGATE, PHASE_SUBMIT = 0, 1, 2  # enum hg_phase
FLAVOR_ID = {"go": 0, "cf": 1}
POOL = 150
SEED = bytes(range(11, 43))
MSG = F.LIB_MESSAGE
INF_G1, INF_G2 = bytes(64), bytes(128)
OFF_CURVE_G1 = (1).to_bytes(32, "big") + (1).to_bytes(32, "big")
OFF_CURVE_G2 = bytes(127) + b"\x01"
G1 = O.g1_marshal(O.G1_GEN)
NEG_G1 = O.g1_marshal(O.g1_neg(O.G1_GEN))


@pytest.fixture(scope="module", autouse=True)
def torch_first():
    """torch's HIP runtime before the engines' (the device forms move tensors)."""
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


POOL_MSGS = _messages(POOL, True, 300)
EOF_MSGS = _messages(2, False, 700)
assert {len(m) for m in POOL_MSGS} == set(M.LENGTHS)
_POOL = {}


def _pool():
    """Keys and the two forms' signatures, made on first use and kept."""
    if not _POOL:
        ks = F.scalars(POOL, seed=b"batch-rlc")
        _POOL["ks"] = ks
        _POOL["pks"] = R.g2_scalar_base(F.scalar_bytes(ks))
        _POOL["one"] = R.sign(MSG, F.scalar_bytes(ks))
        _POOL["msgs"] = [R.sign(POOL_MSGS[i], ks[i].to_bytes(32, "big")) for i in range(POOL)]
    return _POOL


def pk(i):
    return _pool()["pks"][128 * (i % POOL):128 * (i % POOL) + 128]


def sign(i, m):
    return R.sign(m, _pool()["ks"][i % POOL].to_bytes(32, "big"))


def pool_cases(form, n):
    """The first n checks (msg, pk, sig) of the form's pool, all valid."""
    if form == "one":
        return [(MSG, pk(i), _pool()["one"][64 * (i % POOL):64 * (i % POOL) + 64]) for i in range(n)]
    return [(POOL_MSGS[i % POOL], pk(i), _pool()["msgs"][i % POOL]) for i in range(n)]


_CODES = {}  # (msg, pk, sig, flavor) -> the oracle's code: every test shares it


def oracle(cases, flavor):
    """R.verify_batch per check, in the reference's order: for a message that
    cannot be hashed the oracle's own decode of the key and the signature comes
    first (tests/test_gpu_verify_msgs.py _oracle_code)."""
    out = []
    for m, p, s in cases:
        key = (m, p, s, flavor)
        if key not in _CODES:
            c = int(R.verify_batch(m, p, s, flavor=FLAVOR_ID[flavor])[0])
            if c == HASH_EOF:
                d = int(R.verify_batch(MSG, p, s, flavor=FLAVOR_ID[flavor])[0])
                if d not in (HG_OK, SIG_INVALID):
                    c = d
            _CODES[key] = c
        out.append(_CODES[key])
    return np.array(out, dtype=np.int32)


def fold_cf(e, got, cases):
    """The engine's codes in the oracle's terms: cloudflare's named unmarshal
    failures (7..9: pk, 10..12: sig) are the oracle's 4 and 5."""
    out = np.array(got, dtype=np.int32).copy()
    for i in range(len(out)):
        if 7 <= out[i] <= 9:
            assert e.flavor_name == "cf", i
            out[i] = PK_UNMARSHAL
        elif 10 <= out[i] <= 12:
            assert e.flavor_name == "cf", i
            out[i] = SIG_UNMARSHAL
    return out


@pytest.fixture(scope="module", params=["go", "cf"])
def eng(request, torch_first):
    from handel_amd.engine import Engine

    e = Engine(device=0, flavor=request.param)
    assert e.set_message(MSG) == 0
    yield e
    e.close()


def split(cases):
    return [m for m, _, _ in cases], b"".join(p for _, p, _ in cases), b"".join(s for _, _, s in cases)


def run_exact(e, form, cases):
    msgs, pks, sigs = split(cases)
    return e.verify_batch(pks, sigs) if form == "one" else e.verify_batch_msgs(msgs, pks, sigs)


def run_rlc(e, form, cases, group, seed=SEED):
    msgs, pks, sigs = split(cases)
    if form == "one":
        return e.verify_batch_rlc(pks, sigs, seed=seed, group=group)
    return e.verify_batch_msgs_rlc(msgs, pks, sigs, seed=seed, group=group)


def stats_of(want, group, failing, non_g2=0):
    """(groups with a live member, groups holding a failing live member, the
    live members of those groups, non_g2) from the expected codes alone."""
    live = [int(c) in (HG_OK, SIG_INVALID) for c in want]
    groups = failed = rechecked = 0
    for g in range(0, len(want), group):
        members = range(g, min(len(want), g + group))
        cnt = sum(live[i] for i in members)
        groups += cnt > 0
        if any(i in failing for i in members):
            failed += 1
            rechecked += cnt
    return groups, failed, rechecked, non_g2


def check(e, form, cases, group, failing, non_g2=0, seed=SEED):
    """rlc codes == exact codes == oracle codes, and the statistics."""
    want = oracle(cases, e.flavor_name)
    exact = run_exact(e, form, cases)
    got = run_rlc(e, form, cases, group, seed)
    stats = e.batch_rlc_stats()
    print(form, e.flavor_name, len(cases), group, "stats", stats, "want", stats_of(want, group, failing, non_g2))
    assert np.array_equal(got, exact), [(i, int(g), int(x)) for i, (g, x) in enumerate(zip(got, exact)) if g != x]
    assert np.array_equal(fold_cf(e, got, cases), want), [(i, int(g), int(x)) for i, (g, x) in
                                                          enumerate(zip(got, want)) if g != x]
    assert stats == stats_of(want, group, failing, non_g2)
    assert e.rlc_stats() == stats[:3]  # hg_rlc_stats reports on these calls too
    return got


# ---------------------------------------------------------------- 1. the membership probe
def _probe_keys():
    """37 keys, nine full waves of four teams and one team: members, infinity,
    the three small orders, each plus a member, large-order points outside G2,
    a key that does not decode."""
    pts = F.small_order_points()
    member = lambda i: O.g2_unmarshal(pk(i))[0]  # noqa: E731
    special = {
        1: O.g2_marshal(pts[13]), 2: INF_G2, 6: O.g2_marshal(pts[7369]), 7: O.g2_marshal(pts[95797]),
        11: O.g2_marshal(O.g2_add(pts[13], member(11))), 12: O.g2_marshal(O.g2_add(pts[7369], member(12))),
        17: O.g2_marshal(O.g2_add(pts[95797], member(17))), 20: OFF_CURVE_G2, 23: O.g2_marshal(O.g2_mul(pts[13], 5)),
        35: INF_G2,
    }
    for j, q in zip((3, 18, 29, 36), F.non_g2_points(4)):
        special[j] = O.g2_marshal(q)
    return [special.get(i, pk(i)) for i in range(37)]


def test_probe_flags_equal_the_oracles_subgroup_test(eng):
    keys = _probe_keys()
    flags, codes = eng.g2_members(b"".join(keys))
    n_out = 0
    for i, kb in enumerate(keys):
        q, err = O.g2_unmarshal(kb, "go")
        if err is not None:  # does not decode in either flavor
            assert codes[i] != HG_OK and flags[i] == 0, i
            continue
        inside = q is None or O.g2_in_subgroup(q)  # infinity is a member
        n_out += not inside
        if eng.flavor_name == "go":
            assert codes[i] == HG_OK and flags[i] == int(inside), (i, int(flags[i]), inside)
        else:  # cloudflare's decode refuses the keys outside G2
            assert codes[i] == (HG_OK if inside else CF_MALFORMED) and flags[i] == int(inside), (i, int(codes[i]))
    assert n_out == 11 and int(flags.sum()) == 37 - 11 - 1
    # one key alone, and a ragged wave
    assert list(eng.g2_members(keys[0])[0]) == [1]
    f5, _ = eng.g2_members(b"".join(keys[:5]))
    assert list(f5) == [int(x) for x in flags[:5]]


# ---------------------------------------------------------------- 2. all valid
@pytest.mark.parametrize("group", [16, 64])
@pytest.mark.parametrize("form", ["one", "msgs"])
def test_all_valid_pool(eng, form, group):
    cases = pool_cases(form, POOL)
    got = check(eng, form, cases, group, ())
    assert not got.any()
    # the combination ran and nothing hid in the recheck
    assert eng.batch_rlc_stats() == ((POOL + group - 1) // group, 0, 0, 0)


# ---------------------------------------------------------------- 3. planted errors
def _planted(form, n=100):
    """(cases, failing): a tampered signature in two groups, undecodable key and
    signature, an infinity signature, a key at infinity with the infinity
    signature (valid) and with another (invalid), and in the per-message form two
    messages that cannot be hashed."""
    cases = pool_cases(form, n)
    rep = lambda i, **kw: cases.__setitem__(i, (kw.get("m", cases[i][0]), kw.get("p", cases[i][1]),  # noqa: E731
                                                kw.get("s", cases[i][2])))
    rep(5, s=sign(6, cases[5][0]))       # another key's signature: group 0
    rep(40, s=sign(40, b"another message"))  # group 2
    rep(17, p=OFF_CURVE_G2)
    rep(18, s=OFF_CURVE_G1)
    rep(19, p=OFF_CURVE_G2, s=OFF_CURVE_G1)
    rep(50, s=INF_G1)                    # live, fails group 3
    rep(66, p=INF_G2, s=INF_G1)          # e(H, O) e(O, G2Base) = 1: valid, group 4 stays whole
    rep(81, p=INF_G2)                    # a key at infinity under a real signature: group 5 fails
    failing = {5, 40, 50, 81}
    if form == "msgs":
        rep(70, m=EOF_MSGS[0])
        rep(71, m=EOF_MSGS[1], s=OFF_CURVE_G1)  # the unmarshal error comes first
    return cases, failing


@pytest.mark.parametrize("form", ["one", "msgs"])
def test_planted_errors(eng, form):
    cases, failing = _planted(form)
    want = oracle(cases, eng.flavor_name)
    assert {i for i in range(len(cases)) if want[i] == SIG_INVALID} == failing
    assert want[66] == HG_OK and want[17] == want[19] == PK_UNMARSHAL and want[18] == SIG_UNMARSHAL
    if form == "msgs":
        assert want[70] == HASH_EOF and want[71] == SIG_UNMARSHAL
    check(eng, form, cases, 16, failing)
    groups, failed, rechecked, non_g2 = eng.batch_rlc_stats()
    assert (groups, failed, rechecked, non_g2) == (7, 4, 64, 0)  # groups 0, 2, 3 and 5, every member live
    # another seed: the same codes
    check(eng, form, cases, 16, failing, seed=bytes(32))


def test_one_message_form_on_a_message_that_cannot_be_hashed(eng):
    cases = [(EOF_MSGS[0], p, s) for _, p, s in _planted("one")[0][:24]]
    try:
        assert eng.set_message(EOF_MSGS[0]) == HASH_EOF
        got = check(eng, "one", cases, 8, ())
        assert set(int(c) for c in fold_cf(eng, got, cases)) == {HASH_EOF, PK_UNMARSHAL, SIG_UNMARSHAL}
        assert eng.batch_rlc_stats() == (0, 0, 0, 0)
    finally:
        assert eng.set_message(MSG) == 0


# ---------------------------------------------------------------- 4. keys outside G2
@pytest.mark.parametrize("form", ["one", "msgs"])
def test_non_member_keys_fail_their_groups(eng, form):
    """An order-13 key, pk + C13 under a signature valid for pk and a
    large-order point outside G2, in three different groups, the rest valid. In
    go they are live: each fails its group, whatever the group's product, and
    the exact recheck gives the codes. In cf the decode refuses them."""
    n, group, where = 48, 8, (3, 20, 37)
    pts = F.small_order_points()
    cases = pool_cases(form, n)
    keys = [pts[13], O.g2_add(O.g2_unmarshal(pk(20))[0], pts[13]), F.non_g2_points(1, seed=9)[0]]
    for i, q in zip(where, keys):
        cases[i] = (cases[i][0], O.g2_marshal(q), cases[i][2])
    want = oracle(cases, eng.flavor_name)
    go = eng.flavor_name == "go"
    if go:
        assert all(int(want[i]) in (HG_OK, SIG_INVALID) for i in where) and want[3] == SIG_INVALID
        got = check(eng, form, cases, group, set(where), non_g2=3)
        assert eng.batch_rlc_stats() == (6, 3, 24, 3)
    else:
        assert [int(want[i]) for i in where] == [PK_UNMARSHAL] * 3
        got = check(eng, form, cases, group, ())
        assert [int(got[i]) for i in where] == [CF_MALFORMED] * 3 and eng.batch_rlc_stats() == (6, 0, 0, 0)
    assert not np.delete(got, where).any()
    # the probe: the three groups are not accepted, whatever the coefficients
    msgs, pks, sigs = split(cases)
    for coeffs in ([1] * n, [int(x) for x in eng.debug_rlc_coeffs(SEED, 0, n)]):
        codes, gcodes, glive = eng.debug_batch_rlc_groups(None if form == "one" else msgs, pks, sigs, coeffs, group)
        assert list(glive) == ([8] * 6 if go else [7, 8, 7, 8, 7, 8])
        assert [int(c) != HG_OK for c in gcodes] == [go and g in (0, 2, 4) for g in range(6)], list(gcodes)
        assert not np.delete(codes, where).any()


# ---------------------------------------------------------------- 5. the inversion block
@pytest.mark.parametrize("at", [255, 256])
def test_order_13_key_beside_a_full_inversion_block(eng, at):
    """300 groups of one check: 300 final exponentiations across the 256-wide
    inversion block. The order-13 key's Miller value is zero; its neighbours,
    in its block and in the next, stay HG_OK."""
    n = 300
    cases = pool_cases("one", n)
    cases[at] = (MSG, O.g2_marshal(F.small_order_points()[13]), cases[at][2])
    go = eng.flavor_name == "go"
    got = check(eng, "one", cases, 1, {at} if go else (), non_g2=1 if go else 0)
    assert int(got[at]) == (SIG_INVALID if go else CF_MALFORMED)
    assert not np.delete(got, at).any()
    assert eng.batch_rlc_stats() == ((300, 1, 1, 1) if go else (299, 0, 0, 0))


# ---------------------------------------------------------------- 6. secrecy matters
@pytest.mark.parametrize("form", ["one", "msgs"])
def test_cancelling_pair_needs_secret_coefficients(eng, form):
    n, group = 6, 6
    cases = pool_cases(form, n)
    cases[0] = (cases[0][0], cases[0][1], R.g1_add(cases[0][2], G1))      # sig_a + D
    cases[1] = (cases[1][0], cases[1][1], R.g1_add(cases[1][2], NEG_G1))  # sig_b - D
    msgs, pks, sigs = split(cases)
    m = None if form == "one" else msgs
    _, gcodes, glive = eng.debug_batch_rlc_groups(m, pks, sigs, [1] * n, group)
    assert list(gcodes) == [HG_OK] and list(glive) == [n]  # equal coefficients cannot see it
    _, gcodes, _ = eng.debug_batch_rlc_groups(m, pks, sigs, [7] * n, group)
    assert list(gcodes) == [HG_OK]
    _, gcodes, _ = eng.debug_batch_rlc_groups(m, pks, sigs, [1, 2, 1, 1, 1, 1], group)
    assert list(gcodes) == [SIG_INVALID]
    got = check(eng, form, cases, group, {0, 1})
    assert list(got) == [SIG_INVALID, SIG_INVALID, HG_OK, HG_OK, HG_OK, HG_OK]


# ---------------------------------------------------------------- 7. sizes and arguments
@pytest.mark.parametrize("form", ["one", "msgs"])
def test_sizes(eng, form):
    one = pool_cases(form, 1)
    assert list(check(eng, form, one, 64, ())) == [HG_OK] and eng.batch_rlc_stats() == (1, 0, 0, 0)
    bad = [(one[0][0], one[0][1], sign(1, one[0][0]))]
    assert list(check(eng, form, bad, 1, {0})) == [SIG_INVALID] and eng.batch_rlc_stats() == (1, 1, 1, 0)
    # n no multiple of group, with a failing check in the ragged last group; group > n
    cases = pool_cases(form, 13)
    cases[12] = (cases[12][0], cases[12][1], sign(0, cases[12][0]))
    for group, stats in ((5, (3, 1, 3, 0)), (4096, (1, 1, 13, 0))):
        got = check(eng, form, cases, group, {12})
        assert [i for i in range(13) if got[i]] == [12] and eng.batch_rlc_stats() == stats
    # n = 0
    assert len(run_rlc(eng, form, [], 64)) == 0 and eng.batch_rlc_stats() == (0, 0, 0, 0)


def test_argument_errors(eng):
    L, ctx = eng.L, eng.ctx
    msgs, pks, sigs = split(pool_cases("msgs", 2))
    pool, off, ln = eng.pack_messages(msgs)
    u8 = lambda b: np.frombuffer(b, dtype=np.uint8).copy()  # noqa: E731
    a, b, sd = u8(pks), u8(sigs), u8(SEED)
    codes = np.zeros(2, dtype=np.int32)
    p = lambda x: x.ctypes.data_as(ctypes.c_void_p)  # noqa: E731
    for group, seed in ((0, p(sd)), (4097, p(sd)), (64, None)):
        assert L.hg_verify_batch_rlc(ctx, p(a), p(b), 2, seed, group, p(codes)) == HG_ERR_ARG
        assert L.hg_verify_batch_msgs_rlc(ctx, p(pool), len(pool), p(off), p(ln), p(a), p(b), 2, seed, group,
                                          p(codes)) == HG_ERR_ARG
    # a message range that leaves the pool: the whole host call is refused, as hg_verify_batch_msgs
    far = off.copy()
    far[1] = len(pool)
    assert L.hg_verify_batch_msgs_rlc(ctx, p(pool), len(pool), p(far), p(ln), p(a), p(b), 2, p(sd), 64,
                                      p(codes)) == HG_ERR_ARG
    assert b"message 1" in L.hg_last_error(ctx)
    assert L.hg_verify_batch_rlc(ctx, None, None, 0, p(sd), 64, None) == HG_OK


def test_one_message_form_needs_a_message(torch_first):
    from handel_amd.engine import Engine, HandelGPUError

    e = Engine(device=0, flavor="go")
    try:
        _, pks, sigs = split(pool_cases("one", 2))
        with pytest.raises(HandelGPUError):
            e.verify_batch_rlc(pks, sigs, seed=SEED)
        # the per-message form needs none
        msgs, pks, sigs = split(pool_cases("msgs", 2))
        assert not e.verify_batch_msgs_rlc(msgs, pks, sigs, seed=SEED).any()
    finally:
        e.close()


@pytest.mark.parametrize("form", ["one", "msgs"])
def test_device_forms_equal_the_host_forms(eng, form):
    import torch

    group = 16
    cases, failing = _planted(form, 90)
    want = check(eng, form, cases, group, failing)
    stats = eng.batch_rlc_stats()
    msgs, pks, sigs = split(cases)
    n = len(cases)
    dev = torch.device("cuda:0")
    t = lambda a, dt: torch.frombuffer(bytearray(a), dtype=dt).to(dev)  # noqa: E731
    d_pks, d_sigs = t(pks, torch.uint8), t(sigs, torch.uint8)
    if form == "msgs":
        pool, off, ln = eng.pack_messages(msgs)
        ln = ln.copy()
        ln[30] = len(pool) + 1  # a range that leaves the pool: HG_ERR_ARG for that check alone
        want = want.copy()
        want[30] = HG_ERR_ARG
        d_pool, d_off, d_len = t(pool.tobytes(), torch.uint8), t(off.tobytes(), torch.int32), t(ln.tobytes(),
                                                                                               torch.int32)
    try:
        for overlap in (False, True):
            eng.set_fold_overlap(overlap)
            d_codes = torch.full((n,), -1, dtype=torch.int32, device=dev)
            s = torch.cuda.Stream(dev)
            torch.cuda.synchronize()
            if form == "one":
                eng.verify_batch_rlc_device(d_pks.data_ptr(), d_sigs.data_ptr(), n, d_codes.data_ptr(), seed=SEED,
                                            group=group, stream=s.cuda_stream)
                x_codes = torch.full((n,), -1, dtype=torch.int32, device=dev)
                eng.verify_batch_device(d_pks.data_ptr(), d_sigs.data_ptr(), n, x_codes.data_ptr(), s.cuda_stream)
            else:
                eng.verify_batch_msgs_rlc_device(d_pool.data_ptr(), len(pool), d_off.data_ptr(), d_len.data_ptr(),
                                                 d_pks.data_ptr(), d_sigs.data_ptr(), n, d_codes.data_ptr(),
                                                 seed=SEED, group=group, stream=s.cuda_stream)
                x_codes = torch.full((n,), -1, dtype=torch.int32, device=dev)
                eng.verify_batch_msgs_device(d_pool.data_ptr(), len(pool), d_off.data_ptr(), d_len.data_ptr(),
                                             d_pks.data_ptr(), d_sigs.data_ptr(), n, x_codes.data_ptr(),
                                             s.cuda_stream)
            s.synchronize()
            assert np.array_equal(d_codes.cpu().numpy(), want), overlap
            assert np.array_equal(d_codes.cpu().numpy(), x_codes.cpu().numpy()), overlap
            # (check 30 sits in group 1, which holds no failing check: the same counts)
            assert eng.batch_rlc_stats() == stats
    finally:
        eng.set_fold_overlap(True)


# ---------------------------------------------------------------- 8. phase intervals
@pytest.mark.parametrize("form", ["one", "msgs"])
def test_phase_interval_counts(eng, form):
    """What hg_timing_read_phase reports for one combined call: 13 checks in
    groups of 4 (three full groups and a ragged one), check 5 with an invalid
    signature, so the recheck runs inside the intervals. One submission, no
    aggregate interval (nothing is folded), one verify interval (the combination
    and the recheck)."""
    cases = pool_cases(form, 13)
    cases[5] = (cases[5][0], cases[5][1], sign(6, cases[5][0]))
    eng.timing_enable(True)
    try:
        for ph in range(3):
            eng.timing_read_phase(ph)
        got = run_rlc(eng, form, cases, 4)
        read = [eng.timing_read_phase(ph) for ph in (PHASE_SUBMIT, PHASE_AGGREGATE, PHASE_VERIFY)]
    finally:
        eng.timing_enable(False)
    print("submit, aggregate, verify (ms, intervals):", read)
    assert [i for i in range(13) if got[i]] == [5] and got[5] == SIG_INVALID
    assert eng.batch_rlc_stats() == (4, 1, 4, 0)
    assert [k for _, k in read] == [1, 0, 1]
    assert all((ms > 0) == (k > 0) for ms, k in read)
