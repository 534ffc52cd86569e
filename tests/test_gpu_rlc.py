"""GPU suite: aggregate batches verified by random linear combination
(handel_amd/csrc/bn256_rlc.hip, hg_rlc.cpp; include/handel_gpu.h
hg_verify_aggregate_rlc*, hg_rlc_stats, hg_debug_rlc_g1, hg_debug_rlc_groups).

A 50-key registry under three table forms: level 1 (classical), level 2 in
torus form, and level 2 of a registry holding k and r - k, whose set stays
classical. The G1 side is compared with the Python oracle's group law, the
group verdicts are pinned with given coefficients (the Horner chain's top and
bottom bits, an invalid member, the cancelling pair that equal coefficients
cannot see), and the entry point's codes are compared with hg_verify_aggregate
and with the C restatement of the reference (oracle.ref_lib.verify_aggregate),
its statistics with the grouping rule.
"""

import hashlib

import numpy as np
import pytest

from handel_amd import _lib
from handel_amd.engine import REQ_DTYPE, Engine
from oracle import bn256_oracle as O
from oracle import ref_lib as R
from tests import _fixtures as F

pytestmark = pytest.mark.gpu

MSG = F.LIB_MESSAGE
N_REG = 50
CF_CODES = {O.ERR_CF_EXCEEDS: _lib.HG_ERR_SIG_CF_EXCEEDS, O.ERR_CF_MALFORMED: _lib.HG_ERR_SIG_CF_MALFORMED,
            O.ERR_CF_NOT_ENOUGH: _lib.HG_ERR_SIG_CF_SHORT}
OFF_CURVE = (1).to_bytes(32, "big") * 2  # (1, 1): 1 != 1 + 3
INFINITY = bytes(64)
G1 = O.g1_marshal(O.G1_GEN)
NEG_G1 = O.g1_marshal(O.g1_neg(O.G1_GEN))
SEEDS = (hashlib.sha256(b"rlc-gpu-0").digest(), hashlib.sha256(b"rlc-gpu-1").digest())
RANGES = [(0, 50), (0, 32), (32, 18), (16, 16), (48, 2), (5, 40), (7, 1)]
OK, INVALID = _lib.HG_OK, _lib.HG_ERR_SIG_INVALID


class Setup:
    def __init__(self, eng, ks, reg, form):
        self.eng, self.ks, self.reg, self.form = eng, ks, reg, form


# (flavor, table form): every form under go, the torus form under cloudflare's decode rules too
@pytest.fixture(scope="module", params=[("go", "level1"), ("go", "torus"), ("go", "classical2"), ("cf", "torus")],
                ids=lambda p: "-".join(p))
def st(request):
    import torch

    if torch.cuda.is_available():  # torch's HIP runtime before the engine's (the device form moves tensors)
        torch.cuda.set_device(0)
        torch.zeros(1, device="cuda")
    flavor, form = request.param
    e = Engine(device=0, flavor=flavor)
    ks = F.scalars(N_REG, seed=b"rlc-registry")
    if form == "classical2":
        ks[3] = O.ORDER - ks[2]  # keys 2 and 3 sum to zero: e(H, 0) = 1 has no torus form
    level = 1 if form == "level1" else 2
    e.set_aggregate_level(level)
    reg = R.g2_scalar_base(F.scalar_bytes(ks))
    assert not e.registry_load(reg).any()
    assert e.prepare_aggregate_msg(MSG) == 0 and e.aggregate_tables() == level
    assert e.aggregate_tables_torus() == (form == "torus")
    yield Setup(e, ks, reg, form)
    e.close()


def _sign(ks, ranges, bitsets):
    scal = b""
    for (off, _), bits in zip(ranges, bitsets):
        k = sum(ks[off + i] for i, b in enumerate(bits) if b) % O.ORDER
        scal += (k or 1).to_bytes(32, "big")
    return R.sign(MSG, scal)


def _valid_batch(st, n, seed=5):
    """n requests over RANGES with random non-empty bitsets that avoid keys 2
    and 3 together (their sum is zero in the classical2 registry), all signed."""
    rng = np.random.default_rng(seed)
    ranges = [RANGES[int(rng.integers(len(RANGES)))] for _ in range(n)]
    bitsets = F.random_bitsets(rng, [s for _, s in ranges])
    for (off, _), b in zip(ranges, bitsets):
        b[int(rng.integers(len(b)))] = True
        if off <= 2 and off + len(b) > 3:
            b[3 - off] = False
            b[2 - off] = True
    reqs, words = F.pack_requests(ranges, bitsets)
    return np.array(reqs, dtype=REQ_DTYPE), words, bytearray(_sign(st.ks, ranges, bitsets))


def _put(sigs, i, s):
    sigs[64 * i:64 * i + 64] = s


def _get(sigs, i):
    return bytes(sigs[64 * i:64 * i + 64])


def _want(st, reqs, words, sigs):
    sigs = bytes(sigs)
    want = R.verify_aggregate(MSG, st.reg, reqs["offset"], reqs["bitlen"], reqs["level_size"], words,
                              reqs["word_offset"].astype(np.uint64), sigs, nthreads=8)
    if st.eng.flavor_name == "cf":  # the restatement decodes as go: cloudflare's decode errors have their own codes
        for i in range(len(reqs)):
            _, err = O.g1_unmarshal(sigs[64 * i:64 * i + 64], "cf")
            if err is not None:
                want[i] = CF_CODES[err]
    return np.asarray(want)


def _check(st, reqs, words, sigs, group, seed, stats=None, want=None):
    """rlc codes == exact codes == oracle codes (want: computed before for these signatures)."""
    sigs = bytes(sigs)
    if want is None:
        want = _want(st, reqs, words, sigs)
        assert list(st.eng.verify_aggregate(reqs, words, sigs)) == list(want)
    got = st.eng.verify_aggregate_rlc(reqs, words, sigs, seed=seed, group=group)
    assert list(got) == list(want), (group, list(got), list(want))
    s = st.eng.rlc_stats()
    if stats is not None:
        assert s == stats, (s, stats)
    return want, s


def _groups_with_live(want_live, group):
    n = len(want_live)
    return sum(1 for g in range(0, n, group) if any(want_live[g:g + group]))


# ------------------------------------------------------------------ 1. the G1 side
def test_g1_side_matches_the_oracle_group_law(st):
    sigs7 = R.sign(MSG, F.scalar_bytes(F.scalars(7, seed=b"rlc-g1")))
    pts = [O.g1_unmarshal(sigs7[64 * i:64 * i + 64])[0] for i in range(7)]
    # group 0: P, -P, infinity; group 1: the same signature twice, one more; group 2: one
    pts[1] = O.g1_neg(pts[0])
    pts[2] = None
    pts[4] = pts[3]
    sigs = b"".join(O.g1_marshal(p) for p in pts)
    top, full = 1 << 63, (1 << 64) - 1
    for coeffs in ([5, 5, 7, top, top, full, 1],            # P - P + inf = infinity; the doubling case
                   [0, 1, 2, top, full, 2, 0xdeadbeefcafef00d],
                   [full, full, 1, 1, 1, 0, 0]):            # a zero coefficient: infinity on its own
        out = st.eng.debug_rlc_g1(sigs, coeffs, 3)
        for g in range(3):
            acc = None
            for i in range(3 * g, min(7, 3 * g + 3)):
                acc = O.g1_add(acc, O.g1_mul(pts[i], coeffs[i]) if pts[i] is not None else None)
            assert out[64 * g:64 * g + 64] == O.g1_marshal(acc), (coeffs, g)
    assert st.eng.debug_rlc_g1(sigs, [5, 5, 7, top, top, full, 1], 3)[:64] == bytes(64)


# ------------------------------------------------------------------ 2. group verdicts with given coefficients
def test_group_verdicts_with_given_coefficients(st):
    reqs, words, sigs = _valid_batch(st, 6, seed=11)
    top, full = 1 << 63, (1 << 64) - 1
    coeffs = [1, top, full, 3, (1 << 62) + 1, 0x0123456789abcdef]
    codes, gcodes, glive = st.eng.debug_rlc_groups(reqs, words, bytes(sigs), coeffs, 3)
    assert list(codes) == [OK] * 6 and list(gcodes) == [OK, OK] and list(glive) == [3, 3]
    # one invalid signature: its group alone
    bad = bytearray(sigs)
    _put(bad, 4, R.g1_add(_get(sigs, 4), G1))
    codes, gcodes, glive = st.eng.debug_rlc_groups(reqs, words, bytes(bad), coeffs, 3)
    assert list(codes) == [OK] * 6 and list(gcodes) == [OK, INVALID] and list(glive) == [3, 3]
    # the cancelling pair sig_a + D, sig_b - D: equal coefficients cannot see it
    pair = bytearray(sigs)
    _put(pair, 0, R.g1_add(_get(sigs, 0), G1))
    _put(pair, 1, R.g1_add(_get(sigs, 1), NEG_G1))
    _, gcodes, _ = st.eng.debug_rlc_groups(reqs, words, bytes(pair), [1] * 6, 3)
    assert list(gcodes) == [OK, OK]
    _, gcodes, _ = st.eng.debug_rlc_groups(reqs, words, bytes(pair), [1, 2, 1, 1, 1, 1], 3)
    assert list(gcodes) == [INVALID, OK]
    want = _want(st, reqs, words, pair)
    assert list(want) == [INVALID, INVALID, OK, OK, OK, OK]


# ------------------------------------------------------------------ 3. end to end
@pytest.mark.parametrize("n,group", [(1, 1), (7, 4), (130, 64)])
def test_end_to_end_matches_exact_path_and_oracle(st, n, group):
    reqs, words, sigs = _valid_batch(st, n, seed=100 + n)
    ngroups = (n + group - 1) // group
    want, _ = _check(st, reqs, words, sigs, group, SEEDS[0], stats=(ngroups, 0, 0))
    assert list(want) == [OK] * n
    _check(st, reqs, words, sigs, group, SEEDS[1], stats=(ngroups, 0, 0), want=want)
    # one tampered signature: its group fails and is verified one by one
    t = n - 1
    bad = bytearray(sigs)
    _put(bad, t, R.g1_add(_get(sigs, t), G1))
    live_in_group = min(n, (t // group + 1) * group) - (t // group) * group
    want, _ = _check(st, reqs, words, bad, group, SEEDS[0], stats=(ngroups, 1, live_in_group))
    assert list(want) == [OK] * t + [INVALID]
    _check(st, reqs, words, bad, group, SEEDS[1], stats=(ngroups, 1, live_in_group), want=want)
    if n >= 2:  # the cancelling pair, in one group: both rejected
        pair = bytearray(sigs)
        _put(pair, 0, R.g1_add(_get(sigs, 0), G1))
        _put(pair, 1, R.g1_add(_get(sigs, 1), NEG_G1))
        want, _ = _check(st, reqs, words, pair, group, SEEDS[0], stats=(ngroups, 1, min(n, group)))
        assert list(want[:2]) == [INVALID, INVALID] and not want[2:].any()
        _check(st, reqs, words, pair, group, SEEDS[1], stats=(ngroups, 1, min(n, group)), want=want)


def test_checks_decided_before_the_pairing_keep_their_codes(st):
    reqs, words, sigs = _valid_batch(st, 7, seed=77)
    reqs, sigs = reqs.copy(), bytearray(sigs)
    _put(sigs, 0, OFF_CURVE)                       # unmarshal error
    reqs["level_size"][1] = reqs["bitlen"][1] + 1  # level error
    words = words.copy()                           # empty bitset
    w0, nw = int(reqs["word_offset"][2]), (int(reqs["bitlen"][2]) + 63) // 64
    words[w0:w0 + nw] = 0
    # group 0 = {unmarshal, level, empty, valid}: one live member, and it holds
    want, _ = _check(st, reqs, words, sigs, 4, SEEDS[0], stats=(2, 0, 0))
    assert want[0] not in (OK, INVALID) and want[1] == _lib.HG_ERR_LEVEL and want[2] == _lib.HG_ERR_EMPTY_AGG
    assert list(want[3:]) == [OK] * 4
    # an infinity signature on a non-empty set is live and fails its group
    good5 = _get(sigs, 5)
    _put(sigs, 5, INFINITY)
    want, _ = _check(st, reqs, words, sigs, 4, SEEDS[1], stats=(2, 1, 3))
    assert want[5] == INVALID and list(want[[3, 4, 6]]) == [OK] * 3
    # groups of two: {unmarshal, level} has no live member and is skipped
    _put(sigs, 5, good5)
    want, _ = _check(st, reqs, words, sigs, 2, SEEDS[0], stats=(3, 0, 0))
    assert _groups_with_live([c == OK for c in want], 2) == 3


def test_device_form_on_its_own_stream(st):
    import torch

    import bench

    n, group = 7, 4
    reqs, words, sigs = _valid_batch(st, n, seed=31)
    _put(sigs, 2, R.g1_add(_get(sigs, 2), G1))
    want = _want(st, reqs, words, sigs)
    dev = torch.device("cuda", 0)
    d_r, d_w, d_s = (bench._dev_bytes(reqs.tobytes(), dev), bench._dev_bytes(words.tobytes(), dev),
                     bench._dev_bytes(bytes(sigs), dev))
    codes = torch.full((n,), -7, dtype=torch.int32, device=dev)
    torch.cuda.synchronize(dev)
    stream = torch.cuda.Stream(device=dev)
    st.eng.verify_aggregate_rlc_device(d_r.data_ptr(), n, d_w.data_ptr(), d_s.data_ptr(), codes.data_ptr(),
                                       seed=SEEDS[0], group=group, stream=stream.cuda_stream)
    stream.synchronize()
    assert list(codes.cpu().numpy()) == list(want) and list(want) == [OK, OK, INVALID, OK, OK, OK, OK]
    assert st.eng.rlc_stats() == (2, 1, 4)


# ------------------------------------------------------------------ 4. fall-through
def test_without_tables_the_exact_path_runs(st):
    reqs, words, sigs = _valid_batch(st, 7, seed=41)
    _put(sigs, 3, R.g1_add(_get(sigs, 3), G1))
    level = st.eng.aggregate_tables()
    st.eng.set_aggregate_level(0)
    try:
        want, _ = _check(st, reqs, words, sigs, 4, SEEDS[0], stats=(0, 0, 0))
        assert list(want) == [OK, OK, OK, INVALID, OK, OK, OK]
    finally:
        st.eng.set_aggregate_level(level)
    _check(st, reqs, words, sigs, 4, SEEDS[0], stats=(2, 1, 4))


# ------------------------------------------------------------------ 5. phase intervals
def test_phase_interval_counts(st):
    """What hg_timing_read_phase reports for one combined call at a GT level: 13
    checks in groups of 4 (three full groups and a ragged one), check 5 with an
    invalid signature, so the recheck runs inside the intervals. One submission;
    two aggregate intervals (the GT fold, the combination's GT stages); two
    pairing intervals (the groups', the recheck's)."""
    e = st.eng
    reqs, words, sigs = _valid_batch(st, 13, seed=13)
    _put(sigs, 5, R.g1_add(_get(sigs, 5), G1))
    e.timing_enable(True)
    try:
        for ph in range(3):
            e.timing_read_phase(ph)
        got = e.verify_aggregate_rlc(reqs, words, bytes(sigs), seed=SEEDS[0], group=4)
        read = [e.timing_read_phase(ph) for ph in (_lib.HG_PHASE_SUBMIT, _lib.HG_PHASE_AGGREGATE,
                                                   _lib.HG_PHASE_VERIFY)]
    finally:
        e.timing_enable(False)
    print("submit, aggregate, verify (ms, intervals):", read)
    assert [i for i in range(13) if got[i]] == [5] and got[5] == INVALID and e.rlc_stats() == (4, 1, 4)
    assert [k for _, k in read] == [1, 2, 2]
    assert all(ms > 0 for ms, _ in read)
