"""Public keys of small order on the twist, on the CPU: what the two oracles
say about them, pinned here because the GPU tests of
tests/test_gpu_small_order_keys.py lean on it.

x/crypto's G2.Unmarshal accepts any point of the twist curve
(bn256/go/bn256.go:113-120). The twist has n (2p - n) points and
2p - n = 13 * 7369 * (a 239-bit rest), so a go-flavor caller can hand over keys
of order 13, 7369 and 95797. For a key of order 13 the Miller loop's point R
runs into infinity, a line becomes zero, and the Miller value, its final
exponentiation and the marshalled GT value are all zero: such a key verifies
nothing, the infinity signature included (0 != 1). Keys of the other two
orders give ordinary-looking GT values. Also here: the compiled team programs
the GPU runs (tools/gen_g2_schedule.py), driven through a whole pk-side Miller
loop on these keys."""

import os
import sys

import pytest

from oracle import bn256_oracle as O
from oracle import ref_lib as R
from tests import _fixtures as F
from tests import _small_order_fixtures as S

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tools"))
import gen_g2_schedule as G  # noqa: E402

P = O.P
MSGS = (F.LIB_MESSAGE, F.TEST_MESSAGES[0])
F12_ZERO = [O.F2_ZERO] * 6


@pytest.fixture(scope="module")
def pts():
    return F.small_order_points()


@pytest.fixture(scope="module")
def hs():
    return [O.hashed_message(m)[0] for m in MSGS]


def _is_zero12(f):
    return all(O.f2_is_zero(c) for c in f)


# ---------------------------------------------------------------- the points
def test_twist_cofactor_and_the_three_orders(pts):
    assert F.TWIST_COFACTOR % 13 == 0 and F.TWIST_COFACTOR % 7369 == 0
    assert sorted(pts) == [13, 7369, 95797] and 13 * 7369 == 95797
    for m, t in pts.items():
        assert O.g2_on_curve(*t) and not O.g2_in_subgroup(t)
        assert O.g2_mul(t, m) is None
        for d in (1, 13, 7369):  # the order is m itself
            if d < m and m % d == 0:
                assert O.g2_mul(t, d) is not None
    assert F.small_order_points() == pts  # deterministic


def test_unmarshal_go_accepts_cf_refuses(pts):
    for m, t in pts.items():
        for k in (1, 2, 5, m - 1):
            q = O.g2_mul(t, k)
            b = O.g2_marshal(q)
            assert O.g2_unmarshal(b, "go") == (q, None)
            assert O.g2_unmarshal(b, "cf") == (None, O.ERR_CF_MALFORMED)


# ---------------------------------------------------------------- pairings
def test_order_13_pairs_to_zero_in_both_oracles(pts, hs):
    for k in range(1, 13):
        q = O.g2_mul(pts[13], k)
        for h in hs:
            assert _is_zero12(O.miller(q, h)), k
            gt = O.f12_marshal(O.pair(h, q))
            assert gt == R.pair(O.g1_marshal(h), O.g2_marshal(q)) == bytes(384), k
    assert _is_zero12(O.final_exponentiation(F12_ZERO)) and _is_zero12(O.final_exponentiation_fc(F12_ZERO))


def test_orders_7369_and_95797_pair_to_ordinary_values(pts, hs):
    for m in (7369, 95797):
        for k in (1, 2, 5):
            q = O.g2_mul(pts[m], k)
            gt = O.pair(hs[0], q)
            b = O.f12_marshal(gt)
            assert b == R.pair(O.g1_marshal(hs[0]), O.g2_marshal(q)), (m, k)
            assert b != bytes(384) and not O.f12_is_one(gt), (m, k)


# ---------------------------------------------------------------- verdicts
def test_verify_batch_fast_and_reference_agree_on_small_order_keys():
    pks, sigs = S.small_order_batch(F.LIB_MESSAGE)
    slow = R.verify_batch(F.LIB_MESSAGE, pks, sigs, fast=False)
    fast = R.verify_batch(F.LIB_MESSAGE, pks, sigs, fast=True)
    assert list(slow) == list(fast)
    # every order-13 check is invalid, with the infinity signature too (check 5)
    assert [int(slow[i]) for i in S.BATCH_ORDER13] == [R.RC_SIG_INVALID] * len(S.BATCH_ORDER13)
    assert slow[S.BATCH_OFF_CURVE_SIG] == R.RC_SIG_UNMARSHAL
    assert [int(slow[i]) for i in S.BATCH_HONEST] == [R.RC_OK] * len(S.BATCH_HONEST)
    assert [int(slow[i]) for i in S.BATCH_OTHER] == [R.RC_SIG_INVALID] * len(S.BATCH_OTHER)
    # the Python oracle, check by check
    for i in S.BATCH_ORDER13:
        pk = O.g2_unmarshal(pks[128 * i:128 * i + 128])[0]
        sig = O.g1_unmarshal(sigs[64 * i:64 * i + 64])[0]
        assert O.verify_signature(pk, F.LIB_MESSAGE, sig) == O.ERR_SIG_INVALID
        assert O.verify_signature_fast(pk, F.LIB_MESSAGE, sig) == O.ERR_SIG_INVALID


@pytest.mark.parametrize("which", ["mixed", "pure"])
def test_aggregates_of_order_13_registries_follow_the_closed_form(which):
    registry, reqs = ((S.mixed_registry(), S.mixed_requests()) if which == "mixed"
                      else (S.pure_registry(), S.pure_requests()))
    msg = F.LIB_MESSAGE
    sigs = b"".join(registry.signature(q, msg) for q in reqs)
    slow, agg = S.oracle_aggregate(registry, reqs, msg, sigs, fast=False)
    fast, agg_fast = S.oracle_aggregate(registry, reqs, msg, sigs, fast=True)
    assert slow == fast and agg == agg_fast
    for j, q in enumerate(reqs):
        assert agg[128 * j:128 * j + 128] == registry.closed_form(q), q.what
        # the honest keys' signature (infinity when there is none) is valid
        # exactly when the order-13 part cancels
        assert slow[j] == (R.RC_OK if registry.part13(q) == 0 else R.RC_SIG_INVALID), q.what
    zero = sum(agg[128 * j:128 * j + 128] == bytes(128) for j in range(len(reqs)))
    if which == "mixed":
        assert slow.count(R.RC_OK) >= 6 and slow.count(R.RC_SIG_INVALID) >= 6 and zero >= 3
    else:
        assert slow.count(R.RC_OK) == zero >= 4 and slow.count(R.RC_SIG_INVALID) >= 20


# ---------------------------------------------------------------- the team programs
X = None


def _programs():
    global X
    if X is None:
        X = G.compile_all()
    return X


def team_miller(q, h, limbs=False):
    """The pk-side Miller loop as the kernels run it (team_miller_check,
    bn256_pairing.h, without the G2Base side): R starts at (xi Qx, xi Qy,
    W = 1) as g2_regs_init sets it, every step is a compiled team program
    (PDBL, PADD_POS / PADD_NEG, then the two Frobenius additions PADD_F1 and
    PADD_F2) interpreted by run_xprogram, and f takes each step's line
    (LA, LB, LC) through the oracle's mulLine. limbs: the programs run limb
    for limb on Montgomery representatives, reduction tails included."""
    X = _programs()
    rinv = pow(G.R_MONT, -1, P)
    enc = (lambda v: G.to_limbs(v * G.R_MONT % P)) if limbs else (lambda v: v % P)
    dec = (lambda l: G.from_limbs(l) * rinv % P) if limbs else (lambda v: v)
    regs = {i: enc(0) for i in range(G.NREGS)}

    def put(n, v):
        regs[G.comp(n, "x")], regs[G.comp(n, "y")] = enc(v[0]), enc(v[1])

    def get(n):
        return (dec(regs[G.comp(n, "x")]), dec(regs[G.comp(n, "y")]))

    regs[G.REG["ONE"]] = enc(1)
    regs[G.REG["PX"]], regs[G.REG["PY"]] = enc(h[0]), enc(h[1])
    put("X", O.f2_mul_xi(q[0]))
    put("Y", O.f2_mul_xi(q[1]))
    put("Z", O.F2_ONE)
    put("QX", q[0])
    put("QY", q[1])
    put("NQY", O.f2_neg(q[1]))
    put("P1X", O.f2_mul(O.f2_conj(q[0]), O.XI_TO_P_MINUS_1_OVER_3))
    put("P1Y", O.f2_mul(O.f2_conj(q[1]), O.XI_TO_P_MINUS_1_OVER_2))
    put("P2X", O.f2_muls(q[0], O.XI_TO_PSQ_MINUS_1_OVER_3))

    def step(f, prog):
        G.run_xprogram(X[prog], regs, limbs=limbs)
        return O._mul_line(f, get("LA"), get("LB"), get("LC"))

    f = O.F12_ONE
    naf = O.SIX_U_PLUS_2_NAF
    n = len(naf)
    for i in range(n - 1, 0, -1):
        if i != n - 1:
            f = O.f12_sqr(f)
        f = step(f, "PDBL")
        if naf[i - 1]:
            f = step(f, "PADD_POS" if naf[i - 1] > 0 else "PADD_NEG")
    f = step(f, "PADD_F1")
    return step(f, "PADD_F2")


def test_team_programs_give_zero_on_order_13(pts, hs):
    for k in (1, 2, 5, 12):
        assert _is_zero12(team_miller(O.g2_mul(pts[13], k), hs[k % 2])), k


def test_team_programs_give_the_reference_pairing_elsewhere(pts, hs):
    """The projective lines differ from x/crypto's by Fp2 factors, which the
    final exponentiation removes as long as none of them is zero: so it does
    for a key of G2, for the other two small orders and for a twist point of
    large order outside G2."""
    keys = [O.g2_mul(O.G2_GEN, F.scalars(1, seed=b"team-miller")[0]), pts[7369], pts[95797],
            O.g2_mul(pts[95797], 2), F.non_g2_points(1, seed=5)[0]]
    for j, q in enumerate(keys):
        f = team_miller(q, hs[0])
        assert not _is_zero12(f), j
        assert O.final_exponentiation(f) == O.pair(hs[0], q), j


def test_team_programs_limb_for_limb_on_order_13(pts, hs):
    """The same loops on limb vectors (every reduction tail the kernels run)."""
    assert _is_zero12(team_miller(pts[13], hs[0], limbs=True))
    for q in (O.g2_mul(O.G2_GEN, F.scalars(1, seed=b"team-miller")[0]), pts[7369], pts[95797]):
        f = team_miller(q, hs[0], limbs=True)
        assert O.final_exponentiation(f) == O.pair(hs[0], q)
