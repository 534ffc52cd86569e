"""CPU suite of the random linear combination of independent checks on
arbitrary keys (include/handel_gpu.h: hg_verify_batch_rlc,
hg_verify_batch_msgs_rlc and their companions): the number
theory behind the G2 membership rule, the rule on the Python oracle and on the
compiled team programs' final registers, the ABI surface, the argument errors
and the register and LDS budgets of the new kernels. No GPU needed."""

import ctypes
import math
import os
import re
import sys

import pytest

from oracle import bn256_oracle as O
from tests import _fixtures as F

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tools"))
import gen_constants as C  # noqa: E402
import gen_g2_schedule as G  # noqa: E402

LIB = os.path.join(ROOT, "handel_amd", "_build", "libhandel_gpu.so")
P, N, U = O.P, O.ORDER, O.U
NEW_SYMBOLS = ("hg_verify_batch_rlc", "hg_verify_batch_rlc_device", "hg_verify_batch_msgs_rlc",
               "hg_verify_batch_msgs_rlc_device", "hg_batch_rlc_stats", "hg_debug_g2_member",
               "hg_debug_batch_rlc_groups")
HG_OK, HG_ERR_ARG = 0, 100


# ---------------------------------------------------------------- the number theory
def test_the_three_gcd_facts():
    """g(psi) = (6u+2) + psi - psi^2 + psi^3 reduced by psi^2 - t psi + p = 0 is
    a + b psi; its norm N = a^2 + a b t + b^2 p kills every Q with g(psi) Q = O.
    n | N, gcd(N / n, n h) = 1 and gcd(n, h) = 1 then give [n] Q = O."""
    t = 6 * U * U + 1
    h = 2 * P - N
    assert P + 1 - t == N  # the curve's trace
    # psi^2 = t psi - p; psi^3 = t psi^2 - p psi = (t^2 - p) psi - t p
    a = 6 * U + 2 + P - t * P
    b = 1 - t + t * t - P
    norm = a * a + a * b * t + b * b * P
    assert norm % N == 0
    assert math.gcd(norm // N, N * h) == 1
    assert math.gcd(N, h) == 1
    # the converse: on G2 psi acts as multiplication by p
    assert (6 * U + 2 + P - P * P + P ** 3) % N == 0


# ---------------------------------------------------------------- psi and its cube
def psi(q):
    return (O.f2_mul(O.f2_conj(q[0]), O.XI_TO_P_MINUS_1_OVER_3), O.f2_mul(O.f2_conj(q[1]), O.XI_TO_P_MINUS_1_OVER_2))


def psi3_by_constants(q):
    return (O.f2_mul(O.f2_conj(q[0]), C.PSI3[0]), O.f2_mul(O.f2_conj(q[1]), C.PSI3[1]))


def g2_key(j):
    return O.g2_mul(O.G2_GEN, F.scalars(3, seed=b"batch-rlc-host")[j])


def non_members():
    """(name, point): the three small orders, each plus a G2 key, four large-order points."""
    pts = F.small_order_points()
    out = [("order %d" % m, pts[m]) for m in F.SMALL_ORDERS]
    out += [("order %d + key" % m, O.g2_add(pts[m], g2_key(0))) for m in F.SMALL_ORDERS]
    out += [("large order %d" % j, q) for j, q in enumerate(F.non_g2_points(4))]
    return out


def test_psi3_constants_are_three_applications_of_the_map():
    header = open(os.path.join(ROOT, "handel_amd", "csrc", "bn256_constants.h")).read()
    assert "#define HG_PSI3 {" + ", ".join(C.f2_lit(g) for g in C.PSI3) + "}" in header
    assert [tuple(g) for g in C.GAMMA1] == [tuple(g) for g in O.GAMMA1]
    for q in [g2_key(0), O.G2_GEN] + [q for _, q in non_members()]:
        assert psi3_by_constants(q) == psi(psi(psi(q)))
        assert O.g2_on_curve(*psi(q))


def oracle_member(q):
    """[6u+2]Q + psi(Q) - psi^2(Q) == -psi^3(Q) with the oracle's complete group law."""
    r = O.g2_add(O.g2_mul(q, 6 * U + 2), psi(q))
    r = O.g2_add(r, O.g2_neg(psi(psi(q))))
    return r == O.g2_neg(psi(psi(psi(q))))


def test_the_rule_on_the_oracle():
    for j in range(3):
        q = g2_key(j)
        assert O.g2_in_subgroup(q) and oracle_member(q), j
    for name, q in non_members():
        assert O.g2_on_curve(*q) and not O.g2_in_subgroup(q), name
        assert not oracle_member(q), name


# ---------------------------------------------------------------- the team programs
X = None


def _programs():
    global X
    if X is None:
        X = G.compile_all()
    return X


def team_walk(q, limbs=False):
    """The G2 side of the pk Miller loop as the kernels run it
    (team_miller_check, bn256_pairing.h; tests/test_small_order_keys.py
    team_miller without f): R starts at (xi Qx, xi Qy, W = 1), every step is a
    compiled team program interpreted by run_xprogram. Returns the final X, Y
    and W registers as field elements."""
    Xp = _programs()
    h = O.hashed_message(F.LIB_MESSAGE)[0]
    rinv = pow(G.R_MONT, -1, P)
    enc = (lambda v: G.to_limbs(v * G.R_MONT % P)) if limbs else (lambda v: v % P)
    dec = (lambda l: G.from_limbs(l) * rinv % P) if limbs else (lambda v: v % P)
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
    naf = O.SIX_U_PLUS_2_NAF
    n = len(naf)
    for i in range(n - 1, 0, -1):
        G.run_xprogram(Xp["PDBL"], regs, limbs=limbs)
        if naf[i - 1]:
            G.run_xprogram(Xp["PADD_POS" if naf[i - 1] > 0 else "PADD_NEG"], regs, limbs=limbs)
    G.run_xprogram(Xp["PADD_F1"], regs, limbs=limbs)
    G.run_xprogram(Xp["PADD_F2"], regs, limbs=limbs)
    return get("X"), get("Y"), get("Z")


def team_member(q, limbs=False):
    """member(Q) <=> W != 0 and X == T.x xi W and Y == T.y xi W, T = -psi^3(Q)"""
    x, y, w = team_walk(q, limbs)
    t = O.g2_neg(psi3_by_constants(q))
    z = O.f2_mul_xi(w)
    return (not O.f2_is_zero(w)) and x == O.f2_mul(t[0], z) and y == O.f2_mul(t[1], z), w


def test_the_rule_on_the_team_programs():
    for j in range(3):
        ok, w = team_member(g2_key(j))
        assert ok and not O.f2_is_zero(w), j
    for name, q in non_members():
        ok, w = team_member(q)
        assert not ok, name
        # an exceptional step leaves W = 0 for good: the W != 0 term carries order 13's verdict
        assert O.f2_is_zero(w) == (name == "order 13"), name


def test_order_13_ends_with_w_zero_and_both_equalities_true():
    q = F.small_order_points()[13]
    x, y, w = team_walk(q)
    assert O.f2_is_zero(w)
    t = O.g2_neg(psi3_by_constants(q))
    z = O.f2_mul_xi(w)
    assert x == O.f2_mul(t[0], z) and y == O.f2_mul(t[1], z)  # 0 == 0: the comparisons alone would accept


def test_the_rule_limb_for_limb():
    """The same walks on limb vectors (every reduction tail the kernels run)."""
    ok, w = team_member(g2_key(1), limbs=True)
    assert ok and not O.f2_is_zero(w)
    ok, w = team_member(F.small_order_points()[13], limbs=True)
    assert not ok and O.f2_is_zero(w)


# ---------------------------------------------------------------- the ABI surface
def _lib():
    from handel_amd import _lib as B

    return B.load()


def test_header_declares_and_library_exports_the_entry_points():
    from handel_amd import _lib as B

    header = open(os.path.join(ROOT, "include", "handel_gpu.h")).read()
    L = _lib()
    for name in NEW_SYMBOLS:
        assert re.search(r"\bint\s+%s\s*\(" % name, header), name
        assert hasattr(L, name) and name in B.SIGNATURES, name


def test_bindings_go_and_documents_mirror_the_calls():
    from handel_amd.engine import Engine

    for name in ("verify_batch_rlc", "verify_batch_msgs_rlc", "g2_members", "batch_rlc_stats"):
        assert callable(getattr(Engine, name)), name
    go = open(os.path.join(ROOT, "go", "bn256", "hip", "engine.go")).read()
    doc = open(os.path.join(ROOT, "INTEGRATION.md")).read()
    for name in ("hg_verify_batch_rlc", "hg_verify_batch_msgs_rlc"):
        assert re.search(r"C\.%s\(" % name, go), name
        assert name in doc, name
    assert "hg_batch_rlc_stats" in doc
    from handel_amd import build as BLD

    assert {"bn256_batchrlc.hip", "hg_batch_rlc.cpp"} <= set(BLD.SOURCES)


def test_argument_errors_without_gpu():
    L = _lib()
    seed = bytes(range(32))
    buf = ctypes.create_string_buffer(256)
    # a context that is never read: the seed and the group are checked first
    ctx = ctypes.cast(ctypes.create_string_buffer(64), ctypes.c_void_p)
    for fn, args in (
        (L.hg_verify_batch_rlc, lambda c, sd, g: (c, buf, buf, 1, sd, g, buf)),
        (L.hg_verify_batch_rlc_device, lambda c, sd, g: (c, buf, buf, 1, sd, g, buf, None)),
        (L.hg_verify_batch_msgs_rlc, lambda c, sd, g: (c, buf, 1, buf, buf, buf, buf, 1, sd, g, buf)),
        (L.hg_verify_batch_msgs_rlc_device, lambda c, sd, g: (c, buf, 1, buf, buf, buf, buf, 1, sd, g, buf, None)),
    ):
        assert fn(*args(ctx, seed, 0)) == HG_ERR_ARG        # group == 0
        assert fn(*args(ctx, seed, 4097)) == HG_ERR_ARG     # group > 4096
        assert fn(*args(ctx, None, 64)) == HG_ERR_ARG       # NULL seed
        assert fn(*args(None, seed, 64)) == HG_ERR_ARG      # NULL context
    assert L.hg_verify_batch_rlc(ctx, None, buf, 1, seed, 64, buf) == HG_ERR_ARG
    assert L.hg_verify_batch_msgs_rlc(ctx, None, 1, buf, buf, buf, buf, 1, seed, 64, buf) == HG_ERR_ARG  # no pool
    assert L.hg_verify_batch_msgs_rlc(ctx, buf, 1, None, buf, buf, buf, 1, seed, 64, buf) == HG_ERR_ARG
    groups = lambda c, g, off, ln: (c, buf, 1, off, ln, buf, buf, 1, buf, g, buf, buf, buf)  # noqa: E731
    assert L.hg_debug_batch_rlc_groups(*groups(ctx, 0, buf, buf)) == HG_ERR_ARG
    assert L.hg_debug_batch_rlc_groups(*groups(ctx, 4097, buf, buf)) == HG_ERR_ARG
    assert L.hg_debug_batch_rlc_groups(*groups(None, 3, buf, buf)) == HG_ERR_ARG
    assert L.hg_debug_batch_rlc_groups(*groups(ctx, 3, buf, None)) == HG_ERR_ARG  # offsets without lengths
    assert L.hg_debug_batch_rlc_groups(ctx, None, 0, None, None, None, None, 0, None, 3, None, None, None) == HG_OK
    assert L.hg_debug_g2_member(None, buf, 1, buf, buf) == HG_ERR_ARG
    assert L.hg_debug_g2_member(ctx, buf, 1, None, buf) == HG_ERR_ARG
    assert L.hg_debug_g2_member(ctx, None, 0, None, None) == HG_OK  # n == 0: nothing read
    assert L.hg_batch_rlc_stats(None, None, None, None, None) == HG_ERR_ARG


def test_coefficients_are_the_aggregate_calls():
    """seed and r_i as hg_verify_aggregate_rlc: the host rule, by the code the device runs."""
    import hashlib

    import numpy as np

    L = _lib()
    seed = bytes(range(32))
    out = np.zeros(5, dtype=np.uint64)
    assert L.hg_debug_rlc_coeffs(seed, 0, 5, out.ctypes.data_as(ctypes.c_void_p)) == HG_OK
    for i in range(5):
        d = hashlib.sha256(b"hg-rlc-v1" + seed + i.to_bytes(8, "little")).digest()
        assert int(out[i]) == (int.from_bytes(d[:8], "little") or 1)


# ---------------------------------------------------------------- kernel resources
# k_brlc_miller is k_mrlc_miller's body and the rule: k_verify_ml<4>'s budget
# (tests/test_kernel_resources.py: layout V, 20480 bytes of LDS, at most 256
# VGPRs for two waves per SIMD, no scratch)
BUDGETS = {"k_brlc_miller": 20480}
OTHERS = ("k_brlc_one_message", "k_brlc_members", "k_brlc_probe_checks")


@pytest.fixture(scope="module")
def res():
    if not os.path.exists(LIB):
        pytest.skip("libhandel_gpu.so not built")
    import kernel_sizes

    r = kernel_sizes.resources(LIB)
    if not r:
        pytest.skip("no gfx950 code object metadata found")
    return r


def _one(res, part):
    hits = {k: v for k, v in res.items() if part in k}
    assert len(hits) == 1, (part, sorted(hits))
    return next(iter(hits.values()))


@pytest.mark.parametrize("part", tuple(BUDGETS) + OTHERS)
def test_kernels_keep_their_budgets(res, part):
    r = _one(res, part)
    assert r["vgpr_spill"] == 0 and r["sgpr_spill"] == 0 and r["scratch"] == 0, (part, r)
    if part in BUDGETS:
        assert r["lds"] == BUDGETS[part] and r["vgpr"] <= 256, (part, r)


def test_every_new_kernel_is_listed(res):
    names = {k for k in res if "k_brlc_" in k}
    assert len(names) == len(BUDGETS) + len(OTHERS), sorted(names)
    for k in names:
        r = res[k]
        assert r["vgpr_spill"] == 0 and r["sgpr_spill"] == 0 and r["scratch"] == 0, (k, r)
