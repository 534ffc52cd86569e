"""CPU suite: two consecutive G2Base lines as one factor (PairCoef,
bn256_kernels.h; the generator's LINE2_FIX_12; team_miller_sig12).

With the oracle's arithmetic: the 85 normalised line coefficients and the 19
pairs of lines that follow each other with nothing between (the doubling's and
the addition's line of a nonzero NAF digit, the two Frobenius lines); the five
constants of a pair, the five scalars of a signature, and

    L = L0 + L1 w + L2 w^2 + y' w^3 + L4 w^4 = la lb / K3,

at random G1 points and with the scalars x = y' = 0 of a signature at
infinity (L = xi / K3, an Fp2 constant). The Miller value with the pairs fused and f seeded with
the first line differs from the line-by-line one by an Fp2 factor, so both
final exponentiations give the same value. LINE2_FIX_12 itself runs through
the generator's residue and limb interpreters on the edge regions of
tests/test_xinst_edges.py and on real operands against the oracle's product.
"""

import functools
import os
import random
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tools"))
sys.path.insert(0, ROOT)

import gen_g2_schedule as G  # noqa: E402
from oracle import bn256_oracle as O  # noqa: E402
from tests import test_xinst_edges as E  # noqa: E402
from tests.test_oracle import _g2base_lines_normalised, _miller_normalised  # noqa: E402

P = O.P
XI = (1, 3)  # i + 3
NUM_LINES, NUM_PAIRS = 85, 19


@functools.lru_cache(maxsize=None)
def line_coefs():
    """[(bx, cy)] of the 85 lines: the normalised lines at (1, 1)."""
    out = [(b, c) for _, (_, (b, c)) in _g2base_lines_normalised((1, 1))]
    assert len(out) == NUM_LINES
    return out


@functools.lru_cache(maxsize=None)
def pair_starts():
    """First line of every pair, in loop order (k_g2_lines' walk)."""
    naf = O.SIX_U_PLUS_2_NAF
    s, out = 0, []
    for i in range(len(naf) - 1, 0, -1):
        if naf[i - 1]:
            out.append(s)
            s += 1
        s += 1
    out.append(s)  # the two Frobenius lines
    assert s == NUM_LINES - 2 and len(out) == NUM_PAIRS
    return out


def pair_k(a):
    """K0, K1, K2, K3, K4 of the pair of lines a, a + 1."""
    (bxa, cya), (bxb, cyb) = line_coefs()[a], line_coefs()[a + 1]
    return (O.f2_mul(cya, cyb), O.f2_add(O.f2_mul(cya, bxb), O.f2_mul(bxa, cyb)), O.f2_mul(bxa, bxb),
            O.f2_add(cya, cyb), O.f2_add(bxa, bxb))


def pair_record(a):
    """PairCoef: K0 / K3, xi / K3, K1 / K3, K2 / K3, K4 / K3."""
    k0, k1, k2, k3, k4 = pair_k(a)
    inv3 = O.f2_inv(k3)
    return tuple(O.f2_mul(v, inv3) for v in (k0, XI, k1, k2, k4))


def scalars(pt):
    """k_sig_scalars: x, y', y'^2, x y', x^2 of the evaluation point (x, y');
    all 0 for None (a signature at infinity or one that fails to decode)."""
    x, y = (0, 0) if pt is None else pt
    return (x, y, y * y % P, x * y % P, x * x % P)


def pair_value(rec, sc):
    """L from a pair's constants and a signature's scalars (k_sig_lines)."""
    k0, xi, k1, k2, k4 = rec
    x, y, y2, xy, x2 = sc
    return [O.f2_add(O.f2_muls(k0, y2), xi), O.f2_muls(k1, xy), O.f2_muls(k2, x2), (0, y), O.f2_muls(k4, x),
            O.F2_ZERO]


def line_value(s, sc):
    bx, cy = line_coefs()[s]
    return [O.f2_muls(cy, sc[1]), O.f2_muls(bx, sc[0]), O.F2_ZERO, O.F2_ONE, O.F2_ZERO, O.F2_ZERO]


def f12_scale(f, k):
    return [O.f2_mul(c, k) for c in f]


def miller_fused(sc):
    """team_miller_sig12: f = line 0, then per digit f^2 and f * line, or
    f * pair on a nonzero digit, then the Frobenius pair."""
    naf = O.SIX_U_PLUS_2_NAF
    starts = set(pair_starts())
    f = line_value(0, sc)
    s = 1
    for i in range(len(naf) - 2, 0, -1):
        f = O.f12_sqr(f)
        if naf[i - 1]:
            assert s in starts
            f = O.f12_mul(f, pair_value(pair_record(s), sc))
            s += 2
        else:
            assert s not in starts
            f = O.f12_mul(f, line_value(s, sc))
            s += 1
    assert s == NUM_LINES - 2
    return O.f12_mul(f, pair_value(pair_record(s), sc))


def points():
    rng = random.Random(1905)
    return [O.g1_neg(O.g1_mul(O.G1_GEN, rng.randrange(1, O.ORDER))) for _ in range(3)]


def test_first_digit_has_a_line_of_its_own():
    """f is seeded with line 0 alone: the NAF's first digit after the leading one is 0."""
    naf = O.SIX_U_PLUS_2_NAF
    assert naf[-1] == 1 and naf[-2] == 0 and 0 not in pair_starts()
    assert sum(1 for d in naf[:-1] if d) == NUM_PAIRS - 1


def test_no_pair_loses_its_w3_coefficient():
    for a in pair_starts():
        assert pair_k(a)[3] != O.F2_ZERO, a
        assert pair_record(a)[1] != O.F2_ZERO, a  # what hg_create looks at


def test_pair_value_is_the_product_of_its_lines():
    for pt in points():
        sc = scalars(pt)
        assert sc[1] != 0  # G1 has prime order: no finite point with y = 0
        for a in pair_starts():
            want = O.f12_mul(line_value(a, sc), line_value(a + 1, sc))
            k3 = pair_k(a)[3]
            assert want[3] == O.f2_muls(k3, sc[1]) and want[5] == O.F2_ZERO
            assert f12_scale(pair_value(pair_record(a), sc), k3) == want, a
    zero = scalars(None)
    for a in pair_starts():  # at infinity: the nonzero Fp2 constant xi / K3
        rec = pair_record(a)
        assert pair_value(rec, zero) == [rec[1]] + [O.F2_ZERO] * 5 and rec[1] != O.F2_ZERO, a


def test_fused_miller_value_differs_by_an_fp2_factor():
    for pt in points()[:2]:
        fused = miller_fused(scalars(pt))
        plain = _miller_normalised(pt)
        ratio = O.f12_mul(plain, O.f12_inv(fused))
        assert ratio[0] != O.F2_ZERO and all(c == O.F2_ZERO for c in ratio[1:]), "not an Fp2 factor"
        assert O.final_exponentiation(fused) == O.final_exponentiation(plain) == O.pair(pt, O.G2_GEN)
        assert O.final_exponentiation_fc(fused) == O.final_exponentiation_fc(plain)


def test_fused_miller_value_at_infinity_reduces_to_one():
    fused = miller_fused(scalars(None))
    assert O.final_exponentiation(fused) == O.F12_ONE
    assert O.final_exponentiation_fc(fused) == O.F12_ONE


# ------------------------------------------------------------------ the team program
LINE2 = ("LINE2_FIX_12", ("F", "F"), "T")


def line2_entry():
    """The pair product's bound instance: the generator keeps it in
    PAIR_INSTANCES (ALL_INSTANCES numbers the probe's 145 cases), entry
    len(ALL_INSTANCES) of PROBE_INSTANCES and of instance_rounds, probe instance
    PROBE_EXTRA_BASE on the GPU."""
    assert G.PAIR_INSTANCES == [LINE2] and G.PROBE_INSTANCES == G.ALL_INSTANCES + G.PAIR_INSTANCES
    assert LINE2 in G.BOUND_INSTANCES and G.BOUND_INSTANCES[-1] == G.ALL_INSTANCES[-1]
    return len(G.ALL_INSTANCES)


def line2_round():
    (bx,) = G.instance_rounds(E.programs(), line2_entry())
    return bx


def line2_cases():
    """The thirteen edge regions tests/test_xinst_edges.py build_cases gives
    every numbered instance, for this one (layout T, a two-slot binding: the
    structured cases hold the registers of a real step and the element one),
    and a fourteenth with every element at the limb bound check_xround
    assumes."""
    n = E.region_elems()["T"]
    fb = G.probe_reg_base(LINE2[0], "T")
    rng = random.Random(E.SEED * 1000 + line2_entry())
    cases = [("all 2p-1", [G.to_limbs(2 * P - 1) for _ in range(n)]),
             ("all p-1", [G.to_limbs(P - 1) for _ in range(n)]),
             ("all 0", [G.to_limbs(0) for _ in range(n)]),
             ("all p", [G.to_limbs(P) for _ in range(n)]),
             ("alternating limbs", [E._alternating(e) for e in range(n)])]
    for k in range(4):
        mem = []
        for _ in range(n):
            c = rng.randrange(len(E.EDGE_VALUES) + 1)
            mem.append(G.to_limbs(E.EDGE_VALUES[c] if c < len(E.EDGE_VALUES) else rng.randrange(2 * P)))
        cases.append((f"edge draw {k}", mem))
    for k in range(2):
        cases.append((f"canonical {k}", [G.to_limbs(rng.randrange(P)) for _ in range(n)]))
    res = [rng.randrange(P) for _ in range(n)]
    for r, v in E._real_values()[0].items():
        if fb + r < n:
            res[fb + r] = v
    res[0:12] = [0, 1] + [0] * 10
    cases.append(("structured", [E.mont(v) for v in res]))
    cases.append(("structured lazy", [G.to_limbs(v * G.R_MONT % P + P) for v in res]))
    assert len(cases) == E.NCASES
    # (limb for limb the largest operand the generator admits; as a value just above 2p - 1)
    cases.append(("limb bound", [list(G.LAZY_LIMB) for _ in range(n)]))
    for name, mem in cases:
        mem[fb + G.REG["ZERO"]] = G.to_limbs(0)
        mem[fb + G.REG["ONE"]] = E.mont(1)
        assert all(max(l[:9]) <= G.MASK26 and l[9] <= G.LAZY_LIMB[9] for l in mem)
        assert name == "limb bound" or all(G.from_limbs(l) < 2 * P for l in mem)
    return cases


@functools.lru_cache(maxsize=None)
def line2_runs():
    """Every case through the limb model, once per session (the GPU test
    compares the probe with mem_out)."""
    return [E.run_model(line2_entry(), case, mem) for case, mem in line2_cases()]


def test_line2_round_shape():
    """One round: eighteen pre-pass values on lanes 0..11 (at most two per
    lane), 9 Karatsuba products per lane, no linear term (the plain REDC and
    its rare subtraction); inside layout T's region as it was."""
    (xr,) = E.programs()["LINE2_FIX_12"]
    assert (xr.nv, xr.nt, xr.np, xr.nl) == (2, 2, 9, 0)
    assert xr.ks1 == 1 and not xr.one_chain and xr.lz == 0 and xr.kp >= 0
    assert sum(1 for L in xr.lanes[:12] for d, _ in L["pre"] if d != G.NONE) == 18
    assert all(d == G.NONE for L in xr.lanes[12:] for d, _ in L["pre"])
    assert E.region_elems()["T"] == 92
    assert line2_entry() == 145
    assert G.touched(line2_round()) < 92


def test_line2_limb_model_at_the_edges():
    """The cases of tests/test_xinst_edges.py and the limb bound: the limb interpreter raises
    nothing, agrees with the residue interpreter, keeps its results canonical
    and leaves every other element alone."""
    runs = line2_runs()
    assert len(runs) == E.NCASES + 1
    for run in runs:
        rounds = [xr for xr, _, _ in run.rounds]
        res = [G.from_limbs(l) * E.RINV % P for l in run.mem_in]
        G.run_bound(rounds, res)
        written = set()
        for xr, pre, out in run.rounds:
            written |= set(pre) | set(out)
            assert len(out) == 12
            for d, l in out.items():
                assert max(l[:9]) <= G.MASK26 and G.from_limbs(l) < P, (run.case, d)
        for e, (a, b, v) in enumerate(zip(run.mem_in, run.mem_out, res)):
            assert G.from_limbs(b) * E.RINV % P == v, (run.case, e)
            assert e in written or a == b, (run.case, e)
        assert run.subs["csub_rare"][0] == 12 and run.subs["redq"][0] == 0
    assert sum(run.subs["csub_rare"][1] for run in runs) >= 1, "no case takes the rare subtraction"


@pytest.mark.parametrize("lazy", [False, True], ids=["canonical", "lazy"])
def test_line2_limb_interpreter_matches_oracle(lazy):
    """Real operands: f (canonical, or the same residues in [p, 2p)) times a
    pair built from the table's constants and a signature's scalars."""
    rng = random.Random(f"line2{lazy}")
    bx = line2_round()
    fb = G.SIG_T_F_BASE
    res = [rng.randrange(P) for _ in range(fb + G.NREGS)]
    res[fb + G.REG["ZERO"]] = 0
    res[fb + G.REG["ONE"]] = 1
    f = [(rng.randrange(P), rng.randrange(P)) for _ in range(6)]
    res[0:12] = [z for pair in f for z in pair]
    L = pair_value(pair_record(pair_starts()[3]), scalars(points()[0]))
    res[fb + G.REG["NSY"]] = L[3][1]
    for name, v in zip(G.LINE2_REGS, (L[0], L[1], L[2], L[4])):
        res[fb + G.comp(name, "x")], res[fb + G.comp(name, "y")] = v
    mem = [G.to_limbs(v * G.R_MONT % P) for v in res]
    if lazy:
        mem[0:12] = [G.to_limbs(v * G.R_MONT % P + P) for v in res[0:12]]
    G.run_bound_limbs([bx], mem)
    vals = [G.from_limbs(mem[e]) for e in range(12)]
    assert all(v < P for v in vals)
    got = [(vals[2 * k] * E.RINV % P, vals[2 * k + 1] * E.RINV % P) for k in range(6)]
    assert got == O.f12_mul(f, L)


def test_line2_limb_interpreter_at_every_lanes_bound():
    """Every operand at the limb bound check_xround assumes: every pre-pass
    sum, column and quotient at its largest admitted value."""
    bx = line2_round()
    fb = G.SIG_T_F_BASE
    mem = [list(G.LAZY_LIMB) for _ in range(fb + G.NREGS)]
    mem[fb + G.REG["ZERO"]] = G.to_limbs(0)
    mem[fb + G.REG["ONE"]] = G.to_limbs(G.R_MONT % P)
    res = [G.from_limbs(l) * E.RINV % P for l in mem]
    G.run_bound([bx], res)
    G.run_bound_limbs([bx], mem)
    for e in range(12):
        v = G.from_limbs(mem[e])
        assert v < P and v * E.RINV % P == res[e], e
