"""CPU suite: the GT fold's torus form (tools/gen_g2_schedule.py TORMULF,
handel_amd/csrc/bn256_gt.hip k_tor_chunks / k_tor_compare_bits).

A unitary g = a + b w (a, b in Fp6, w^2 = v) equals (alpha + w)/(alpha - w)
with alpha = (1 + a)/b, and a running product is any X in Fp12 with value
X/conj(X). These tests run the generated program — the compiled rounds on
residues and the bound instance limb for limb — against the oracle's Fp12
arithmetic for random unitary g and random X, and check the identities the
kernels rest on: -alpha is the conjugate, an Fp6 factor of X does not change
its value, values multiply, and fe conj(X) == X exactly when fe == X/conj(X).
"""

import os
import random
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tools"))

import gen_g2_schedule as G  # noqa: E402
from oracle import bn256_oracle as O  # noqa: E402

P = G.P
ZERO2, ONE2 = (0, 0), (0, 1)


def _rand12(rng):
    return [(rng.randrange(P), rng.randrange(P)) for _ in range(6)]


def _embed6(c):
    """An Fp6 element (three Fp2 coefficients of 1, v, v^2) in Fp12: v = w^2."""
    return [c[0], ZERO2, c[1], ZERO2, c[2], ZERO2]


def _unitary(rng):
    f = _rand12(rng)
    g = O.f12_mul(O.f12_conj(f), O.f12_inv(f))
    assert O.f12_mul(g, O.f12_conj(g)) == [ONE2] + [ZERO2] * 5
    return g


def _alpha(g):
    """alpha = (1 + a)/b of g = a + b w, as three Fp2 coefficients."""
    a = [g[0], g[2], g[4]]
    b = [g[1], g[3], g[5]]
    a1 = [((a[0][0]) % P, (a[0][1] + 1) % P), a[1], a[2]]
    q = O.f12_mul(_embed6(a1), O.f12_inv(_embed6(b)))
    assert q[1] == q[3] == q[5] == ZERO2  # Fp6 is closed
    return [q[0], q[2], q[4]]


def _alpha_w(al):
    return [al[0], ONE2, al[1], ZERO2, al[2], ZERO2]


def _value(x):
    return O.f12_mul(x, O.f12_inv(O.f12_conj(x)))


def _flat(v):
    return [z for pair in v for z in pair]


def _unflat(d):
    return [(d[2 * k], d[2 * k + 1]) for k in range(6)]


def _neg6(al):
    return [((-x) % P, (-y) % P) for x, y in al]


@pytest.fixture(scope="module")
def prog():
    rounds = [G.compile_round(r, f"TORMULF[{i}]", G.SCRATCH_CAP["FOLD"], pre_lanes=G.PRE_LANES["TORMULF"],
                              ks_min=G.KARATSUBA_MIN_PROG["TORMULF"])
              for i, r in enumerate(G.PROGRAMS["TORMULF"])]
    return rounds


def _run(prog, x, al, junk):
    F = {G.REG["ZERO"]: 0, G.REG["ONE"]: 1}
    return _unflat(G.run_xprogram(prog, F, _flat(x), _flat(al) + junk))


def test_conj_is_w_to_minus_w():
    f = _rand12(random.Random(1))
    c = O.f12_conj(f)
    assert [c[k] for k in (0, 2, 4)] == [f[k] for k in (0, 2, 4)]
    assert [c[k] for k in (1, 3, 5)] == [((-x) % P, (-y) % P) for x, y in (f[1], f[3], f[5])]


def test_alpha_represents_g():
    rng = random.Random(2)
    for _ in range(3):
        g = _unitary(rng)
        al = _alpha(g)
        assert _value(_alpha_w(al)) == g
        assert _value(_alpha_w(_neg6(al))) == O.f12_conj(g)  # the conjugate (= inverse) is -alpha


def test_program_shape(prog):
    (xr,) = prog
    # six products per lane (MUL12F: twelve), one R-shifted linear group, one
    # reduction; every pre-pass value on lanes 0..11 (12-lane teams)
    assert (xr.np, xr.nv, xr.np2, xr.nl2) == (6, 1, 0, 0) and xr.nl >= 1
    assert xr.ks1 == 1 and not xr.one_chain and not xr.lz
    assert all(d == G.NONE for L in xr.lanes[12:] for d, _ in L["pre"])
    assert all(L["dst"] != G.NONE for L in xr.lanes[:12]) and all(L["dst"] == G.NONE for L in xr.lanes[12:])


def test_program_multiplies_values(prog):
    rng = random.Random(3)
    for _ in range(4):
        g, x = _unitary(rng), _rand12(rng)
        al = _alpha(g)
        junk = [rng.randrange(P) for _ in range(6)]  # elements 6..11 of slot B are never read
        x1 = _run(prog, x, al, junk)
        assert x1 == O.f12_mul(x, _alpha_w(al))
        assert _value(x1) == O.f12_mul(_value(x), g)
        # conjugated operand: -alpha
        xc = _run(prog, x, _neg6(al), junk)
        assert _value(xc) == O.f12_mul(_value(x), O.f12_conj(g))
        # an Fp6 factor of X leaves the value alone
        s = _embed6([(rng.randrange(P), rng.randrange(P)) for _ in range(3)])
        xs = _run(prog, O.f12_mul(x, s), al, junk)
        assert xs == O.f12_mul(x1, s) and _value(xs) == _value(x1)


def test_first_term_and_chain(prog):
    """k_tor_chunks' chain: X = +-alpha_0 + w, then one program run per term;
    partial products combine by the plain Fp12 product."""
    rng = random.Random(4)
    gs = [_unitary(rng) for _ in range(5)]
    conj = [True, False, True, True, False]
    want = O.f12_conj(gs[0]) if conj[0] else gs[0]
    x = _alpha_w(_neg6(_alpha(gs[0])) if conj[0] else _alpha(gs[0]))
    for g, c in list(zip(gs, conj))[1:3]:
        x = _run(prog, x, _neg6(_alpha(g)) if c else _alpha(g), [0] * 6)
        want = O.f12_mul(want, O.f12_conj(g) if c else g)
    y = _alpha_w(_neg6(_alpha(gs[3])))
    y = _run(prog, y, _alpha(gs[4]), [0] * 6)
    want = O.f12_mul(want, O.f12_mul(O.f12_conj(gs[3]), gs[4]))
    assert _value(O.f12_mul(x, y)) == want


def test_comparison_identity():
    rng = random.Random(5)
    for _ in range(3):
        x = _rand12(rng)
        fe = _value(x)
        assert O.f12_mul(fe, O.f12_conj(x)) == x
        other = _unitary(rng)
        assert other != fe and O.f12_mul(other, O.f12_conj(x)) != x


def test_bound_instance_limb_for_limb(prog):
    """The FOLD-region instance k_tor_chunks runs, on Montgomery limbs with the
    reduction tail, for a unitary entry's alpha and its negation."""
    rng = random.Random(6)
    assert G.ALL_INSTANCES[-1] == ("TORMULF", ("A", "A", "B"), "")
    rounds = [G.bind(xr, ("A", "A", "B"), "FOLD") for xr in prog]
    fb = G.F_BASE_CTX["FOLD"]
    assert max(G.touched(b) for b in rounds) < G.REGION_END["FOLD"]
    rinv = pow(G.R_MONT, -1, P)
    for neg in (False, True):
        g, x = _unitary(rng), _rand12(rng)
        al = _neg6(_alpha(g)) if neg else _alpha(g)
        mem = [rng.randrange(P) for _ in range(G.REGION_END["FOLD"])]
        mem[fb + G.REG["ZERO"]], mem[fb + G.REG["ONE"]] = 0, 1
        mem[12:24] = _flat(x)
        mem[24:30] = _flat(al)
        lmem = [G.to_limbs(v * G.R_MONT % P) for v in mem]
        G.run_bound_limbs(rounds, lmem)
        got = [G.from_limbs(l) * rinv % P for l in lmem[12:24]]
        assert _unflat(got) == O.f12_mul(x, _alpha_w(al))
        assert all(G.from_limbs(l) < P for l in lmem[12:24])  # canonical: the comparison is on words


def test_fold_region_and_other_tables_unchanged():
    """The new instance fits the fold kernels' team region as it was (60
    elements: 12 000 B per five-team workgroup) and is listed last, so no other
    instance's table moves."""
    text = open(os.path.join(ROOT, "handel_amd", "csrc", "bn256_xtab.h")).read()
    assert "kFoldTeamElems = 60;" in text
    assert "kSigTTeamElems = 92;" in text
    assert text.rstrip().splitlines()[-2].startswith("template <> struct XInst<XP_TORMULF, S_A, S_A, S_B>")
