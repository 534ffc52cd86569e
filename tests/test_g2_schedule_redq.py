"""The one-chain reduction of the 12-lane programs' linear-term rounds in the
generator (tools/gen_g2_schedule.py ONE_CHAIN_PROGRAMS, check_one_chain,
xround_limbs): every layout-T instance of CYC_SQR_X_12 and LINE_FIX_12,
interpreted limb for limb with the tail the emitter selects
(XQ<QMAX>::x_round, bn256_redq.h), gives the oracle's Fp12 result on random
inputs (canonical and lazy) and the residue interpreter's on inputs whose
every limb sits at the generator's bound; the emitted QMAX is at least the
bound recomputed here from the compiled lanes; and only those two programs
carry one.
"""

import os
import random
import re
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tools"))
sys.path.insert(0, ROOT)
import gen_g2_schedule as G  # noqa: E402
from oracle import bn256_oracle as O  # noqa: E402

P = G.P
RM = G.R_MONT
RINV = pow(RM, -1, P)
PROGRAMS = ("CYC_SQR_X_12", "LINE_FIX_12")
T_INSTANCES = [(n, b) for n, b, lay in G.ALL_INSTANCES if lay == "T" and n in PROGRAMS]


@pytest.fixture(scope="module")
def compiled():
    return G.compile_all()


@pytest.fixture(scope="module")
def emitted(compiled, tmp_path_factory):
    """(program, layout, binding) -> per round (QMAX or None, x_round's template arguments)"""
    path = tmp_path_factory.mktemp("xtab") / "bn256_xtab.h"
    G.emit_x(compiled, str(path))
    out = {}
    for m in re.finditer(r"struct XInst<XP_(\w+?)(?:_([STV]))?((?:, S_\w)*)> \{(.*?)\} \};", path.read_text()):
        rounds = [(int(q) if q else None, tuple(int(v) for v in r.split(",")))
                  for q, r in re.findall(r"(?:XQ<(\d+)>::)?x_round<([^>]*)>", m.group(4))]
        out[(m.group(1), m.group(2) or "", tuple(re.findall(r"S_(\w)", m.group(3))))] = rounds
    return out


def mont(v, lazy=False):
    return G.to_limbs(v * RM % P + (P if lazy else 0))


def test_instances_cover_both_programs():
    assert {n for n, _ in T_INSTANCES} == set(PROGRAMS)
    assert set(G.ONE_CHAIN_PROGRAMS) == set(PROGRAMS)


@pytest.mark.parametrize("name,binding", T_INSTANCES, ids=[f"{n}-{''.join(b)}" for n, b in T_INSTANCES])
@pytest.mark.parametrize("lazy", [False, True], ids=["canonical", "lazy"])
def test_limb_interpreter_matches_oracle(compiled, name, binding, lazy):
    rng = random.Random(f"redq{name}{binding}{lazy}")
    rounds = [G.bind(xr, binding, G.X_PROGRAMS[name], "T") for xr in compiled[name]]
    assert all(bx.one_chain and bx.qmax >= 1 for bx in rounds if bx.nl > 0)
    assert [bx.lz for bx in rounds] == [int(name == "CYC_SQR_X_12" and bx.nl > 0) for bx in rounds]
    fb = G.SIG_T_F_BASE
    res = [rng.randrange(P) for _ in range(fb + G.NREGS)]
    res[fb + G.REG["ZERO"]] = 0
    res[fb + G.REG["ONE"]] = 1
    f = [(rng.randrange(P), rng.randrange(P)) for _ in range(6)]
    if name == "CYC_SQR_X_12":  # an element of the cyclotomic subgroup
        f = O.f12_mul(O.f12_conj(f), O.f12_inv(f))
        f = O.f12_mul(f, O.f12_frob2(f))
    D, A = binding
    a0 = 12 * G.SLOTS.index(A)
    res[a0:a0 + 12] = [z for pair in f for z in pair]
    mem = [mont(v) for v in res]
    mem[a0:a0 + 12] = [mont(v, lazy) for v in res[a0:a0 + 12]]  # lazy: the same residues in [p, 2p)
    if name == "LINE_FIX_12":
        lb, lc = [(res[fb + G.comp(n, "x")], res[fb + G.comp(n, "y")]) for n in ("FB", "FC")]
        want = O._mul_line(f, O.F2_ONE, lb, lc)
    else:
        want = O.f12_sqr(f)
    G.run_bound_limbs(rounds, mem)
    d0 = 12 * G.SLOTS.index(D)
    vals = [G.from_limbs(mem[d0 + e]) for e in range(12)]
    assert all(v < (2 * P if name == "CYC_SQR_X_12" else P) for v in vals), "the representative's range"
    got = [(vals[2 * k] * RINV % P, vals[2 * k + 1] * RINV % P) for k in range(6)]
    assert got == want, (name, binding)


@pytest.mark.parametrize("name,binding", T_INSTANCES, ids=[f"{n}-{''.join(b)}" for n, b in T_INSTANCES])
def test_limb_interpreter_at_every_lanes_bound(compiled, name, binding):
    """Every operand at the limb bound check_xround assumes (LAZY_LIMB: nine
    limbs of 2^26 - 1 under the top limb of 2p - 1), which drives every
    pre-pass sum, column and quotient to its largest admitted value: the model
    asserts every register width and the result's range on the way, and the
    result is the residue interpreter's."""
    rounds = [G.bind(xr, binding, G.X_PROGRAMS[name], "T") for xr in compiled[name]]
    fb = G.SIG_T_F_BASE
    mem = [list(G.LAZY_LIMB) for _ in range(fb + G.NREGS)]
    mem[fb + G.REG["ZERO"]] = G.to_limbs(0)
    mem[fb + G.REG["ONE"]] = mont(1)
    res = [G.from_limbs(l) * RINV % P for l in mem]
    G.run_bound(rounds, res)
    G.run_bound_limbs(rounds, mem)
    d0 = 12 * G.SLOTS.index(binding[0])
    for e in range(12):
        v = G.from_limbs(mem[d0 + e])
        assert v < (2 * P if name == "CYC_SQR_X_12" else P) and v * RINV % P == res[d0 + e], (name, binding, e)


@pytest.mark.parametrize("name", PROGRAMS)
def test_emitted_qmax_covers_the_recomputed_bound(compiled, emitted, name):
    """V < sum(products) / R + linear terms + p, with every element below 2p,
    every negated term 4p - x <= 4p (its correction K (4p)'' counted whole) and
    every pre-pass value bounded the same way."""
    two_p = 2 * P
    for key, rounds in emitted.items():
        if key[0] != name or key[1] != "T":
            continue
        assert len(rounds) == len(compiled[name])
        for (q, targs), xr in zip(rounds, compiled[name]):
            assert len(targs) == 15
            if xr.nl == 0:
                assert q is None
                continue
            assert xr.kp >= 0 and xr.kl1 >= 0, "round-uniform corrections"
            vb = {}
            for L in xr.lanes:
                for d, terms in L["pre"]:
                    if d != G.NONE:
                        vb[d] = xr.kp * 4 * P + sum(k * two_p for _, k in terms if k > 0)
            need = 0
            for L in xr.lanes:
                prod = sum(vb.get(u, two_p) * vb.get(v, two_p) for u, v in L["prod"])
                lin = xr.kl1 * 4 * P + sum(k * two_p for _, k in L["lin"] if k > 0)
                bound = -(-prod // RM) + lin + P           # V < bound
                need = max(need, (bound - 1) // P)         # floor(V / p) <= need
            assert q is not None and q >= need and q == xr.qmax, (key, q, need)
            assert q <= G.ONE_CHAIN_QMAX_LIMIT


def test_only_the_12_lane_linear_rounds_carry_a_qmax(emitted):
    for key, rounds in emitted.items():
        for q, targs in rounds:
            nl = targs[3]
            assert (q is not None) == (key[0] in PROGRAMS and nl > 0), key


def test_check_one_chain_rejects_what_the_tail_cannot_take():
    cmax = (1 << 63)
    G.check_one_chain("t", 13, cmax)
    for bad in (lambda: G.check_one_chain("t", 0, cmax), lambda: G.check_one_chain("t", 65, cmax),
                lambda: G.check_one_chain("t", 13, (1 << 64) - (1 << 30))):
        with pytest.raises(AssertionError):
            bad()
