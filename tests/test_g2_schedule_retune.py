"""The 12-lane pairing programs' per-program codegen choices (tools/
gen_g2_schedule.py KARATSUBA_MIN_PROG, REDC_FUSE): every layout-T instance of
SQR12_12, LINE_FIX_12, MUL12_12 and CYC_SQR_X_12 still computes the oracle's
Fp12 result, on canonical and on lazy ([p, 2p)) inputs, with the KS / FU flags
the emitter writes for it — a silent fall-back to schoolbook products or to
the fused reduction fails here — inside the generator's bounds, with at most
two pre-pass values per lane and layout T's team region unchanged. The
16-lane programs of layout S keep their flags.
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
# program -> (KS of its job, FU) as the emitter must write them (layout T)
FLAGS_T = {"SQR12_12": (1, 0), "LINE_FIX_12": (1, 0), "MUL12_12": (1, 0), "CYC_SQR_X_12": (1, 0)}
# ... and the 16-lane programs of k_verify_sig (layout S), which stay as they were
FLAGS_S = {"SDBL": (1, 1), "LFEV": (1, 1), "LINE_FIX": (1, 1), "MUL12": (1, 1), "CYC_SQR_X": (0, 1)}
T_INSTANCES = [(n, b) for n, b, lay in G.ALL_INSTANCES if lay == "T"]


@pytest.fixture(scope="module")
def compiled():
    return G.compile_all()


@pytest.fixture(scope="module")
def emitted(compiled, tmp_path_factory):
    """(program, layout, binding) -> the template arguments of each x_round call the emitter writes."""
    path = tmp_path_factory.mktemp("xtab") / "bn256_xtab.h"
    G.emit_x(compiled, str(path))
    text = path.read_text()
    out = {}
    for m in re.finditer(r"struct XInst<XP_(\w+?)(?:_([STV]))?((?:, S_\w)*)> \{(.*?)\} \};", text):
        rounds = [tuple(int(v) for v in r.split(",")) for r in re.findall(r"x_round<([^>]*)>", m.group(4))]
        binding = tuple(re.findall(r"S_(\w)", m.group(3)))
        out[(m.group(1), m.group(2) or "", binding)] = rounds
    out["kSigTTeamElems"] = int(re.search(r"kSigTTeamElems = (\d+)", text).group(1))
    return out


def _ks_fu(targs):
    # x_round<NV, NT, NP, NL, W, NP2, NL2, KP, KL1, KL2, KS1, KS2, LZ, EF, FU>
    assert len(targs) == 15
    return targs[10], targs[14]


def test_t_instances_cover_the_four_programs():
    assert {n for n, _ in T_INSTANCES} == set(FLAGS_T)


@pytest.mark.parametrize("name,binding", T_INSTANCES, ids=[f"{n}-{''.join(b)}" for n, b in T_INSTANCES])
@pytest.mark.parametrize("lazy", [False, True], ids=["canonical", "lazy"])
def test_bound_instance_matches_oracle_with_emitted_flags(compiled, emitted, name, binding, lazy):
    rounds_t = emitted[(name, "T", binding)]
    assert [_ks_fu(t) for t in rounds_t] == [FLAGS_T[name]] * len(compiled[name]), (name, rounds_t)
    rng = random.Random(f"{name}{binding}{lazy}")
    ctx = G.X_PROGRAMS[name]
    rounds = [G.bind(xr, binding, ctx, "T") for xr in compiled[name]]
    # the emitted flags are the compiled rounds' own
    assert [t[10] for t in rounds_t] == [bx.ks1 for bx in rounds]
    fb = G.SIG_T_F_BASE
    mem = [rng.randrange(P) for _ in range(fb + G.NREGS)]
    mem[fb + G.REG["ZERO"]] = 0
    mem[fb + G.REG["ONE"]] = 1
    f = [(rng.randrange(P), rng.randrange(P)) for _ in range(6)]
    g = [(rng.randrange(P), rng.randrange(P)) for _ in range(6)]
    if name == "CYC_SQR_X_12":  # an element of the cyclotomic subgroup
        f = O.f12_mul(O.f12_conj(f), O.f12_inv(f))
        f = O.f12_mul(f, O.f12_frob2(f))
    D, A, B = (list(binding) + [binding[1]])[:3]
    if name == "MUL12_12" and A == B:
        g = f
    lift = P if lazy else 0  # lazy elements: the same residues in [p, 2p)
    for s, v in ((A, f), (B, g)) if name == "MUL12_12" else ((A, f),):
        flat = [z for pair in v for z in pair]
        mem[12 * G.SLOTS.index(s):12 * G.SLOTS.index(s) + 12] = [z + lift for z in flat]
    if name == "LINE_FIX_12":
        lb, lc = [(mem[fb + G.comp(n, "x")], mem[fb + G.comp(n, "y")]) for n in ("FB", "FC")]
        want = O._mul_line(f, O.F2_ONE, lb, lc)
    elif name == "MUL12_12":
        want = O.f12_mul(f, g)
    else:
        want = O.f12_sqr(f)
    G.run_bound(rounds, mem)
    d0 = 12 * G.SLOTS.index(D)
    got = [(mem[d0 + 2 * k], mem[d0 + 2 * k + 1]) for k in range(6)]
    assert got == want, (name, binding)


@pytest.mark.parametrize("name", sorted(FLAGS_T))
def test_rounds_pass_the_generator_bounds(compiled, name):
    """check_xround on the compiled rounds, with the pre-pass values read back
    from the lanes: limb sums < 2^32 (the Karatsuba half sums included),
    columns < 2^64, REDC result in range — with the round-uniform correction
    (no per-lane fall-back) and the Karatsuba flag it was compiled with."""
    for xr in compiled[name]:
        order = {}
        for L in xr.lanes:
            for d, terms in L["pre"]:
                if d != G.NONE:
                    order[d - G.X_SCR] = tuple((s, k) for s, k in terms if k != 0)
        assert sorted(order) == list(range(len(order)))
        assert xr.kp >= 0 and xr.kl1 >= 0, "round-uniform corrections"
        ks = xr.ks1
        G.check_xround(xr, [order[i] for i in range(len(order))], G.KARATSUBA_MIN_PROG.get(name))
        assert xr.ks1 == ks == FLAGS_T[name][0]
        if name == "CYC_SQR_X_12":
            assert xr.nv <= 2 and xr.np == 3, "at most two pre-pass values per lane, 3-product jobs"
            assert len(order) <= 24
        assert all(d == G.NONE for L in xr.lanes[12:] for d, _ in L["pre"]), "pre-pass on lanes 0..11"


def test_karatsuba_needs_every_lane_to_qualify(compiled):
    """The threshold alone does not switch Karatsuba on: the 16-lane cyclotomic
    squaring's forms (18 a_x + 6 a_y, ...) fail the half-sum bound at threshold 3."""
    xr = G.compile_round(G.PROGRAMS["CYC_SQR_X"][0], "CYC_SQR_X[0]", G.SCRATCH_CAP["FE"], ks_min=3)
    assert xr.ks1 == 0
    assert compiled["CYC_SQR_X"][0].ks1 == 0


def test_layout_t_team_region_is_unchanged(emitted):
    assert emitted["kSigTTeamElems"] == 92
    assert G.SIG_T_F_BASE == 60 and G.SCRATCH_CAP["FE"] == 48


def test_layout_s_programs_keep_their_flags(emitted):
    seen = set()
    for key, rounds in emitted.items():
        if isinstance(key, tuple) and key[1] == "S" and key[0] in FLAGS_S:
            assert [_ks_fu(t) for t in rounds] == [FLAGS_S[key[0]]] * len(rounds), key
            seen.add(key[0])
    assert seen == set(FLAGS_S)
