"""CPU suite: the generator's limb-level model of the team-program executor
(tools/gen_g2_schedule.py run_bound_limbs) at the edges of the admitted input
range, for every bound instance of bn256_xtab.h: it raises no assertion, means
what the abstract bound program means (run_bound on the residues), keeps its
results in range and leaves every other element alone.

This module also builds the case list and the model's results that
tests/test_gpu_xinst.py compares the GPU with (fixed seed, no GPU imports),
and checks the condition on those inputs that the GPU test relies on: every
form of the executor's guarded final subtraction is TAKEN at least once in
every layout whose rounds use that form. The forms and the layouts that use them:

  csub_rare  acc_reduce's fp_csub_rare (rounds without linear terms)      D S T V F
  wide       acc_reduce_wide's subtraction (linear terms, canonical)     D S V F
  redq       the canonical one-chain tail redq_tail<QMAX, false>         T

(layout T has no acc_reduce_wide round: its only canonical linear-term program,
LINE_FIX_12, reduces in one chain; that program is the one user of the
canonical one-chain tail, the other one-chain program, CYC_SQR_X_12, is lazy.)
No form is skipped, and no case beyond the thirteen had to be added: the
fillings "every element p" and the draws from {0, 1, p-1, p, p+1, 2p-1, ...}
give REDC results of exactly p in every layout and form.
"""

import functools
import os
import random
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tools"))

import gen_g2_schedule as G  # noqa: E402

P = G.P
SEED = 20240611
RINV = pow(G.R_MONT, -1, P)
LAYOUTS = G.PROBE_LAYOUTS
FORMS = ("csub_rare", "wide", "redq")
# layouts whose rounds use each form (checked against the rounds in test_forms_per_layout)
FORM_LAYOUTS = {"csub_rare": ("D", "S", "T", "V", "F"), "wide": ("D", "S", "V", "F"), "redq": ("T",)}
NCASES = 13


@functools.lru_cache(maxsize=None)
def programs():
    return G.compile_all()


@functools.lru_cache(maxsize=None)
def region_elems():
    return G.probe_region_elems(programs())


def layout_of(i):
    name, _, layout = G.ALL_INSTANCES[i]
    return G.probe_layout(name, layout)


def instances(layout):
    return [i for i in range(len(G.ALL_INSTANCES)) if layout_of(i) == layout]


def label(i):
    name, binding, layout = G.ALL_INSTANCES[i]
    return f"#{i} {name}{'_' + layout if layout else ''}<{','.join(binding)}>"


def mont(v):
    """Residue -> the limbs of its canonical Montgomery representative."""
    return G.to_limbs(v * G.R_MONT % P)


# ------------------------------------------------------------------ structured inputs (cases 12, 13)
@functools.lru_cache(maxsize=None)
def _real_values():
    """Residues of one real Miller-loop state, as validate_x sets it up: the
    point registers of a doubling / addition step, the evaluation point, a
    normalised G2Base line; and a unitary (cyclotomic) g with its conjugate."""
    from oracle import bn256_oracle as O

    rng = random.Random(SEED)
    Q = O.g2_mul(O.G2_GEN, rng.randrange(1, O.ORDER))
    Hp = O.g1_mul(O.G1_GEN, rng.randrange(1, O.ORDER))
    Rj = O.jac_mul(O.FP2_OPS, O.to_jac(O.FP2_OPS, Q), rng.randrange(2, 1000))
    rx = O.f2_mul(Rj[0], O.f2_inv(O.f2_sqr(Rj[2])))
    ry = O.f2_mul(Rj[1], O.f2_inv(O.f2_mul(O.f2_sqr(Rj[2]), Rj[2])))
    Wr = (rng.randrange(1, P), rng.randrange(P))
    Zr = O.f2_mul((1, 3), Wr)
    rnd2 = lambda: (rng.randrange(P), rng.randrange(P))  # noqa: E731
    regs = {"X": O.f2_mul(rx, Zr), "Y": O.f2_mul(ry, Zr), "Z": Wr, "QX": Q[0], "QY": Q[1], "NQY": O.f2_neg(Q[1]),
            "P1X": O.f2_mul(Q[0], rnd2()), "P1Y": rnd2(), "P2X": rnd2(), "FBX": rnd2(), "FCY": rnd2()}
    F = {}
    for n, (x, y) in regs.items():
        F[G.comp(n, "x")], F[G.comp(n, "y")] = x, y
    F[G.REG["PX"]], F[G.REG["PY"]] = Hp
    F[G.REG["SX"]], F[G.REG["NSY"]] = rng.randrange(P), rng.randrange(P)
    f = [rnd2() for _ in range(6)]
    g = O.f12_mul(O.f12_conj(f), O.f12_inv(f))
    g = O.f12_mul(g, O.f12_frob2(g))
    assert [tuple(c) for c in O.f12_mul(g, O.f12_conj(g))] == [tuple(c) for c in O.F12_ONE], "g is unitary"
    flat = lambda v: [z for pair in v for z in pair]  # noqa: E731
    return F, flat(g), flat(O.f12_conj(g))


def _structured(i, rng):
    """The residues of cases 12 and 13: random canonical elements, then the registers
    of a real step, then the operand slots: a unitary g in A and conj(g) in B
    for a three-slot program (an in-place binding keeps both; with A = B the
    slot holds g), the element one for a two-slot program."""
    name, binding, layout = G.ALL_INSTANCES[i]
    n = region_elems()[layout_of(i)]
    fb = G.probe_reg_base(name, layout)
    res = [rng.randrange(P) for _ in range(n)]
    F, g, gc = _real_values()
    if G.X_PROGRAMS[name] != "FOLD":  # FOLD keeps ZERO and ONE only
        for r, v in F.items():
            if fb + r < n:
                res[fb + r] = v
    if len(binding) == 3:
        a, b = 12 * G.SLOTS.index(binding[1]), 12 * G.SLOTS.index(binding[2])
        res[b:b + 12] = gc
        res[a:a + 12] = g
    elif len(binding) == 2:
        a = 12 * G.SLOTS.index(binding[1])
        res[a:a + 12] = [0, 1] + [0] * 10
    return res


def _alternating(e):
    """Limbs alternating 0 and 2^26 - 1 (phase: the element's parity), the top
    limb at LAZY_LIMB[9] where that keeps the value below 2p."""
    low = [G.MASK26 if (j + e) & 1 else 0 for j in range(9)]
    top = G.LAZY_LIMB[9]
    if G.from_limbs(low + [top]) >= 2 * P:
        top -= 1
    return low + [top]


EDGE_VALUES = (0, 1, P - 1, P, P + 1, 2 * P - 1)


def build_cases(i):
    """[(case name, region)] for instance i: region is a list of elements,
    each ten limbs, with ZERO and ONE set; the pre-pass scratch is filled like
    any other element."""
    name, _, layout = G.ALL_INSTANCES[i]
    n = region_elems()[layout_of(i)]
    fb = G.probe_reg_base(name, layout)
    rng = random.Random(SEED * 1000 + i)
    cases = [("all 2p-1", [G.to_limbs(2 * P - 1) for _ in range(n)]),
             ("all p-1", [G.to_limbs(P - 1) for _ in range(n)]),
             ("all 0", [G.to_limbs(0) for _ in range(n)]),
             ("all p", [G.to_limbs(P) for _ in range(n)]),
             ("alternating limbs", [_alternating(e) for e in range(n)])]
    for k in range(4):
        mem = []
        for _ in range(n):
            c = rng.randrange(len(EDGE_VALUES) + 1)
            mem.append(G.to_limbs(EDGE_VALUES[c] if c < len(EDGE_VALUES) else rng.randrange(2 * P)))
        cases.append((f"edge draw {k}", mem))
    for k in range(2):
        cases.append((f"canonical {k}", [G.to_limbs(rng.randrange(P)) for _ in range(n)]))
    res = _structured(i, rng)
    cases.append(("structured", [mont(v) for v in res]))
    # the same with every operand in its lazy form x + p (below 2p for every canonical x)
    cases.append(("structured lazy", [G.to_limbs(v * G.R_MONT % P + P) for v in res]))
    assert len(cases) == NCASES
    for _, mem in cases:
        mem[fb + G.REG["ZERO"]] = G.to_limbs(0)
        mem[fb + G.REG["ONE"]] = mont(1)
        assert all(G.from_limbs(l) < 2 * P and max(l[:9]) <= G.MASK26 for l in mem)
    return cases


# ------------------------------------------------------------------ the model's results, with what its rounds did
class Run:
    """One (instance, case): the region before and after run_bound_limbs, the
    rounds' results, and the guarded subtractions per form: [calls, taken]."""
    def __init__(self, inst, case, mem_in):
        self.inst, self.case, self.mem_in = inst, case, mem_in
        self.mem_out = None
        self.rounds = []  # (bound round, pre, out) of xround_limbs
        self.subs = {f: [0, 0] for f in FORMS}


def run_model(i, case, mem_in):
    """run_bound_limbs on a copy of mem_in, observed: the generator's own
    xround_limbs, _csub_model and redq_tail_model run wrapped, unchanged."""
    run = Run(i, case, mem_in)
    rounds = G.instance_rounds(programs(), i)
    orig = G.xround_limbs, G._csub_model, G.redq_tail_model

    def xround(xr, read):
        pre, out = orig[0](xr, read)
        run.rounds.append((xr, pre, out))
        return pre, out

    def csub(x, rare):
        r = orig[1](x, rare)
        s = run.subs["csub_rare" if rare else "wide"]
        s[0] += 1
        s[1] += r != list(x)
        return r

    def redq(c, qmax, lazy):
        r = orig[2](c, qmax, lazy)
        if not lazy:
            run.subs["redq"][0] += 1
            run.subs["redq"][1] += r != orig[2](c, qmax, True)
        return r

    G.xround_limbs, G._csub_model, G.redq_tail_model = xround, csub, redq
    try:
        mem = [list(l) for l in mem_in]
        G.run_bound_limbs(rounds, mem)
    finally:
        G.xround_limbs, G._csub_model, G.redq_tail_model = orig
    run.mem_out = mem
    return run


@functools.lru_cache(maxsize=None)
def instance_runs(i):
    """Every case of instance i through the model, computed once per session
    and shared (the GPU test compares the probe with mem_out)."""
    return [run_model(i, case, mem) for case, mem in build_cases(i)]


# the tests' parameters: a layout's instances, the big default layout in three parts
PARTS = [("D", 0), ("D", 1), ("D", 2), ("S", 0), ("T", 0), ("V", 0), ("F", 0)]
PART_IDS = [f"{lay}{k}" for lay, k in PARTS]


def part_instances(layout, part):
    return instances(layout)[part::sum(1 for lay, _ in PARTS if lay == layout)]


def reference(layout):
    return [run for i in instances(layout) for run in instance_runs(i)]


def taken_counts(layout):
    """{form: [calls, taken]} over the layout's probed (instance, case, lane) results."""
    tot = {f: [0, 0] for f in FORMS}
    for run in reference(layout):
        for f in FORMS:
            tot[f][0] += run.subs[f][0]
            tot[f][1] += run.subs[f][1]
    return tot


# ------------------------------------------------------------------ tests
def test_case_list_covers_every_instance():
    assert sorted(i for lay in LAYOUTS for i in instances(lay)) == list(range(len(G.ALL_INSTANCES)))
    assert len(G.ALL_INSTANCES) == 145 and len(instances("S")) == 28
    assert all(len(build_cases(i)) == NCASES for i in (0, len(G.ALL_INSTANCES) - 1))


@pytest.mark.parametrize("layout,part", PARTS, ids=PART_IDS)
def test_limb_model_at_the_edges(layout, part):
    """run_bound_limbs raised no assertion (instance_runs ran it); its results
    are congruent to run_bound's, in range, and nothing else moved."""
    for run in (r for i in part_instances(layout, part) for r in instance_runs(i)):
        who = f"{label(run.inst)} case {run.case!r}"
        rounds = [xr for xr, _, _ in run.rounds]
        res = [G.from_limbs(l) * RINV % P for l in run.mem_in]
        G.run_bound(rounds, res)
        for e, (l, v) in enumerate(zip(run.mem_out, res)):
            assert G.from_limbs(l) * RINV % P == v, f"{who}: element {e} differs from run_bound"
        written = set()
        for xr, pre, out in run.rounds:
            written |= set(pre) | set(out)
            lazy_dsts = {L["dst"] for L in xr.lanes} if xr.lz else set()
            for d, l in out.items():
                v = G.from_limbs(l)
                assert max(l[:9]) <= G.MASK26, f"{who}: {xr.name} element {d}: a low limb above 26 bits"
                if d in lazy_dsts:
                    assert v < 2 * P, f"{who}: lazy {xr.name} element {d} not below 2p"
                else:
                    assert v < P, f"{who}: {xr.name} element {d} not below p"
        for e, (a, b) in enumerate(zip(run.mem_in, run.mem_out)):
            assert e in written or a == b, f"{who}: element {e} changed, no round writes it"


def test_forms_per_layout():
    """FORM_LAYOUTS is what the bound rounds say."""
    uses = {f: set() for f in FORMS}
    for i, (name, binding, layout) in enumerate(G.ALL_INSTANCES):
        for xr in G.instance_rounds(programs(), i):
            jobs = [(xr.nl, xr.one_chain, xr.lz)] + ([(xr.nl2, False, 0)] if xr.fused else [])
            for nl, one_chain, lz in jobs:
                if nl == 0:
                    uses["csub_rare"].add(layout_of(i))
                elif not lz:
                    uses["redq" if one_chain else "wide"].add(layout_of(i))
    assert {f: tuple(l for l in LAYOUTS if l in s) for f, s in uses.items()} == FORM_LAYOUTS
    one_chain_canonical = {n for n, _, _ in G.ALL_INSTANCES for xr in programs()[n] if xr.one_chain and not xr.lz}
    assert one_chain_canonical == {"LINE_FIX_12"}


@pytest.mark.parametrize("layout", LAYOUTS)
def test_rare_subtractions_are_taken(layout):
    """A condition on the inputs, not on the kernel: in every form this
    layout's rounds use, some probed lane takes the subtraction."""
    tot = taken_counts(layout)
    print(f"layout {layout}: taken / guarded subtractions: " + ", ".join(f"{f} {tot[f][1]}/{tot[f][0]}" for f in FORMS))
    for f in FORMS:
        if layout in FORM_LAYOUTS[f]:
            assert tot[f][1] >= 1, f"layout {layout}: no probed lane takes the {f} subtraction"
        else:
            assert tot[f][0] == 0, f"layout {layout}: form {f} runs after all"


def test_issue_examples_take_the_rare_subtraction():
    """g * conj(g) leaves exactly p in 11 of 12 lanes of the Fp12 products;
    the element one takes the rare subtraction in 3 lanes of the squarings."""
    by_name = {}
    for lay in LAYOUTS:
        for run in reference(lay):
            name, binding, _ = G.ALL_INSTANCES[run.inst]
            if run.case == "structured" and (len(binding) < 3 or len(set(binding[1:])) == 2):
                by_name.setdefault(name, run)
    for name in ("MUL12", "MUL12_12", "MUL12F"):
        assert by_name[name].subs["csub_rare"] == [12, 11], name
    for name in ("SQR12", "SQR12_12"):
        assert by_name[name].subs["csub_rare"] == [12, 3], name
    assert by_name["CYC_SQR"].subs["wide"] == [12, 5]
