"""THE LAYOUT TABLE and the per-call-site instances: one Layout record per team
region a kernel gives its programs, each with the instances bound on it.
bind gives every instance its own table with absolute team element indices
(slot s element e -> 12 s + e, register r -> the layout's register base + r),
so the executor needs no address selects."""

from __future__ import annotations

import random
from dataclasses import dataclass
from types import MappingProxyType

from .field import NONE, NREGS, P, REG, SLOT_A
from .limbs import R_MONT, from_limbs, run_bound_limbs, to_limbs
from .programs import SCRATCH_CAP, X_PROGRAMS
from .xround import X_SCR, X_SLOT_B, run_xprogram

SLOTS = ["F", "A", "B", "C", "D", "E", "G", "H", "I", "J", "K", "L"]   # enum S_F.. (bn256_pairing.h)
ALL_REGS = range(NREGS)


@dataclass(frozen=True)
class Layout:
    """A team region: Fp12 slots of 12 elements from element 0 on, the register
    file (or a part of it) from reg_base on, and the pre-pass scratch of each
    scratch context it admits. Adding a layout is one record here with its
    instance list; bind, the region check, the emitters and the probe look the
    record up."""
    key: str            # bind's layout argument and the suffix of XP_<program>_<key> ("": none)
    probe: str          # the instance probe's name of the region (XPL_<probe>, bn256_xprobe.h)
    slots: list         # the slots an instance may name
    reg_base: int       # team element of register 0
    scr_base: dict      # scratch context -> first scratch element; the contexts the layout admits
    end: int            # no index of a bound round reaches this element
    regs: object = ALL_REGS    # registers a program may read
    wregs: object = ALL_REGS   # ... and write
    # scratch context -> [lo, hi): where that context's pre-pass destinations
    # must fall (a Miller loop's scratch lies in slots that are dead meanwhile)
    pre_window: dict = MappingProxyType({})
    # The emitted region size: end itself (None), or the largest element an
    # instance touches + 1, at least floor (the registers the kernel's
    # hand-written helpers use).
    floor: int | None = None
    # the two constants of bn256_xtab.h, (name, trailing comment) each: the
    # register base and the region's element count (rounded up to even)
    consts: tuple | None = None
    instances: list = ()   # (program, binding): the call sites, XInst<XP_program[_key], S_binding...>


# ---- the full region (bn256_pairing.h, kTeamWords): 12 Fp12 slots, then the
# register file. FE scratch: the register file from register 2 on; ML scratch:
# slots C..J during the Miller loop.
F_BASE = 12 * len(SLOTS)


def _pow_u_mul_instances(dst, sa):
    """t12_pow_u_x<dst, sa> (bn256_xprog.h): three exponentiations by v,
    a -> dst, dst -> J, J -> dst, each with the conjugate of its base in K."""
    out = []
    for d, base in ((dst, sa), ("J", dst), (dst, "J")):
        out += [("CYC_SQR_X", (d, base)), ("CYC_SQR_X", (d, d)), ("MUL12", (d, d, "K")), ("MUL12", (d, d, base))]
    return out


INSTANCES = sorted(set(
    [("MUL12", b) for b in [("F", "B", "A"), ("F", "F", "A"), ("A", "A", "B"), ("H", "C", "H"), ("I", "E", "I"),
                            ("K", "K", "H"), ("K", "K", "D"), ("J", "G", "D"), ("J", "J", "K"), ("K", "K", "C"),
                            ("K", "J", "L"), ("J", "J", "A"), ("F", "K", "J"), ("L", "F", "K"), ("A", "K", "L"),
                            ("F", "A", "B"), ("L", "A", "K"), ("F", "K", "L")]]
    # team_final_exp's exp-by-v chain (slots I <-> J, conjugate in K) and the a^u probe
    + [("CYC_SQR_X", b) for b in [("J", "I"), ("J", "J"), ("I", "J"), ("I", "I")]]
    + [("MUL12", b) for b in [("J", "J", "K"), ("J", "J", "I"), ("I", "I", "K"), ("I", "I", "J")]]
    + _pow_u_mul_instances("F", "A")
    + [("CYC_SQR_X", b) for b in [("K", "I"), ("J", "J"), ("K", "K"), ("F", "A")]]
    + [("SQR12", ("F", "F")), ("SQR12", ("F", "A")), ("LINE_PK", ("F", "F")), ("LINE_FIX", ("F", "F"))]
    # tools/opcycles.hip
    + [("CYC_SQR_X", ("A", "A")), ("SQR12", ("A", "A")), ("LINE_PK", ("A", "A"))]
    + [(g, ()) for g in ("PDBL", "PADD_POS", "PADD_NEG", "PADD_F1", "PADD_F2", "PDBL_1")]
    + [(f"PADD_{v}_{i}", ()) for v in ("POS", "NEG", "F1", "F2") for i in (1, 3)]
    + [(f"MADD_{v}_2", ("F", "F")) for v in ("POS", "NEG", "F1", "F2")]
    + [("MDBL_1", ("F", "F")), ("MDBL_2", ("F", "F"))]
    # team_final_exp_fc (bn256_pairing.h): the Fuentes-Castaneda hard part
    + [("CYC_SQR_X", ("B", "A")), ("CYC_SQR", ("I", "C"))]
    + [("MUL12", b) for b in [("B", "A", "B"), ("B", "C", "D"), ("E", "B", "J"), ("D", "A", "E"), ("A", "C", "E"),
                              ("A", "F", "A"), ("A", "G", "A"), ("G", "G", "D"), ("F", "G", "A")]]
    # bn256_gtfold.h: the GT fold and its table builders. A FOLD-context
    # program: bound on the FOLD region below (region() goes by the context),
    # listed here so that it keeps its place among the unsuffixed instances
    + [("MUL12F", ("A", "A", "B"))]))
FULL = Layout("", "D", SLOTS, F_BASE, {"FE": F_BASE + 2, "ML": 12 * SLOTS.index("C")}, F_BASE + NREGS,
              instances=INSTANCES)

# ---- k_verify_sig's compact team region (layout "S", bn256_sig16.hip): slots F, A, B,
# C, D, E, G — the sig-only Miller loop and the Fuentes-Castaneda final
# exponentiation (team_final_exp_fc_s) need no more — then the register file.
# The Miller loop's pre-pass scratch lies in slots A.. (only F is live there),
# the final exponentiation's past register ONE (the Miller registers are dead
# there), as in the full layout. 118 elements per team instead of 180: 18.9 KB
# of LDS per 4-team wave, so two pairing waves fit on a SIMD and the CU keeps
# room for a fold workgroup beside its eight pairing waves.
SIG_SLOTS = SLOTS[:7]
SIG_F_BASE = 12 * len(SIG_SLOTS)
SIG_INSTANCES = sorted(set(
    [("SDBL", ("F", "F")), ("LFEV", ("F", "F")), ("FEVAL", ()), ("LINE_FIX", ("F", "F"))]
    # the easy part (inversion scratch D, E) and the exponentiations by v
    # (D <-> E, conjugate of the base in G)
    + [("MUL12", b) for b in [("E", "F", "D"), ("A", "D", "E"), ("F", "B", "A"), ("F", "F", "A"),
                              ("E", "E", "G"), ("E", "E", "D"), ("D", "D", "G"), ("D", "D", "E"),
                              ("B", "A", "B"), ("B", "C", "G"), ("G", "B", "E"), ("B", "A", "G"),
                              ("A", "C", "G"), ("A", "F", "A"), ("A", "D", "A"), ("D", "D", "B"), ("F", "D", "A")]]
    + [("CYC_SQR_X", b) for b in [("E", "D"), ("E", "E"), ("D", "E"), ("D", "D"), ("A", "A"), ("B", "A")]]
    # t3 = t2^2 as a product (canonical, 21 scratch elements: the canonical
    # CYC_SQR's 34 would set the region's end)
    + [("MUL12", ("D", "C", "C"))]))
SIG = Layout("S", "S", SIG_SLOTS, SIG_F_BASE, {"FE": SIG_F_BASE + 2, "ML": 12 * SLOTS.index("A")}, SIG_F_BASE + NREGS,
             pre_window={"ML": (12, SIG_F_BASE)},       # the Miller scratch stays inside slots A..G
             floor=SIG_F_BASE + REG["FC.y"] + 1,        # team_miller_sig's registers: ZERO .. FC
             consts=(("kSigRegBase", "k_verify_sig's layout S: registers here"),
                     ("kSigTeamElems", "k_verify_sig's team region (layout S)")),
             instances=SIG_INSTANCES)

# ---- k_verify_sig12's team region (layout "T", bn256_sig12.hip): FIVE Fp12 slots
# F, A, B, C, D — the final exponentiation parks two values (res and t0) in
# HBM while the exponentiations by u run (bn256_sigfe.h team_final_exp_fc_t),
# so five slots are live at most — then the register file (ZERO, ONE; the
# Miller loop's FB, FC; the final exponentiation's pre-pass scratch from
# register 2 on). 92 elements (94 before the r06 shared-operand squaring):
# five 12-lane teams take 18.4 KB of LDS per
# wave, so a CU holds eight pairing waves (two per SIMD) and a fold workgroup.
SIG_T_SLOTS = SLOTS[:5]
SIG_T_F_BASE = 12 * len(SIG_T_SLOTS)
SIG_T_INSTANCES = sorted(set(
    [("SQR12_12", ("F", "F")), ("LINE_FIX_12", ("F", "F"))]
    # the easy part and the three phases' exponentiations by v (C <-> D, the
    # conjugate of the base in B / F) and their tails
    + [("MUL12_12", b) for b in [("B", "F", "D"), ("A", "D", "B"), ("F", "B", "A"), ("F", "F", "A"),
                                 ("C", "C", "B"), ("C", "C", "F"), ("D", "D", "B"), ("D", "D", "F"),
                                 ("B", "A", "B"), ("B", "A", "F"), ("D", "A", "A"), ("D", "B", "C"),
                                 ("F", "A", "D"), ("F", "A", "F"), ("F", "C", "F"), ("D", "D", "C"), ("C", "C", "D")]]
    + [("CYC_SQR_X_12", b) for b in [("C", "F"), ("C", "C"), ("D", "C"), ("D", "D"), ("C", "D"), ("C", "B"),
                                     ("A", "A"), ("B", "A")]]))
SIG_T = Layout("T", "T", SIG_T_SLOTS, SIG_T_F_BASE, {"FE": SIG_T_F_BASE + 2, "ML": 12 * SLOTS.index("A")},
               SIG_T_F_BASE + NREGS,
               pre_window={"ML": (12, SIG_T_F_BASE)},   # the Miller scratch stays inside slots A..D
               floor=SIG_T_F_BASE + REG["FC.y"] + 1,    # team_miller_sig12's registers: ZERO, ONE, FB, FC
               consts=(("kSigTRegBase", "k_verify_sig12's layout T: registers here"),
                       ("kSigTTeamElems", "k_verify_sig12's team region")),
               instances=SIG_T_INSTANCES)
# team_miller_sig12's pair product, bound on layout T. A list of its own:
# ALL_INSTANCES numbers the instance probe's cases (bn256_xprobe.h), which stay
# as they are; the tables, the region check and check_instances take both
# lists (BOUND_INSTANCES), the fold's instance still last.
PAIR_INSTANCES = [("LINE2_FIX_12", ("F", "F"), SIG_T.key)]

# ---- k_verify_ml's team region (layout "V", bn256_verify.hip, r06): the
# two-pairing Miller loop of config 2 alone — f in slot F, the pre-pass values
# of its programs right after it (MDBL_1's 50 at most), then the whole runtime
# register file — 128 elements, so a 4-team wave takes 20480 bytes of LDS and
# a CU's 160 KiB holds eight, two per SIMD (k_verify's 212-element region:
# four). The final
# exponentiation runs on the 12-lane split kernels (bn256_sig12.hip).
V_SCRATCH = 50
V_F_BASE = 12 + V_SCRATCH
V_INSTANCES = ([("MDBL_1", ("F", "F")), ("MDBL_2", ("F", "F")), ("PDBL_1", ()), ("LINE_PK", ("F", "F"))]
               + [(f"PADD_{v}_{i}", ()) for v in ("POS", "NEG", "F1", "F2") for i in (1, 3)]
               + [(f"MADD_{v}_2", ("F", "F")) for v in ("POS", "NEG", "F1", "F2")])
V = Layout("V", "V", SLOTS[:1], V_F_BASE, {"ML": 12}, V_F_BASE + NREGS,
           pre_window={"ML": (12, V_F_BASE)},           # the scratch lies between slot F and the registers
           consts=(("kVRegBase", "k_verify_ml's layout V: registers here"),
                   ("kVTeamElems", "k_verify_ml's team region")),
           instances=V_INSTANCES)

# ---- the FOLD context's region (bn256_gtfold.h, the GT fold kernels): slots
# F, A, B, then registers ZERO and ONE only, then the pre-pass scratch. No
# layout of its own for bind: a FOLD-context program bound with layout ""
# lands here. The programs write slots only.
FOLD_SLOTS = SLOTS[:3]
FOLD_F_BASE = 12 * len(FOLD_SLOTS)
# bn256_gt.hip k_tor_chunks: X = X * (alpha + w). Listed last, so the tables
# of every other instance keep their places in kXTab.
TOR_INSTANCES = [("TORMULF", ("A", "A", "B"))]
FOLD = Layout("", "F", FOLD_SLOTS, FOLD_F_BASE, {"FOLD": FOLD_F_BASE + 2}, FOLD_F_BASE + 2 + SCRATCH_CAP["FOLD"],
              regs=(REG["ZERO"], REG["ONE"]), wregs=(),
              floor=FOLD_F_BASE + 2,                    # ZERO, ONE
              consts=(("kFoldRegBase", "FOLD team region: ZERO, ONE here"),
                      ("kFoldTeamElems", "elements the fold programs touch")),
              instances=TOR_INSTANCES)

# The order is enum XProbeLayout's and that of the instances in kXTab and in
# the probe; the _S / _T / _V variants of enum XProg follow it too.
LAYOUTS = (FULL, SIG, SIG_T, V, FOLD)
PROBE_LAYOUTS = tuple(lay.probe for lay in LAYOUTS)
_REGION = {(lay.key, ctx): lay for lay in LAYOUTS for ctx in lay.scr_base}
assert all(lay.scr_base[ctx] + SCRATCH_CAP[ctx] <= lay.end for (_, ctx), lay in _REGION.items())


def region(ctx, layout=""):
    """The Layout record of a program of scratch context ctx bound with bind's layout argument."""
    assert (layout, ctx) in _REGION, f"layout {layout!r} admits no {ctx} program"
    return _REGION[layout, ctx]


# the full region's numbers per scratch context, as the tests read them
F_BASE_CTX = MappingProxyType({ctx: region(ctx).reg_base for ctx in SCRATCH_CAP})
REGION_END = MappingProxyType({ctx: region(ctx).end for ctx in SCRATCH_CAP})

ALL_INSTANCES = [(n, b, lay.key) for lay in LAYOUTS for n, b in lay.instances]
# The probe runs the pair instances too, behind its numbered cases: instance k of
# PAIR_INSTANCES is probe instance PROBE_EXTRA_BASE + k (hg_debug_xinst), and
# entry len(ALL_INSTANCES) + k of PROBE_INSTANCES, kXProbeInfo and instance_rounds.
PROBE_EXTRA_BASE = 1 << 16
PROBE_INSTANCES = ALL_INSTANCES + PAIR_INSTANCES
BOUND_INSTANCES = ALL_INSTANCES[:-len(TOR_INSTANCES)] + PAIR_INSTANCES + ALL_INSTANCES[-len(TOR_INSTANCES):]


def bind(xr, binding, ctx, layout=""):
    """Translates a compiled round to absolute team element indices."""
    lay = region(ctx, layout)
    D, A, B = (list(binding) + [None, None, None])[:3]
    if len(binding) == 2:
        D, A = binding
        B = A
    assert all(b in lay.slots for b in binding), f"layout {lay.probe}: slots {lay.slots[0]}..{lay.slots[-1]} only"
    sbase, fbase = lay.scr_base[ctx], lay.reg_base

    def src(code):
        if code >= X_SCR:
            return sbase + (code - X_SCR)
        if code >= X_SLOT_B:
            return 12 * SLOTS.index(B) + (code - X_SLOT_B)
        if code >= SLOT_A:
            return 12 * SLOTS.index(A) + (code - SLOT_A)
        assert code in lay.regs, f"layout {lay.probe} does not keep register {code}"
        return fbase + code

    def dst(code):
        if code == NONE:
            return NONE
        if code >= SLOT_A:
            return 12 * SLOTS.index(D) + (code - SLOT_A)
        assert code in lay.wregs, f"layout {lay.probe}: register {code} is not written"
        return fbase + code

    lanes = []
    for L in xr.lanes:
        b = {"pre": [(NONE if d == NONE else src(d), [(src(s), c) for s, c in t]) for d, t in L["pre"]],
             "prod": [(src(u), src(v)) for u, v in L["prod"]],
             "lin": [(src(s), c) for s, c in L["lin"]], "dst": dst(L["dst"])}
        if xr.fused:
            b["prod2"] = [(src(u), src(v)) for u, v in L["prod2"]]
            b["lin2"] = [(src(s), c) for s, c in L["lin2"]]
            b["dst2"] = dst(L["dst2"])
        lanes.append(b)
    out = xr.with_lanes(lanes)
    assert touched(out) < lay.end, "index out of the kernels' team region"
    lo, hi = lay.pre_window.get(ctx, (0, lay.end))
    assert all(d == NONE or lo <= d < hi for L in lanes for d, _ in L["pre"]), f"layout {lay.probe}: {ctx} scratch"
    return out


def run_bound(rounds, mem):
    """Interprets bound rounds on a flat team memory (list of residues)."""
    for xr in rounds:
        for L in xr.lanes:
            for d, terms in L["pre"]:
                if d != NONE:
                    mem[d] = sum(k * mem[s] for s, k in terms) % P
        out = {}
        for L in xr.lanes:
            for pk, lk, dk in (("prod", "lin", "dst"), ("prod2", "lin2", "dst2")):
                if dk in L and L[dk] != NONE:
                    out[L[dk]] = (sum(mem[u] * mem[v] for u, v in L[pk])
                                  + sum(k * mem[s] for s, k in L[lk])) % P
        for d, v in out.items():
            mem[d] = v


def check_instances(X, seed=3):
    """Every bound instance computes the same as the abstract program."""
    rng = random.Random(seed)
    for name, binding, layout in BOUND_INSTANCES:
        ctx = X_PROGRAMS[name]
        fb = region(ctx, layout).reg_base
        rounds = [bind(xr, binding, ctx, layout) for xr in X[name]]
        mem = [rng.randrange(P) for _ in range(FULL.end)]
        mem[fb + REG["ZERO"]] = 0
        mem[fb + REG["ONE"]] = 1
        F = {r: mem[fb + r] for r in range(NREGS)}
        A = B = None
        if binding:
            bd = list(binding) + ([binding[1]] if len(binding) == 2 else [])
            A = mem[12 * SLOTS.index(bd[1]):12 * SLOTS.index(bd[1]) + 12]
            B = mem[12 * SLOTS.index(bd[2]):12 * SLOTS.index(bd[2]) + 12]
        want_D = run_xprogram(X[name], F, A, B)
        # the limb-level model of the same instance (Montgomery representatives)
        lmem = [to_limbs(v * R_MONT % P) for v in mem]
        run_bound(rounds, mem)
        run_bound_limbs(rounds, lmem)
        rinv = pow(R_MONT, -1, P)
        assert all(from_limbs(l) * rinv % P == v for l, v in zip(lmem, mem)), f"instance {name}{binding}: limb model"
        if binding:
            d0 = 12 * SLOTS.index(binding[0])
            assert all(mem[d0 + e] == v for e, v in want_D.items()), f"instance {name}{binding}"
        else:
            for r, v in F.items():
                assert mem[fb + r] == v, f"instance {name} reg {r}"


def touched(bx):
    """Largest team element index a bound round reads or writes."""
    m = 0
    for L in bx.lanes:
        idx = [L["dst"], L.get("dst2", NONE)] + [d for d, _ in L["pre"]]
        idx += [s_ for _, t in L["pre"] for s_, _ in t]
        for pk, lk in (("prod", "lin"), ("prod2", "lin2")):
            idx += [u for u, v in L.get(pk, [])] + [v for u, v in L.get(pk, [])] + [s_ for s_, _ in L.get(lk, [])]
        m = max([m] + [v for v in idx if v != NONE])
    return m


def region_ends(X):
    """{probe layout: last element + 1 that the kernels' team region must
    hold}, before rounding up to an even count (see Layout.floor)."""
    ends = {lay.probe: lay.end if lay.floor is None else lay.floor for lay in LAYOUTS}
    for name, binding, layout in BOUND_INSTANCES:
        ctx = X_PROGRAMS[name]
        lay = region(ctx, layout)
        if lay.floor is not None:
            ends[lay.probe] = max([ends[lay.probe]] + [touched(bind(xr, binding, ctx, layout)) + 1 for xr in X[name]])
    return ends


# ------------------------------------------------------------------ the instance probe's view (bn256_xprobe.h)
# hg_debug_xinst runs ONE bound instance on a raw team region (bn256_xprobe.hip).
# A probe layout is the team region a production kernel gives the instance: D
# (the full region, kTeamWords), S, T, V (the compact layouts) and F (the FOLD
# context's region): Layout.probe.
def probe_layout(name, layout):
    return region(X_PROGRAMS[name], layout).probe


def probe_region_elems(X):
    """Elements of the team region per probe layout, as the kernels size it
    (kTeamWords / 10, kSigTeamElems, kSigTTeamElems, kVTeamElems, kFoldTeamElems)."""
    return {lay: end + end % 2 for lay, end in region_ends(X).items()}


def probe_reg_base(name, layout):
    """Team element of register 0 (ZERO; ONE follows) in the instance's region."""
    return region(X_PROGRAMS[name], layout).reg_base


def instance_rounds(X, i):
    """The bound rounds of entry i of PROBE_INSTANCES: instance i of ALL_INSTANCES,
    then PAIR_INSTANCES (run_bound / run_bound_limbs run them)."""
    name, binding, layout = PROBE_INSTANCES[i]
    return [bind(xr, binding, X_PROGRAMS[name], layout) for xr in X[name]]
