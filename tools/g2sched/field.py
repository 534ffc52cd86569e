"""The field's constants, the team's register file and the expression helpers
the source programs are written with."""

P = 65000549695646603732796438742359905742825358107623003571877145026864184071783
R_BITS = 286  # Montgomery R = 2^286 (11 REDC digits, bn256_constants.h kRedcSteps)
SLOT_A = 128
SLOT_B = 160
NONE = 255

# ------------------------------------------------------------------ register file
FP_SCALARS = ["ZERO", "ONE", "PX", "PY", "SX", "NSY"]
# The kernels' register file (kG2Regs): the projective Miller-loop programs'
# point, pk, line coefficients and temporaries. FBX, FCY must stay
# consecutive (load_fixed_line: the normalised G2Base line, a = 1).
FP2_REGS = ["X", "Y", "Z", "QX", "QY", "NQY", "P1X", "P1Y", "P2X",
            "FBX", "FCY", "FB", "FC", "LA", "LB", "LC",
            # projective doubling temporaries
            "A", "B", "S", "C", "G",
            # projective addition temporaries
            "AB", "S1", "D", "I", "S2", "H", "J", "AV", "L1"]
REG = {}
for i, n in enumerate(FP_SCALARS):
    REG[n] = i
_base = len(FP_SCALARS)
for i, n in enumerate(FP2_REGS):
    REG[n + ".x"] = _base + 2 * i
    REG[n + ".y"] = _base + 2 * i + 1
NREGS = _base + 2 * len(FP2_REGS)  # kG2Regs
assert NREGS <= 128
# Fp12 source slots: Fp2 coefficient k of slot A is "A{k}", of slot B "B{k}"
for k in range(6):
    for ci, c in enumerate("xy"):
        REG[f"A{k}.{c}"] = SLOT_A + 2 * k + ci
        REG[f"B{k}.{c}"] = SLOT_B + 2 * k + ci
        REG[f"D{k}.{c}"] = SLOT_A + 2 * k + ci  # destination slot element (same encoding)


def comp(name, c):
    return REG[f"{name}.{c}"]


# ------------------------------------------------------------------ limb constants
P_LIMB_TOP = P >> 234
P_LIMBS = [(P >> (26 * j)) & ((1 << 26) - 1) for j in range(9)] + [P >> 234]

# Negations in a pre-pass or a linear term subtract x from a multiple of p
# re-spread limb-wise, (NEG_MULT p)'' below: every limb of it dominates the
# same limb of any element. Elements may be LAZY, below 2p instead of p: the
# cyclotomic squaring leaves its result unreduced (Program.lazy), so the
# multiple is 4p, whose top limb dominates the top limb of anything below 2p.
NEG_MULT = 4


def _pneg_limbs(m):
    """(m p)'': m p re-spread so limb l >= 2^26 (l < 9) and the top limb is (m p >> 234) - 1."""
    v = m * P
    q = [(v >> (26 * l)) & ((1 << 26) - 1) for l in range(9)] + [v >> 234]
    out = [q[0] + (1 << 26)] + [q[l] + (1 << 26) - 1 for l in range(1, 9)] + [q[9] - 1]
    assert sum(x << (26 * l) for l, x in enumerate(out)) == v
    return out


P2N = _pneg_limbs(NEG_MULT)                          # the negation constant (HG_P2N)
LAZY_LIMB = [(1 << 26) - 1] * 9 + [(2 * P - 1) >> 234]  # limb bounds of an element below 2p
assert all(a <= b for a, b in zip(LAZY_LIMB, P2N)), "the negation constant must dominate every element"

# The one-chain reduction tail (bn256_redq.h redq_tail<QMAX, LAZY>): the
# quotient estimate q = floor(t / (p9 + 1)), t = c9 + floor(c8 / 2^26), is taken
# from the top two columns before they are normalised, and q (Z - p) is added
# limb by limb in the normalising chain (Z: zero re-spread, REDQ_Z).
ONE_CHAIN_QMAX_LIMIT = 64   # kRedqMaxQ
ONE_CHAIN_COMPARE_Q = 2     # kRedqCompareQ: up to here q is a sum of compares
REDQ_Z = [1 << 26] + [(1 << 26) - 1] * 8
assert sum(z << (26 * j) for j, z in enumerate(REDQ_Z)) == 1 << 234


# ------------------------------------------------------------------ expression helpers
# An Fp2 linear combination is a list of (fp2_name, coef); its component c is
# the Fp lincomb [(reg(name.c), coef)].
def fp2_comp(lc, c):
    return [(comp(n, c), k) for n, k in lc]


def neg(terms):
    return [(r, -k) for r, k in terms]


def scale(terms, s):
    return [(r, k * s) for r, k in terms]


def add(*ts):
    out = {}
    for t in ts:
        for r, k in t:
            out[r] = out.get(r, 0) + k
    return [(r, k) for r, k in out.items() if k != 0] or [(REG["ZERO"], 1)]


def one():
    return [(REG["ONE"], 1)]


def scal(name):
    return [(REG[name], 1)]


class Lane:
    def __init__(self, dst, slots):
        self.dst = dst
        self.slots = slots  # list of (A_terms, B_terms)


def sq(dst, U):
    """dst (Fp2) = U^2 : two lanes (x, y)."""
    ux, uy = fp2_comp(U, "x"), fp2_comp(U, "y")
    return [Lane(comp(dst, "x"), [(add(ux, ux), uy)]),
            Lane(comp(dst, "y"), [(add(uy, ux), add(uy, neg(ux)))])]


def mul(dst, U, V):
    """dst (Fp2) = U * V."""
    ux, uy = fp2_comp(U, "x"), fp2_comp(U, "y")
    vx, vy = fp2_comp(V, "x"), fp2_comp(V, "y")
    return [Lane(comp(dst, "x"), [(ux, vy), (uy, vx)]),
            Lane(comp(dst, "y"), [(uy, vy), (neg(ux), vx)])]


def smul(dst, U, s_name, k=1):
    """dst (Fp2) = k * U * s (s an Fp scalar register)."""
    return [Lane(comp(dst, c), [([(r, kk * k) for r, kk in fp2_comp(U, c)], scal(s_name))]) for c in ("x", "y")]


def lin(dst, U):
    return [Lane(comp(dst, c), [(fp2_comp(U, c), one())]) for c in ("x", "y")]


# Fp-level product terms of Fp2 expressions, for building sums per component.
def prod_terms(U, V, c, k=1):
    """component c of k * U * V as a list of Fp slots."""
    ux, uy = fp2_comp(U, "x"), fp2_comp(U, "y")
    vx, vy = fp2_comp(V, "x"), fp2_comp(V, "y")
    if c == "x":
        return [(scale(ux, k), vy), (scale(uy, k), vx)]
    return [(scale(uy, k), vy), (scale(neg(ux), k), vx)]


def sq_terms(U, c, k=1):
    ux, uy = fp2_comp(U, "x"), fp2_comp(U, "y")
    if c == "x":
        return [(scale(add(ux, ux), k), uy)]
    return [(scale(add(uy, ux), k), add(uy, neg(ux)))]


def xi_terms(slots_x, slots_y, c):
    """component c of xi * Z where Z = (sum slots_x, sum slots_y):
    xi Z = (3 Zx + Zy) i + (3 Zy - Zx)."""
    if c == "x":
        return [(scale(a, 3), b) for a, b in slots_x] + list(slots_y)
    return [(scale(a, 3), b) for a, b in slots_y] + [(neg(a), b) for a, b in slots_x]


def xi_lc(lx, ly):
    """components of xi * (lx i + ly) for Fp lincombs lx, ly: (3lx + ly, 3ly - lx)."""
    return add(scale(lx, 3), ly), add(scale(ly, 3), neg(lx))
