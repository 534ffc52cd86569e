"""CPU suite: the edge corpus of the per-thread field and curve arithmetic
(handel_amd/csrc/bn256_fp.h, bn256_curve.h) and its expected results from
plain Python integers, for the probe hg_debug_field (bn256_fprobe.hip).

This module builds, per probe op, the case list and what the GPU must return
(fixed seed, no GPU imports); tests/test_gpu_field.py runs each list in one
launch and compares. An element is ten 26-bit limbs, value sum l_i 2^(26 i),
Montgomery form with R = 2^286; the field ops are given RAW limb values v in
[0, p) (so the corpus chooses the limb patterns: fp_mul(a, b) must be the
canonical limbs of a b R^-1 mod p), the curve ops Montgomery forms of the
oracle's residues. The group law is oracle/bn256_oracle.py's, and a curve
result is compared as a POINT (canonical limbs, Z == 0 exactly for infinity,
else the oracle's affine point), which no change of formulas invalidates.

The tests here check what the GPU comparison relies on:
  * an integer REDC model pre(T) = (T + ((-T p^-1) mod R) p) / R classifies
    every reduction of the multiplying ops into: guard false; guard true and
    the value kept (pre >> 234 >= p >> 234, pre < p); guard true and p
    subtracted (pre >= p). Every reduction has a case in every class
    (test_rare_subtractions_are_taken);
  * the named field edges (a + b in {p-1, p, p+1, 2p-2}, a - b in {-1, 0, 1},
    the byte-op integers at all four byte offsets) and the named curve classes
    (the same point under two Z, opposite points, infinities in both forms,
    the order-13 twist point's coincidences) are present, and the oracle gives
    each exceptional pair its kind;
  * every input lies in its function's domain.
"""

import functools
import os
import random
import re

import numpy as np

from oracle import bn256_oracle as O
from tests import _fixtures as FX

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
P = O.P
SEED = 20241021
LIMB_BITS = 26
MASK = (1 << LIMB_BITS) - 1
R = 1 << 286
RP = R % P
RINV = pow(R, -1, P)
PINV = pow(P, -1, R)
PTOP = P >> 234
MAX_CASES = 512

# name: (op number, words in, words out) — the table of bn256_fprobe.hip (test_op_table_matches_the_probe_source)
OPS = {
    "fp_add": (0, 20, 10), "fp_sub": (1, 20, 10), "fp_neg": (2, 10, 10), "fp_dbl": (3, 10, 10),
    "fp_mul3": (4, 10, 10), "fp_mul": (5, 20, 10), "fp_sqr": (6, 10, 10), "fp_inv": (7, 10, 10),
    "fp_neg_loose": (8, 10, 10), "fp_add_loose": (9, 20, 10), "fp_to_mont": (10, 8, 10),
    "fp_from_mont": (11, 10, 8), "fp_from_be": (12, 10, 12), "fp_to_be": (13, 10, 8),
    "f2_mul": (14, 40, 20), "f2_sqr": (15, 20, 20), "f2_muls": (16, 30, 20), "f2_mul_xi": (17, 20, 20),
    "f2_inv": (18, 20, 20), "f2_sub": (19, 40, 20), "f2_neg": (20, 20, 20), "f2_conj": (21, 20, 20),
    "g1_double": (22, 30, 30), "g1_add": (23, 60, 30), "g1_madd": (24, 50, 30), "g1_on_curve": (25, 20, 1),
    "g1_affine": (26, 30, 20), "g2_double": (27, 60, 60), "g2_add": (28, 120, 60), "g2_madd": (29, 100, 60),
    "g2_add_affine": (30, 100, 60), "g2_on_curve": (31, 40, 1), "g2_affine": (32, 60, 40),
}
POINT_OPS = ("g1_double", "g1_add", "g1_madd", "g2_double", "g2_add", "g2_madd", "g2_add_affine")
PAIR_OPS = ("g1_add", "g1_madd", "g2_add", "g2_madd", "g2_add_affine")
# ops whose operands are not all ten-limb elements
WORD_OPS = ("fp_to_mont", "fp_from_be")


# ------------------------------------------------------------------ limbs and words
def limbs(v):
    """The normalised limbs of 0 <= v < 2^260 (limb 9 holds what is left)."""
    assert 0 <= v < 1 << 260
    return [(v >> (LIMB_BITS * i)) & MASK for i in range(9)] + [v >> 234]


def val(l):
    return sum(int(x) << (LIMB_BITS * i) for i, x in enumerate(l))


def words8(v):
    return [(v >> (32 * i)) & 0xFFFFFFFF for i in range(8)]


def mont(a):
    """Residue -> the limbs of its canonical Montgomery representative."""
    return limbs(a % P * R % P)


def is_canonical(l):
    return all(0 <= int(x) <= MASK for x in l) and val(l) < P


def be_words(b):
    """Bytes as the little-endian 32-bit words a device buffer holds them in."""
    return [int(x) for x in np.frombuffer(bytes(b), dtype="<u4")]


class Case:
    """label; inp: the words in; want: the words out (None for a point op);
    args: the operands as integers; group, expect, kind: a point op's curve,
    the oracle's affine result (None: infinity) and the pair's class."""

    def __init__(self, label, inp, want=None, args=(), group=None, expect=None, kind=None):
        self.label, self.inp, self.want, self.args = label, inp, want, args
        self.group, self.expect, self.kind = group, expect, kind


# ------------------------------------------------------------------ the REDC model
def pre(T):
    """What acc_redc leaves before the guarded subtraction, as an integer."""
    m = (-T * PINV) % R
    q, rem = divmod(T + m * P, R)
    assert rem == 0
    return q


CLASSES = ("guard_false", "kept", "subtracted")


def classify(T):
    v = pre(T)
    if v >> 234 < PTOP:
        return "guard_false"
    return "kept" if v < P else "subtracted"


def reductions(op, args):
    """The (name, T) of every REDC input the multiplying op `op` forms from raw operands."""
    if op == "fp_mul":
        return [("fp_mul", args[0] * args[1])]
    if op == "fp_sqr":
        return [("fp_sqr", args[0] ** 2)]
    if op == "f2_mul":
        ax, ay, bx, by = args
        return [("f2_mul.re", ay * by + (P - ax) * bx), ("f2_mul.im", ax * by + ay * bx)]  # fp_neg_loose(0) = p
    if op == "f2_sqr":
        ax, ay = args
        return [("f2_sqr.re", (ay + ax) * ((ay - ax) % P)), ("f2_sqr.im", 2 * ax * ay)]
    if op == "f2_muls":
        ax, ay, s = args
        return [("f2_muls.x", ax * s), ("f2_muls.y", ay * s)]
    if op == "f2_inv":
        ax, ay = args
        return [("f2_inv.norm", ax * ax + ay * ay)]
    return []


REDUCTIONS = ("fp_mul", "fp_sqr", "f2_mul.re", "f2_mul.im", "f2_sqr.re", "f2_sqr.im", "f2_muls.x", "f2_muls.y",
              "f2_inv.norm")
MUL_OPS = ("fp_mul", "fp_sqr", "f2_mul", "f2_sqr", "f2_muls", "f2_inv")


# ------------------------------------------------------------------ field values
def _ones_below_p():
    """All-ones limb patterns below p: limbs 0..8 full, and with the largest limb 9 that stays below p."""
    low = (1 << 234) - 1
    return [("ones234", low), ("ones_top", ((PTOP - 1) << 234) | low), ("ones26", MASK)]


EDGES = [("0", 0), ("1", 1), ("2", 2), ("p-2", P - 2), ("p-1", P - 1), ("(p-1)/2", (P - 1) // 2),
         ("(p+1)/2", (P + 1) // 2), ("R", RP), ("p-R", P - RP), ("ptop<<234", PTOP << 234)] + _ones_below_p()
KEPT_S = P - 5           # a canonical result in [2^234 (p >> 234), p): guard true, value kept
SUB_S = (1, 2, 3)        # small canonical results: pre = s + p, p subtracted

BYTE_INTS = [("0", 0), ("1", 1), ("p-1", P - 1), ("p", P), ("p+1", P + 1), ("2^255", 1 << 255),
             ("2^256-p-1", (1 << 256) - P - 1), ("2^256-p", (1 << 256) - P), ("2^256-1", (1 << 256) - 1)] + \
            [(f"byte{k}", ((0xA1 + 5 * k) & 0xFF | 1) << (8 * (31 - k))) for k in range(32)]


def _sqrt(a):
    r = pow(a % P, (P + 1) // 4, P)
    return r if r * r % P == a % P else None


def _fp_case(label, args, want_vals):
    return Case(label, [w for a in args for w in limbs(a)], [w for v in want_vals for w in limbs(v)], tuple(args))


def _pairs(rng, nrand=40):
    out = [(f"{na},{nb}", a, b) for na, a in EDGES for nb, b in EDGES]
    out += [(f"rand{i}", rng.randrange(P), rng.randrange(P)) for i in range(nrand)]
    return out


def _sum_diff_pairs(rng):
    """a + b in {p-1, p, p+1, 2p-2} and a - b in {-1, 0, 1}."""
    out = [("sum=2p-2", P - 1, P - 1)]
    for i in range(4):
        a = rng.randrange(2, P - 1)
        out += [(f"sum=p-1#{i}", a, P - 1 - a), (f"sum=p#{i}", a, P - a), (f"sum=p+1#{i}", a, P + 1 - a),
                (f"diff=-1#{i}", a, a + 1), (f"diff=0#{i}", a, a), (f"diff=1#{i}", a, a - 1)]
    return out


def _singles(rng, nrand=40):
    return list(EDGES) + [(f"rand{i}", rng.randrange(P)) for i in range(nrand)]


def _product_recipes(rng, tag, n=3):
    """(label, a, b) with a b = s R mod p: s = p - 5 (kept), s in {1, 2, 3} (subtracted)."""
    out = []
    for i in range(n):
        for s in (KEPT_S,) + SUB_S:
            a = rng.randrange(2, P)
            out.append((f"{tag}:s={'p-5' if s == KEPT_S else s}#{i}", a, s * R * pow(a, -1, P) % P))
    return out


def _square_recipes():
    """(label, a) with a^2 = s R mod p for the s nearest p - 5 and nearest 1 for which s R is a square."""
    out = []
    for name, start, step in (("kept", KEPT_S, -1), ("sub", 1, 1)):
        s, found = start, 0
        while found < 3:
            a = _sqrt(s * R)
            if a is not None:
                tag = f"sqr:{name}:s={'p-' + str(P - s) if step < 0 else s}"
                out += [(tag, a), (tag + ":other root", P - a)]  # s a power of 4: one root is 2^k, and pre = s
                found += 1
            s += step
    return out


# ------------------------------------------------------------------ the Fp and byte corpora
def _build_fp(op, rng):
    two = {"fp_add": lambda a, b: (a + b) % P, "fp_sub": lambda a, b: (a - b) % P,
           "fp_mul": lambda a, b: a * b * RINV % P}
    one = {"fp_neg": lambda a: -a % P, "fp_dbl": lambda a: 2 * a % P, "fp_mul3": lambda a: 3 * a % P,
           "fp_sqr": lambda a: a * a * RINV % P,
           "fp_inv": lambda a: 0 if a == 0 else R * R * pow(a, -1, P) % P,  # (a / R)^-1 R
           "fp_neg_loose": lambda a: P - a}                                # p for a = 0: not reduced
    if op in two:
        ps = _pairs(rng)
        ps += _sum_diff_pairs(rng) if op != "fp_mul" else _product_recipes(rng, "mul")
        return [_fp_case(lb, (a, b), (two[op](a, b),)) for lb, a, b in ps]
    if op == "fp_add_loose":
        cs = []
        for lb, a, b in _pairs(rng) + _sum_diff_pairs(rng):
            cs.append(Case(lb, limbs(a) + limbs(b), [x + y for x, y in zip(limbs(a), limbs(b))], (a, b)))
        return cs
    ss = _singles(rng)
    if op in ("fp_dbl", "fp_mul3"):
        # 2a and 3a next to p and 2p
        ss += [(f"{k}p/{d}{'+1' if e else ''}", k * P // d + e) for d in (2, 3) for k in range(1, d) for e in (0, 1)]
    if op == "fp_sqr":
        ss += _square_recipes()
    return [_fp_case(lb, (a,), (one[op](a),)) for lb, a in ss]


def _build_bytes(op, rng):
    ints = BYTE_INTS + [(f"rand{i}", rng.getrandbits(256)) for i in range(12)]
    if op == "fp_to_mont":
        return [Case(lb, words8(w), limbs(w * R % P), (w,)) for lb, w in ints]
    if op == "fp_from_be":
        cs = []
        for lb, w in ints:
            for k in range(4):
                buf = bytearray(rng.getrandbits(8) | 1 for _ in range(36))  # nonzero bytes around the coordinate
                buf[k:k + 32] = w.to_bytes(32, "big")
                cs.append(Case(f"{lb}@{k}", [k] + be_words(buf), limbs(w * R % P) + [int(w >= P), int(w != 0)],
                               (w, k)))
        return cs
    # the two ways out: canonical elements whose residues are the integers below p, the edges, random ones
    elems = [(f"int:{lb}", w * R % P) for lb, w in ints if w < P] + _singles(rng)
    if op == "fp_from_mont":
        return [Case(lb, limbs(a), words8(a * RINV % P), (a,)) for lb, a in elems]
    assert op == "fp_to_be"
    return [Case(lb, limbs(a), be_words((a * RINV % P).to_bytes(32, "big")), (a,)) for lb, a in elems]


# ------------------------------------------------------------------ the Fp2 corpus
def _f2_want(op, args):
    if op == "f2_mul":
        return O.f2_muls(O.f2_mul(args[0:2], args[2:4]), RINV)
    if op == "f2_sqr":
        return O.f2_muls(O.f2_sqr(args[0:2]), RINV)
    if op == "f2_muls":
        return O.f2_muls(O.f2_muls(args[0:2], args[2]), RINV)
    if op == "f2_mul_xi":
        return O.f2_mul_xi(args)
    if op == "f2_inv":
        return (0, 0) if args == (0, 0) else O.f2_muls(O.f2_inv(args), R * R % P)
    if op == "f2_sub":
        return O.f2_sub(args[0:2], args[2:4])
    if op == "f2_neg":
        return O.f2_neg(args)
    assert op == "f2_conj"
    return O.f2_conj(args)


def _build_f2(op, rng):
    ev = [v for _, v in EDGES]
    pick = lambda: rng.choice(ev) if rng.random() < 0.7 else rng.randrange(P)  # noqa: E731
    nargs = OPS[op][1] // 10
    cs = []
    for na, a in EDGES:
        for nb, b in EDGES:
            cs.append((f"{na},{nb}", (a, b) + tuple(pick() for _ in range(nargs - 2))))
    cs += [(f"mix{i}", tuple(pick() for _ in range(nargs))) for i in range(60)]
    cs += [(f"rand{i}", tuple(rng.randrange(P) for _ in range(nargs))) for i in range(40)]
    if op == "f2_mul":
        for lb, a, b in _product_recipes(rng, "re"):        # re = ay by with bx = 0
            cs.append((lb, (rng.randrange(P), a, 0, b)))
        for lb, a, b in _product_recipes(rng, "im"):        # im = ax by with ay = 0
            cs.append((lb, (a, 0, rng.randrange(P), b)))
        for i in range(3):                                  # ax = 0: the real part holds p bx
            cs.append((f"ax=0#{i}", (0, rng.randrange(P), rng.randrange(1, P), rng.randrange(P))))
            cs.append((f"ax=ay=0#{i}", (0, 0, rng.randrange(1, P), rng.randrange(P))))  # pre = p exactly, result 0
    if op == "f2_sqr":
        cs += [("x=y=p-1", (P - 1, P - 1))] + [(f"x=y#{i}", (v, v)) for i, v in enumerate((1, rng.randrange(P)))]
        half = pow(2, -1, P)
        for lb, s, d in _product_recipes(rng, "re", n=6):   # (y + x)(y - x) = s R
            cs.append((lb, ((s - d) * half % P, (s + d) * half % P)))
        for lb, a, b in _product_recipes(rng, "im", n=6):   # 2 x y = s R
            cs.append((lb, (a, b * half % P)))
    if op == "f2_muls":
        for lb, a, s in _product_recipes(rng, "x"):
            cs.append((lb, (a, rng.randrange(P), s)))
        for lb, a, s in _product_recipes(rng, "y"):
            cs.append((lb, (rng.randrange(P), a, s)))
    if op == "f2_inv":
        cs.append(("zero", (0, 0)))
        for s in (KEPT_S,) + SUB_S:                         # x^2 + y^2 = s R
            found = 0
            while found < 3:
                x = rng.randrange(P)
                y = _sqrt(s * R - x * x)
                if y is not None:
                    cs.append((f"norm:s={'p-5' if s == KEPT_S else s}#{found}", (x, y)))
                    found += 1
    out = []
    for lb, args in cs:
        want = _f2_want(op, args)
        out.append(Case(lb, [w for a in args for w in limbs(a)], limbs(want[0] % P) + limbs(want[1] % P), args))
    return out


# ------------------------------------------------------------------ the curve corpora
class Group:
    def __init__(self, name, F, gen, on_curve):
        self.name, self.F, self.gen, self.on_curve = name, F, gen, on_curve
        self.fp2 = name == "g2"

    def flat(self, coords):
        """Coordinates -> the Fp residues in the order the probe takes them."""
        return [v for c in coords for v in (c if self.fp2 else (c,))]

    def words(self, coords):
        return [w for v in self.flat(coords) for w in mont(v)]

    def coords(self, residues):
        return [tuple(residues[i:i + 2]) for i in range(0, len(residues), 2)] if self.fp2 else list(residues)

    def jac(self, aff, z):
        F = self.F
        z2 = F.sqr(z)
        return (F.mul(aff[0], z2), F.mul(aff[1], F.mul(z2, z)), z)

    def neg(self, aff):
        return (aff[0], self.F.sub(self.F.zero, aff[1]))

    def rand_elem(self, rng):
        return (rng.randrange(P), rng.randrange(1, P)) if self.fp2 else rng.randrange(1, P)

    def elem(self, v):
        return (0, v % P) if self.fp2 else v % P

    def mul(self, aff, k):
        return O.jac_affine(self.F, O.jac_mul(self.F, O.to_jac(self.F, aff), k))


G1 = Group("g1", O.FP_OPS, O.G1_GEN, O.g1_on_curve)
G2 = Group("g2", O.FP2_OPS, O.G2_GEN, O.g2_on_curve)
GROUPS = {"g1": G1, "g2": G2}


@functools.lru_cache(maxsize=None)
def _points(name):
    """P, Q: random multiples of the generator; zs: the Z of the Jacobian forms;
    infs: infinity as (1, 1, 0) and as (random, random, 0)."""
    g = GROUPS[name]
    rng = random.Random(f"{SEED}-{name}")
    pt = g.mul(g.gen, rng.randrange(2, O.ORDER))
    q = g.mul(g.gen, rng.randrange(2, O.ORDER))
    zs = [("Z=1", g.elem(1)), ("Z=p-1", g.elem(P - 1)), ("Z=rand", g.rand_elem(rng))]
    infs = [("inf(1,1,0)", (g.F.one, g.F.one, g.F.zero)),
            ("inf(rand,rand,0)", (g.rand_elem(rng), g.rand_elem(rng), g.F.zero))]
    return pt, q, zs, infs, g.rand_elem(rng)


@functools.lru_cache(maxsize=None)
def _t13():
    return FX.small_order_points()[13]


def _pair_case(g, label, kind, a, b, b_affine):
    """a: Jacobian; b: Jacobian, or affine when the op takes an affine operand."""
    bj = O.to_jac(g.F, b) if b_affine else b
    expect = O.jac_affine(g.F, O.jac_add(g.F, a, bj))
    return Case(label, g.words(a) + g.words(b), None, (a, bj), g.name, expect, kind)


def _build_pairs(op):
    g = GROUPS[op[:2]]
    aff = not op.endswith("_add")           # madd, add_affine: the second operand is affine
    pt, q, zs, infs, _ = _points(g.name)
    bzs = [("affine", None)] if aff else zs
    second = lambda a, z: a if aff else g.jac(a, z)  # noqa: E731
    cs = []
    for na, za in zs:
        for nb, zb in bzs:
            same = "equal Z" if na == (nb if not aff else "Z=1") else "different Z"  # an affine operand has Z = 1
            cs.append(_pair_case(g, f"P+Q generic {na} {nb}", "generic", g.jac(pt, za), second(q, zb), aff))
            cs.append(_pair_case(g, f"P+P {same} {na} {nb}", "doubling", g.jac(pt, za), second(pt, zb), aff))
            cs.append(_pair_case(g, f"P+(-P) {same} {na} {nb}", "infinity", g.jac(pt, za), second(g.neg(pt), zb),
                                 aff))
    for ni, inf in infs:
        for nb, zb in bzs:
            cs.append(_pair_case(g, f"inf+P {ni} {nb}", "left_inf", inf, second(pt, zb), aff))
        if not aff:
            for na, za in zs:
                cs.append(_pair_case(g, f"P+inf {na} {ni}", "right_inf", g.jac(pt, za), inf, False))
            for nj, inf2 in infs:
                cs.append(_pair_case(g, f"inf+inf {ni} {nj}", "both_inf", inf, inf2, False))
    if g.fp2:
        t = _t13()
        mult = {k: g.mul(t, k) for k in range(1, 13)}
        for k in range(1, 13):
            na, za = zs[k % 3]
            nb, zb = bzs[(k // 3) % len(bzs)]
            cs.append(_pair_case(g, f"order13 {k}T+{13 - k}T {na} {nb}", "infinity", g.jac(mult[k], za),
                                 second(mult[13 - k], zb), aff))
        for na, za in zs:
            nb, zb = bzs[-1]
            cs.append(_pair_case(g, f"order13 6T+6T {na} {nb}", "doubling", g.jac(mult[6], za), second(mult[6], zb),
                                 aff))
    return cs


def _build_double(op):
    g = GROUPS[op[:2]]
    pt, q, zs, infs, _ = _points(g.name)
    cs = []
    for lb, a in [(f"P {n}", g.jac(pt, z)) for n, z in zs] + [(f"Q generic {n}", g.jac(q, z)) for n, z in zs[2:]] + \
                 list(infs) + ([(f"order13 {k}T", g.jac(g.mul(_t13(), k), zs[k % 3][1])) for k in (1, 6, 12)]
                               if g.fp2 else []):
        kind = "infinity" if g.F.is_zero(a[2]) else "generic"
        cs.append(Case(lb, g.words(a), None, (a,), g.name, O.jac_affine(g.F, O.jac_double(g.F, a)), kind))
    return cs


def _build_on_curve(op):
    g = GROUPS[op[:2]]
    pt, q, _, _, rnd = _points(g.name)
    F = g.F
    bump = lambda c: F.add(c, F.one)  # noqa: E731
    cs = [("P", pt), ("Q", q), ("-P", g.neg(pt)), ("generator", g.gen), ("-generator", g.neg(g.gen)),
          ("P x+1", (bump(pt[0]), pt[1])), ("P y+1", (pt[0], bump(pt[1]))),
          ("P x-1", (F.sub(pt[0], F.one), pt[1])), ("P y-1", (pt[0], F.sub(pt[1], F.one))),
          ("(0,0)", (F.zero, F.zero)), ("(0,y)", (F.zero, pt[1])), ("(x,0)", (pt[0], F.zero)),
          ("(Px,Qy)", (pt[0], q[1])), ("(rand,rand)", (rnd, g.neg((rnd, rnd))[1]))]
    if g.fp2:
        t = _t13()
        cs += [("order13 T", t), ("P x.y+1", ((pt[0][0], (pt[0][1] + 1) % P), pt[1])),
               ("P y.x+1", (pt[0], ((pt[1][0] + 1) % P, pt[1][1])))]
    else:
        y0 = _sqrt(O.CURVE_B)
        if y0 is not None:
            cs.append(("(0,sqrt b)", (0, y0)))
    return [Case(lb, g.words(c), [int(bool(g.on_curve(*c)))], c, g.name) for lb, c in cs]


def _build_affine(op):
    g = GROUPS[op[:2]]
    pt, q, zs, infs, _ = _points(g.name)
    cs = [(f"{nm} {n}", g.jac(a, z), a) for nm, a in (("P", pt), ("Q", q), ("generator", g.gen)) for n, z in zs]
    cs += [(n, inf, (g.F.zero, g.F.zero)) for n, inf in infs]  # fp_inv(0) = 0: infinity gives (0, 0)
    return [Case(lb, g.words(a), g.words(want), (a,), g.name) for lb, a, want in cs]


@functools.lru_cache(maxsize=None)
def cases(op):
    rng = random.Random(f"{SEED}-{op}")
    if op in ("fp_to_mont", "fp_from_mont", "fp_from_be", "fp_to_be"):
        return _build_bytes(op, rng)
    if op.startswith("fp_"):
        return _build_fp(op, rng)
    if op.startswith("f2_"):
        return _build_f2(op, rng)
    if op in PAIR_OPS:
        return _build_pairs(op)
    if op.endswith("_double"):
        return _build_double(op)
    if op.endswith("_on_curve"):
        return _build_on_curve(op)
    assert op.endswith("_affine")
    return _build_affine(op)


def inputs(op):
    return np.array([c.inp for c in cases(op)], dtype=np.uint32)


# ------------------------------------------------------------------ the comparison the GPU test makes
def mismatch(op, case, got):
    """None when the words `got` are what the probe must return for `case`,
    else a message naming the first differing word and both values."""
    got = [int(w) for w in got]
    assert len(got) == OPS[op][2]
    if case.want is not None:
        for w, (a, b) in enumerate(zip(got, case.want)):
            if a != b:
                return f"word {w}: GPU 0x{a:08x}, model 0x{b:08x}"
        return None
    g = GROUPS[case.group]
    for e in range(len(got) // 10):
        if not is_canonical(got[10 * e:10 * e + 10]):
            w = next((10 * e + i for i in range(10) if got[10 * e + i] > MASK), 10 * e + 9)
            return f"word {w}: GPU 0x{got[w]:08x} in element {e}, which is not canonical (limbs below 2^26, value < p)"
    x, y, z = g.coords([val(got[10 * e:10 * e + 10]) * RINV % P for e in range(len(got) // 10)])
    nz = len(got) // 30 * 10
    if g.F.is_zero(z):
        if case.expect is None:
            return None
        return f"word {2 * nz}: GPU Z = 0 (infinity), model the finite point {case.expect}"
    if case.expect is None:
        w = next(i for i in range(2 * nz, 3 * nz) if got[i])
        return f"word {w}: GPU 0x{got[w]:08x} (Z != 0, a finite point), model 0 (infinity)"
    have = O.jac_affine(g.F, (x, y, z))
    if have != case.expect:
        w = 0 if have[0] != case.expect[0] else nz
        return (f"word {w}: GPU 0x{got[w]:08x}; as a point the GPU gives {have}, "
                f"model {case.expect} ({'X/Z^2' if w == 0 else 'Y/Z^3'} differs)")
    return None


def model_output(op, case):
    """One output the comparison accepts: the expected words, or for a point op
    the oracle's own Jacobian result in Montgomery form."""
    if case.want is not None:
        return list(case.want)
    g = GROUPS[case.group]
    r = O.jac_double(g.F, case.args[0]) if op.endswith("_double") else O.jac_add(g.F, *case.args)
    return g.words(r)


def reduction_counts():
    """{reduction: {class: cases}} over the corpora of the multiplying ops."""
    tot = {r: dict.fromkeys(CLASSES, 0) for r in REDUCTIONS}
    for op in MUL_OPS:
        for c in cases(op):
            for name, T in reductions(op, c.args):
                tot[name][classify(T)] += 1
    return tot


def curve_classes(op):
    """{class name: cases} of a pair op's corpus, by the named classes of the issue."""
    names = ["P+Q generic", "P+P equal Z", "P+P different Z", "P+(-P) equal Z", "P+(-P) different Z", "inf+P"]
    if op.endswith("_add"):
        names += ["P+inf", "inf+inf"]
    if op.startswith("g2"):
        names += [f"order13 {k}T+{13 - k}T" for k in range(1, 13)] + ["order13 6T+6T"]
    return {n: [c for c in cases(op) if c.label.startswith(n + " ")] for n in names}


# ------------------------------------------------------------------ the tests
def test_op_table_matches_the_probe_source():
    with open(os.path.join(ROOT, "handel_amd", "csrc", "bn256_fprobe.hip")) as f:
        rows = re.findall(r"^\s*X\((\d+), (\w+), (\d+), (\d+)\)", f.read(), flags=re.M)
    assert {name.lower(): (int(n), int(i), int(o)) for n, name, i, o in rows} == OPS
    assert sorted(v[0] for v in OPS.values()) == list(range(len(OPS)))


def test_every_op_is_one_launch_of_well_formed_cases():
    for op, (_, wi, wo) in OPS.items():
        cs = cases(op)
        assert 1 <= len(cs) <= MAX_CASES, (op, len(cs))
        assert len({c.label for c in cs}) == len(cs), op
        for c in cs:
            assert len(c.inp) == wi and all(0 <= w < 1 << 32 for w in c.inp), (op, c.label)
            assert (c.want is None) == (op in POINT_OPS), (op, c.label)
            if c.want is not None:
                assert len(c.want) == wo and all(0 <= w < 1 << 32 for w in c.want), (op, c.label)


def test_every_input_lies_in_its_domain():
    for op in OPS:
        for c in cases(op):
            if op == "fp_to_mont":
                assert 0 <= c.args[0] < 1 << 256 and c.inp == words8(c.args[0])
                continue
            if op == "fp_from_be":
                w, k = c.args
                assert c.inp[0] == k and 0 <= k < 4 and 0 <= w < 1 << 256
                buf = b"".join(int(x).to_bytes(4, "little") for x in c.inp[1:])
                assert len(buf) == 36 and buf[k:k + 32] == w.to_bytes(32, "big"), c.label
                continue
            elems = [c.inp[i:i + 10] for i in range(0, len(c.inp), 10)]
            assert all(is_canonical(e) for e in elems), (op, c.label)
            if c.group is None:
                assert [val(e) for e in elems] == list(c.args), (op, c.label)
                continue
            g = GROUPS[c.group]
            res = g.coords([val(e) * RINV % P for e in elems])
            if op in POINT_OPS:
                n2 = len(res) - 3
                pts = [tuple(res[0:3])] + ([tuple(res[3:6])] if n2 == 3 else [])
                for x, y, z in pts:  # on the curve, Y^2 = X^3 + b Z^6, or at infinity
                    z6 = g.F.sqr(g.F.mul(g.F.sqr(z), z))
                    assert g.F.is_zero(z) or g.F.sub(g.F.sqr(y), g.F.add(g.F.mul(g.F.sqr(x), x), g.F.mul(g.F.b, z6))) \
                        == g.F.zero, (op, c.label)
                if n2 == 2:          # the affine operand: a finite point of the curve
                    assert g.on_curve(*res[3:5]), (op, c.label)


def test_the_redc_model_is_consistent_with_the_expected_results():
    """pre = T / R mod p, pre < 2p, and where the op's result is that reduction
    alone, the expected limbs are pre reduced once."""
    direct = {"fp_mul": [0], "fp_sqr": [0], "f2_mul": [1, 0], "f2_sqr": [1, 0], "f2_muls": [0, 1]}
    n = 0
    for op in MUL_OPS:
        for c in cases(op):
            for k, (name, T) in enumerate(reductions(op, c.args)):
                v = pre(T)
                assert T < P * R and v < 2 * P and v % P == T * RINV % P, (name, c.label)
                if op in direct:
                    e = direct[op][k]
                    assert val(c.want[10 * e:10 * e + 10]) == (v - P if v >= P else v), (name, c.label)
                n += 1
    assert n > 1000


def test_rare_subtractions_are_taken():
    """Every reduction of the multiplying ops has a case with the guard false,
    one with the guard true and the value kept, one with p subtracted."""
    tot = reduction_counts()
    assert set(tot) == set(REDUCTIONS)
    for name in REDUCTIONS:
        for cl in CLASSES:
            assert tot[name][cl] >= 1, (name, cl, tot[name])
    by = {c.label: c for c in cases("f2_mul")}
    c = by["ax=ay=0#0"]  # pre is exactly p: the result must be 0
    assert pre(reductions("f2_mul", c.args)[0][1]) == P and c.want[10:20] == [0] * 10
    c = {c.label: c for c in cases("f2_sqr")}["x=y=p-1"]
    assert sum(limbs(P - 1)) * 2 == sum(x + y for x, y in zip(limbs(c.args[0]), limbs(c.args[1])))  # loose 2p - 2


def test_field_edges_are_present():
    for op in ("fp_add", "fp_sub", "fp_add_loose"):
        sums = {a + b for c in cases(op) for a, b in [c.args]}
        diffs = {a - b for c in cases(op) for a, b in [c.args]}
        assert {P - 1, P, P + 1, 2 * P - 2} <= sums and {-1, 0, 1} <= diffs, op
        have = {c.args for c in cases(op)}
        assert all((a, b) in have for _, a in EDGES for _, b in EDGES), op
    assert {P - 1, P + 1, 2 * P - 2} <= {2 * c.args[0] for c in cases("fp_dbl")}
    triples = {3 * c.args[0] for c in cases("fp_mul3")}
    assert any(P <= t <= P + 2 for t in triples) and any(P - 3 <= t < P for t in triples)
    assert any(2 * P <= t <= 2 * P + 2 for t in triples) and any(2 * P - 3 <= t < 2 * P for t in triples)
    for op in ("fp_neg", "fp_neg_loose", "fp_inv", "fp_sqr", "fp_dbl", "fp_mul3"):
        assert {v for _, v in EDGES} <= {c.args[0] for c in cases(op)}, op
    assert {c.label: c for c in cases("fp_neg_loose")}["0"].want == limbs(P)
    assert {c.label: c for c in cases("fp_inv")}["0"].want == [0] * 10
    assert {c.label: c for c in cases("f2_inv")}["zero"].want == [0] * 20
    assert len(BYTE_INTS) == 41 and all(sum(1 for b in w.to_bytes(32, "big") if b) == 1 for _, w in BYTE_INTS[9:])
    assert sorted(w.to_bytes(32, "big").index(max(w.to_bytes(32, "big"))) for _, w in BYTE_INTS[9:]) == list(range(32))
    assert {(w, k) for _, w in BYTE_INTS for k in range(4)} <= {c.args for c in cases("fp_from_be")}
    assert {w for _, w in BYTE_INTS} <= {c.args[0] for c in cases("fp_to_mont")}
    for op in ("fp_to_be", "fp_from_mont"):
        assert {w for _, w in BYTE_INTS if w < P} <= {c.args[0] * RINV % P for c in cases(op)}, op
    for _, a in _ones_below_p():
        assert a < P and all(x in (0, MASK, PTOP - 1) for x in limbs(a))
    assert PTOP << 234 <= KEPT_S < P


def test_curve_classes_are_present_and_of_their_kind():
    for op in PAIR_OPS:
        g = GROUPS[op[:2]]
        for name, cs in curve_classes(op).items():
            assert cs, (op, name)
            for c in cs:
                a, b = c.args
                fa, fb = O.jac_affine(g.F, a), O.jac_affine(g.F, b)
                if c.kind == "doubling":
                    assert name.startswith("P+P") or name == "order13 6T+6T"
                    assert fa == fb is not None and c.expect == O.jac_affine(g.F, O.jac_double(g.F, a)) is not None
                elif c.kind == "infinity":
                    assert name.startswith("P+(-P)") or name.startswith("order13")
                    assert fa is not None and fb is not None and fa != fb and c.expect is None
                elif c.kind == "generic":
                    assert fa is not None and fb is not None and fa[0] != fb[0] and c.expect is not None
                else:
                    want = {"left_inf": (True, False), "right_inf": (False, True), "both_inf": (True, True)}[c.kind]
                    assert (fa is None, fb is None) == want
                    assert c.expect == (fb if fa is None else fa)
                if "equal Z" in name and not op.endswith("_add"):
                    assert a[2] == g.F.one
                elif "equal Z" in name:
                    assert a[2] == b[2]
                if "different Z" in name:
                    assert a[2] != b[2] and (fa == fb or fa == g.neg(fb))
        kinds = {c.kind for c in cases(op)}
        assert {"generic", "doubling", "infinity", "left_inf"} <= kinds
    for op in ("g1_double", "g2_double"):
        g = GROUPS[op[:2]]
        cs = cases(op)
        same = [c for c in cs if c.label.startswith("P Z=")]
        assert len(same) == 3 and len({c.args[0][2] for c in same}) == 3 and len({c.expect for c in same}) == 1
        assert sum(c.kind == "infinity" for c in cs) == 2 and any(c.label.startswith("Q generic") for c in cs)
        assert all((c.expect is None) == (c.kind == "infinity") for c in cs)
    for op in ("g1_on_curve", "g2_on_curve"):
        by = {c.label: c.want[0] for c in cases(op)}
        assert by["P"] == by["Q"] == by["generator"] == 1
        assert by["P x+1"] == by["P y+1"] == by["P x-1"] == by["P y-1"] == by["(0,0)"] == 0
        assert {"(0,y)", "(x,0)"} <= set(by)
    assert O.g2_mul(_t13(), 13) is None and O.g2_on_curve(*_t13())


def test_the_comparison_accepts_the_oracle_and_refuses_changes():
    for op in OPS:
        for c in cases(op):
            out = model_output(op, c)
            assert mismatch(op, c, out) is None, (op, c.label)
    for op in POINT_OPS:
        g = GROUPS[op[:2]]
        nz = OPS[op][2] // 3
        finite = next(c for c in cases(op) if c.expect is not None)
        inf = next(c for c in cases(op) if c.expect is None)
        good = model_output(op, finite)
        bad = list(good)
        bad[0] ^= 1                                   # another X
        assert "X/Z^2" in mismatch(op, finite, bad)
        bad = list(good)
        bad[2 * nz:] = [0] * nz                       # infinity for a finite sum
        assert "infinity" in mismatch(op, finite, bad)
        assert "finite" in mismatch(op, inf, good)    # a finite point for infinity
        bad = list(good)
        bad[0:10] = limbs(val(good[0:10]) + P)        # the same residue, not reduced
        assert "not canonical" in mismatch(op, finite, bad)
        # another Jacobian form of the same point passes: (X l^2, Y l^3, Z l)
        x, y, z = g.coords([val(good[10 * e:10 * e + 10]) * RINV % P for e in range(len(good) // 10)])
        lam = g.elem(7)
        l2 = g.F.sqr(lam)
        other = (g.F.mul(x, l2), g.F.mul(y, g.F.mul(l2, lam)), g.F.mul(z, lam))
        assert mismatch(op, finite, g.words(other)) is None
    c = cases("fp_mul")[5]
    bad = list(c.want)
    bad[3] ^= 4
    assert mismatch("fp_mul", c, bad).startswith("word 3: GPU 0x")
