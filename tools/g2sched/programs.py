"""The source programs and THE PROGRAM TABLE: one Program record per team
program, in the order of enum XProg, with everything compile_all and the
emitters need to know about it."""

from __future__ import annotations

import os
import random
import sys
from dataclasses import dataclass, field
from types import MappingProxyType

from .field import (NREGS, P, REG, SLOT_A, SLOT_B, Lane, comp, fp2_comp, lin, mul, neg, one, prod_terms, scal, scale,
                    smul, sq, sq_terms, xi_lc, xi_terms)


# ------------------------------------------------------------------ source programs
def fixed_line_eval(sfx=""):
    # FB = FBX * SX, FC = FCY * NSY  (the G2Base line at -sig), line set sfx
    return smul("FB" + sfx, [("FBX" + sfx, 1)], "SX") + smul("FC" + sfx, [("FCY" + sfx, 1)], "NSY")


# ---- homogeneous projective G2 steps (the Miller loop's point R lives in X, Y, Z
# with the Z register holding W = Z/xi, so that b' Z^2 = (3/xi) xi^2 W^2 = 3 xi W^2
# needs no multiplication by the constant b'). Textbook formulas: Costello, Lange,
# Naehrig (PKC 2010) doubling / add-1998-cmo-2 mixed addition, with the lines of
# Aranha et al. (Eurocrypt 2011) for the D-type twist; each output is a lazy sum of
# products of the previous round's values, so a doubling takes 2 rounds and an
# addition 3 (x/crypto's Jacobian lineFunctionDouble/Add take 3 and 5). The lines
# differ from x/crypto's by Fp2 factors and the points are the same points in other
# coordinates; the final exponentiation removes Fp2 factors, so the pairing (and
# every verdict) is unchanged for points of the prime-order group. The same is
# checked for twist points outside it that x/crypto's Unmarshal accepts, the
# small orders 13, 7369 and 95797 included: an order-13 key gives the Miller
# value 0 here as in x/crypto, the others the reference's pairing
# (tests/test_small_order_keys.py drives the compiled programs through whole
# Miller loops, tests/test_gpu_small_order_keys.py the kernels).
PD = {"XY": "A", "B": "B", "U": "S", "YW": "C", "X2": "G"}            # doubling temporaries
PA = {"TH": "AB", "LAM": "S1", "D": "D", "C": "I", "K": "S2", "N": "H", "J": "J", "V": "AV", "YL": "L1"}


def _xi_lc(name):
    """component lincombs of xi * name: ((3x + y), (3y - x))."""
    x, y = comp(name, "x"), comp(name, "y")
    return [(x, 3), (y, 1)], [(y, 3), (x, -1)]


def prog_double_proj(sfx=""):
    """T = (X : Y : xi W) -> 2T (scaled by 4) and the tangent line at (PX, PY):
       XY, B = Y^2, U = 9 xi W^2 (= 3 b' Z^2), YW, X2 = X^2
       X' = 2 XY (B - 3U), Y' = (B + 3U)^2 - 12 U^2, W' = 8 B YW
       line c + b w + a w^3: c = -2 xi YW PY, b = 3 X2 PX, a = U - B"""
    wx, wy = comp("Z", "x"), comp("Z", "y")
    u = [Lane(comp(PD["U"], "x"), [([(wx, 6)], [(wy, 9)]), ([(wy, 9), (wx, 9)], [(wy, 1), (wx, -1)])]),
         Lane(comp(PD["U"], "y"), [([(wy, 9), (wx, 9)], [(wy, 3), (wx, -3)]), ([(wx, -18)], [(wy, 1)])])]
    r1 = (mul(PD["XY"], [("X", 1)], [("Y", 1)]) + sq(PD["B"], [("Y", 1)]) + u
          + mul(PD["YW"], [("Y", 1)], [("Z", 1)]) + sq(PD["X2"], [("X", 1)]) + fixed_line_eval(sfx))
    b, uu = PD["B"], PD["U"]
    y3 = [Lane(comp("Y", c), sq_terms([(b, 1), (uu, 3)], c) + sq_terms([(uu, 1)], c, k=-12)) for c in "xy"]
    cx, cy = _xi_lc(PD["YW"])
    lc = [Lane(comp("LC" + sfx, "x"), [(scale(cx, -2), scal("PY"))]),
          Lane(comp("LC" + sfx, "y"), [(scale(cy, -2), scal("PY"))])]
    r2 = (mul("X", [(PD["XY"], 2)], [(b, 1), (uu, -3)]) + y3 + mul("Z", [(b, 8)], [(PD["YW"], 1)])
          + lc + smul("LB" + sfx, [(PD["X2"], 3)], "PX") + lin("LA" + sfx, [(uu, 1), (b, -1)]))
    return [r1, r2]


def prog_add_proj(px, py, sfx=""):
    """T = (X : Y : xi W) -> T + (px, py) and the line through them at (PX, PY):
       TH = Y - py xi W, LAM = X - px xi W
       D = LAM^2, C = TH^2, K = W LAM, N = X LAM, J = TH LAM, V = W TH, YL = Y LAM
       X' = D D + xi K C - 2 N D, Y' = J (3N - D) - xi V C - YL D, W' = K D
       line: c = LAM PY, b = -TH PX, a = TH px - LAM py"""
    wxi = _xi_lc("Z")

    def diff(dst, base, pt):
        # dst = base - pt * xi W
        out = []
        ptx, pty = comp(pt, "x"), comp(pt, "y")
        for c in "xy":
            if c == "x":   # (pt xi W).x = pt.x (xi W).y + pt.y (xi W).x
                slots = [([(ptx, -1)], wxi[1]), ([(pty, -1)], wxi[0])]
            else:          # (pt xi W).y = pt.y (xi W).y - pt.x (xi W).x
                slots = [([(pty, -1)], wxi[1]), ([(ptx, 1)], wxi[0])]
            out.append(Lane(comp(dst, c), slots + [([(comp(base, c), 1)], one())]))
        return out

    th, lam = PA["TH"], PA["LAM"]
    r1 = diff(th, "Y", py) + diff(lam, "X", px) + fixed_line_eval(sfx)
    r2 = (sq(PA["D"], [(lam, 1)]) + sq(PA["C"], [(th, 1)]) + mul(PA["K"], [("Z", 1)], [(lam, 1)])
          + mul(PA["N"], [("X", 1)], [(lam, 1)]) + mul(PA["J"], [(th, 1)], [(lam, 1)])
          + mul(PA["V"], [("Z", 1)], [(th, 1)]) + mul(PA["YL"], [("Y", 1)], [(lam, 1)]))
    d, cc, k, n, j, v, yl = (PA[x] for x in ("D", "C", "K", "N", "J", "V", "YL"))
    kx, ky = _xi_lc(k)
    vx, vy = _xi_lc(v)
    ccx, ccy = [(comp(cc, "x"), 1)], [(comp(cc, "y"), 1)]

    def xi_times_c(ax, ay, c, sign=1):
        # component c of sign * (ax i + ay) * C
        if c == "x":
            return [(scale(ax, sign), ccy), (scale(ay, sign), ccx)]
        return [(scale(ay, sign), ccy), (scale(neg(ax), sign), ccx)]

    x3 = [Lane(comp("X", c), sq_terms([(d, 1)], c) + xi_times_c(kx, ky, c) + prod_terms([(n, -2)], [(d, 1)], c))
          for c in "xy"]
    y3 = [Lane(comp("Y", c), prod_terms([(j, 1)], [(n, 3), (d, -1)], c) + xi_times_c(vx, vy, c, -1)
               + prod_terms([(yl, -1)], [(d, 1)], c)) for c in "xy"]
    la = [Lane(comp("LA" + sfx, c), prod_terms([(th, 1)], [(px, 1)], c) + prod_terms([(lam, -1)], [(py, 1)], c))
          for c in "xy"]
    r3 = (x3 + y3 + mul("Z", [(k, 1)], [(d, 1)]) + smul("LC" + sfx, [(lam, 1)], "PY")
          + smul("LB" + sfx, [(th, -1)], "PX") + la)
    return [r1, r2, r3]


def prog_cyc_sqr():
    """Granger-Scott squaring of f = (c0 + c3 s) + (c1 + c4 s) w + (c2 + c5 s) w^2
    (s = w^3, s^2 = xi) in the cyclotomic subgroup:
        A^2 = (a^2 + xi b^2) + ((a + b)^2 - a^2 - b^2) s = (a^2 + xi b^2) + 2ab s
        c0' = 3 (A^2)_0 - 2 c0      c3' = 3 (A^2)_1 + 2 c3        (A = (c0, c3))
        c2' = 3 (B^2)_0 - 2 c2      c5' = 3 (B^2)_1 + 2 c5        (B = (c1, c4))
        c1' = 3 xi (C^2)_1 + 2 c1   c4' = 3 (C^2)_0 - 2 c4        (C = (c2, c5))"""
    lanes = []

    def a0(a, b, c):  # component c of 3 (a^2 + xi b^2)
        bx = sq_terms([(b, 1)], "x")
        by = sq_terms([(b, 1)], "y")
        return [(scale(x, 3), y) for x, y in sq_terms([(a, 1)], c) + xi_terms(bx, by, c)]

    def a1(a, b, c, k=3):  # component c of k * 2ab
        return prod_terms([(a, 2 * k)], [(b, 1)], c)

    for c in "xy":
        lanes.append(Lane(comp("D0", c), a0("A0", "A3", c) + [(fp2_comp([("A0", -2)], c), one())]))
        lanes.append(Lane(comp("D3", c), a1("A0", "A3", c) + [(fp2_comp([("A3", 2)], c), one())]))
        lanes.append(Lane(comp("D2", c), a0("A1", "A4", c) + [(fp2_comp([("A2", -2)], c), one())]))
        lanes.append(Lane(comp("D5", c), a1("A1", "A4", c) + [(fp2_comp([("A5", 2)], c), one())]))
        lanes.append(Lane(comp("D4", c), a0("A2", "A5", c) + [(fp2_comp([("A4", -2)], c), one())]))
        # 3 xi (C^2)_1 = xi * 6 c2 c5
        px = prod_terms([("A2", 6)], [("A5", 1)], "x")
        py = prod_terms([("A2", 6)], [("A5", 1)], "y")
        lanes.append(Lane(comp("D1", c), xi_terms(px, py, c) + [(fp2_comp([("A1", 2)], c), one())]))
    return [lanes]


def prog_cyc_sqr_x():
    """Granger-Scott squaring with at most 3 products per lane (the operand
    combinations are shared by the team's pre-pass): per group (a, b),
        3(a^2 + xi b^2).x = (6ax) ay + (18bx) by + 3(by + bx)(by - bx)
        3(a^2 + xi b^2).y = 3(ay + ax)(ay - ax) - (6bx) by + 9(by + bx)(by - bx)
        6ab = (6ax by + 6ay bx) i + (6ay by - 6ax bx)
        6 xi ab = (6(3ax + ay) by + 6(3ay - ax) bx) i + (6(3ay - ax) by - 6(3ax + ay) bx)
    plus -2c (squared lanes) or +2c (product lanes) as a linear term."""
    def e(name, c):
        return comp(name, c)

    lanes = []
    groups = {0: ("A0", "A3"), 1: ("A1", "A4"), 2: ("A2", "A5")}
    # output coefficient k -> (group, kind): sq = a^2 + xi b^2 part, ab = 2ab part, xi = 2 xi ab part
    kinds = {0: (0, "sq"), 3: (0, "ab"), 2: (1, "sq"), 5: (1, "ab"), 4: (2, "sq"), 1: (2, "xi")}
    for k in range(6):
        g, kind = kinds[k]
        a, b = groups[g]
        ax, ay, bx, by = e(a, "x"), e(a, "y"), e(b, "x"), e(b, "y")
        for c in "xy":
            if kind == "sq":
                if c == "x":
                    slots = [([(ax, 6)], [(ay, 1)]), ([(bx, 18)], [(by, 1)]),
                             ([(by, 3), (bx, 3)], [(by, 1), (bx, -1)])]
                else:
                    slots = [([(ay, 3), (ax, 3)], [(ay, 1), (ax, -1)]), ([(bx, -6)], [(by, 1)]),
                             ([(by, 9), (bx, 9)], [(by, 1), (bx, -1)])]
                lin = [(e(f"A{k}", c), -2)]
            elif kind == "ab":
                if c == "x":
                    slots = [([(ax, 6)], [(by, 1)]), ([(ay, 6)], [(bx, 1)])]
                else:
                    slots = [([(ay, 6)], [(by, 1)]), ([(ax, -6)], [(bx, 1)])]
                lin = [(e(f"A{k}", c), 2)]
            else:
                u = [(ax, 18), (ay, 6)]
                v = [(ay, 18), (ax, -6)]
                if c == "x":
                    slots = [(u, [(by, 1)]), (v, [(bx, 1)])]
                else:
                    slots = [(v, [(by, 1)]), (u, [(bx, -1)])]
                lin = [(e(f"A{k}", c), 2)]
            lanes.append(Lane(comp(f"D{k}", c), slots + [(lin, one())]))
    return [lanes]


def prog_cyc_sqr_x_shared():
    """CYC_SQR_X's forms rewritten so that the lanes share their operand
    combinations (r06, the 12-lane teams: 24 pre-pass values instead of 31,
    two per lane on lanes 0..11 instead of three). The b-part of a squared
    group's two lanes,
        3(a^2 + xi b^2).x  b-part:  3 by^2 + 18 bx by - 3 bx^2 = bx V1 + by V2
        3(a^2 + xi b^2).y  b-part:  9 by^2 -  6 bx by - 9 bx^2 = by V1 + (-bx) V2
    with V1 = 9 by - 3 bx, V2 = 9 bx + 3 by, uses three values (V1, V2, -bx)
    where CYC_SQR_X uses five (18 bx, 3(by + bx), by - bx, -6 bx,
    9(by + bx)). The product lanes take their sign from -bx as well,
        6ab.y = (6ay) by + (6ax)(-bx),
    and the xi lanes keep the factor 6 on the plain element,
        6 xi ab.x = (6ax) W1 + (6ay) W2       W1 = 3 by - bx
        6 xi ab.y = (6ay) W1 + (6ax)(-W2)     W2 = by + 3 bx,
    so no value carries a coefficient above 9 or a negation above 4: with the
    round's correction 4 (4p)'' every limb stays below 2^31, the 5-limb half
    sums below 2^32, and the round's 3-product jobs run as Karatsuba products
    (Program.ks_min). Still 24 values and at most three products per
    lane, plus -2c / +2c as a linear term."""
    def e(name, c):
        return comp(name, c)

    lanes = []
    groups = {0: ("A0", "A3"), 1: ("A1", "A4"), 2: ("A2", "A5")}
    kinds = {0: (0, "sq"), 3: (0, "ab"), 2: (1, "sq"), 5: (1, "ab"), 4: (2, "sq"), 1: (2, "xi")}
    for k in range(6):
        g, kind = kinds[k]
        a, b = groups[g]
        ax, ay, bx, by = e(a, "x"), e(a, "y"), e(b, "x"), e(b, "y")
        v1 = [(by, 9), (bx, -3)]
        v2 = [(bx, 9), (by, 3)]
        nbx = [(bx, -1)]
        for c in "xy":
            if kind == "sq":
                if c == "x":
                    slots = [([(ax, 6)], [(ay, 1)]), ([(bx, 1)], v1), ([(by, 1)], v2)]
                else:
                    slots = [([(ay, 3), (ax, 3)], [(ay, 1), (ax, -1)]), ([(by, 1)], v1), (nbx, v2)]
                lin = [(e(f"A{k}", c), -2)]
            elif kind == "ab":
                if c == "x":
                    slots = [([(ax, 6)], [(by, 1)]), ([(ay, 6)], [(bx, 1)])]
                else:
                    slots = [([(ay, 6)], [(by, 1)]), ([(ax, 6)], nbx)]
                lin = [(e(f"A{k}", c), 2)]
            else:
                w1 = [(by, 3), (bx, -1)]
                w2 = [(by, 1), (bx, 3)]
                if c == "x":
                    slots = [([(ax, 6)], w1), ([(ay, 6)], w2)]
                else:
                    slots = [([(ay, 6)], w1), ([(ax, 6)], neg(w2))]
                lin = [(e(f"A{k}", c), 2)]
            lanes.append(Lane(comp(f"D{k}", c), slots + [(lin, one())]))
    return [lanes]


def prog_sqr12():
    """f^2 in Fp2[w]/(w^6 - xi): c_k = sum_{i<=j, i+j = k mod 6} (2 - [i==j]) a_i a_j xi^[i+j>=6]."""
    def xi_prod(i, j, c, mult):
        # component c of mult * (xi a_i) * a_j, xi a = (3x + y) i + (3y - x)
        ux = [(comp(f"A{i}", "x"), 3 * mult), (comp(f"A{i}", "y"), mult)]
        uy = [(comp(f"A{i}", "y"), 3 * mult), (comp(f"A{i}", "x"), -mult)]
        vx, vy = [(comp(f"A{j}", "x"), 1)], [(comp(f"A{j}", "y"), 1)]
        if c == "x":
            return [(ux, vy), (uy, vx)]
        return [(uy, vy), (neg(ux), vx)]

    lanes = []
    for k in range(6):
        for c in "xy":
            slots = []
            for i in range(6):
                for j in range(i, 6):
                    if (i + j) % 6 != k:
                        continue
                    mult = 1 if i == j else 2
                    if i + j >= 6:
                        slots += xi_prod(i, j, c, mult)
                    elif i == j:
                        slots += sq_terms([(f"A{i}", 1)], c)
                    else:
                        slots += prod_terms([(f"A{i}", mult)], [(f"A{j}", 1)], c)
            lanes.append(Lane(comp(f"D{k}", c), slots))
    return [lanes]


def prog_mul12():
    """dst = A * B in Fp2[w]/(w^6 - xi): lane (k, c) sums over i the component c of
    A_i' B_j, j = k - i mod 6, A_i' = xi A_i when k - i < 0 (x/crypto gfP12.Mul)."""
    lanes = []
    for k in range(6):
        for c in "xy":
            slots = []
            for i in range(6):
                j = (k - i) % 6
                ax, ay = [(comp(f"A{i}", "x"), 1)], [(comp(f"A{i}", "y"), 1)]
                if k - i < 0:
                    ax, ay = xi_lc(ax, ay)
                bx, by = [(comp(f"B{j}", "x"), 1)], [(comp(f"B{j}", "y"), 1)]
                if c == "x":
                    slots += [(ax, by), (ay, bx)]
                else:
                    slots += [(ay, by), (neg(ax), bx)]
            lanes.append(Lane(comp(f"D{k}", c), slots))
    return [lanes]


def prog_line(la, lb, lc):
    """dst = A * (lc + lb w + la w^3) (sparse line, coefficients in F registers);
    xi is applied to the line coefficient of a wrapped term."""
    lanes = []
    for k in range(6):
        for c in "xy":
            slots = []
            for jpos, L in ((0, lc), (1, lb), (3, la)):
                i = k - jpos
                lx, ly = [(comp(L, "x"), 1)], [(comp(L, "y"), 1)]
                if i < 0:
                    i += 6
                    lx, ly = xi_lc(lx, ly)
                fx, fy = [(comp(f"A{i}", "x"), 1)], [(comp(f"A{i}", "y"), 1)]
                if c == "x":
                    slots += [(fx, ly), (fy, lx)]
                else:
                    slots += [(fy, ly), (fx, neg(lx))]
            lanes.append(Lane(comp(f"D{k}", c), slots))
    return [lanes]


def prog_line_n(lb, lc):
    """dst = A * (lc + lb w + w^3): a G2Base line divided by its constant
    coefficient a (bn256_kernels.hip k_g2_lines; the Fp2 factor a is removed by
    the final exponentiation), so the w^3 part is A * w^3, a linear term (a
    coefficient shift, xi on the wrapped ones): 4 products per lane instead of
    prog_line's 6."""
    lanes = []
    for k in range(6):
        for c in "xy":
            slots = []
            for jpos, L in ((0, lc), (1, lb)):
                i = k - jpos
                lx, ly = [(comp(L, "x"), 1)], [(comp(L, "y"), 1)]
                if i < 0:
                    i += 6
                    lx, ly = xi_lc(lx, ly)
                fx, fy = [(comp(f"A{i}", "x"), 1)], [(comp(f"A{i}", "y"), 1)]
                if c == "x":
                    slots += [(fx, ly), (fy, lx)]
                else:
                    slots += [(fy, ly), (fx, neg(lx))]
            i = k - 3
            fx, fy = [(comp(f"A{i % 6}", "x"), 1)], [(comp(f"A{i % 6}", "y"), 1)]
            if i < 0:
                fx, fy = xi_lc(fx, fy)   # xi * A_{k+3}
            slots.append((fx if c == "x" else fy, one()))
            lanes.append(Lane(comp(f"D{k}", c), slots))
    return [lanes]


def prog_line2_n(l0, l1, l2, l4, y):
    """dst = A * (l0 + l1 w + l2 w^2 + y w^3 + l4 w^4), y an Fp scalar
    register: the product of two consecutive normalised G2Base lines (a
    doubling's and its addition's, or the two Frobenius lines) divided by the
    constant Fp2 part K3 of its w^3 coefficient K3 y', a factor the final
    exponentiation removes like prog_line_n's a (bn256_kernels.hip k_g2_lines
    has the pair constants, bn256_sig12.hip k_sig_lines the coefficients). One
    round of 9 products per lane, no linear term, instead of prog_line_n's two
    rounds. (Dividing by y' as well would make the w^3 part a linear term, 8
    products; the inversion it needs costs the headline more than the product:
    DESIGN.md 3d.) xi sits on the line coefficient of a wrapped term and, for
    the w^3 part, on A (twelve pre-pass values), the y components' sign on the
    A side, -A_i.x (six more): eighteen values, at most two per lane of a
    12-lane team."""
    lanes = []
    for k in range(6):
        for c in "xy":
            slots = []
            for jpos, L in ((0, l0), (1, l1), (2, l2), (4, l4)):
                i = k - jpos
                lx, ly = [(comp(L, "x"), 1)], [(comp(L, "y"), 1)]
                if i < 0:
                    i += 6
                    lx, ly = xi_lc(lx, ly)
                fx, fy = [(comp(f"A{i}", "x"), 1)], [(comp(f"A{i}", "y"), 1)]
                if c == "x":
                    slots += [(fx, ly), (fy, lx)]
                else:
                    slots += [(fy, ly), (neg(fx), lx)]
            i = k - 3
            fx, fy = [(comp(f"A{i % 6}", "x"), 1)], [(comp(f"A{i % 6}", "y"), 1)]
            if i < 0:
                fx, fy = xi_lc(fx, fy)   # xi * A_{k+3}
            slots.append((fx if c == "x" else fy, scal(y)))
            lanes.append(Lane(comp(f"D{k}", c), slots))
    return [lanes]


def prog_tor_mul():
    """dst = A * (alpha + w) for A = n + d w (n = the even powers of w, d the odd
    ones: Fp6 = Fp2[v]/(v^3 - xi), v = w^2) and alpha in Fp6 in elements 0..5 of
    slot B (B0, B1, B2):
        n' = n alpha + v d,    d' = d alpha + n.
    A unitary g = a + b w equals (alpha + w)/(alpha - w) with alpha = (1 + a)/b,
    so a GT table entry kept as alpha multiplies a running X (value X/conj(X))
    with two Fp6 products: 6 Fp products per lane instead of MUL12's 12. xi and
    the sign of the i * i products are applied on the alpha side (9 pre-pass
    values shared by all lanes); v d and n are the round's linear terms."""
    lanes = []
    for k in range(6):
        m, odd = k // 2, k % 2
        for c in "xy":
            slots = []
            for i in range(3):
                j = (m - i) % 3
                src = f"A{2 * i + odd}"
                fx, fy = [(comp(src, "x"), 1)], [(comp(src, "y"), 1)]
                ax, ay = [(comp(f"B{j}", "x"), 1)], [(comp(f"B{j}", "y"), 1)]
                if m - i < 0:
                    ax, ay = xi_lc(ax, ay)   # xi * alpha_j
                if c == "x":
                    slots += [(fx, ay), (fy, ax)]
                else:
                    slots += [(fy, ay), (fx, neg(ax))]
            if odd:       # + n_m
                lx, ly = [(comp(f"A{2 * m}", "x"), 1)], [(comp(f"A{2 * m}", "y"), 1)]
            elif m > 0:   # + (v d)_m = d_{m-1}
                lx, ly = [(comp(f"A{2 * m - 1}", "x"), 1)], [(comp(f"A{2 * m - 1}", "y"), 1)]
            else:         # + (v d)_0 = xi d_2
                lx, ly = xi_lc([(comp("A5", "x"), 1)], [(comp("A5", "y"), 1)])
            slots.append((lx if c == "x" else ly, one()))
            lanes.append(Lane(comp(f"D{k}", c), slots))
    return [lanes]


# ------------------------------------------------------------------ the program table
# Scratch contexts: where a program's pre-pass values live, and how many fit.
# FE: the register file from register 2 on; ML: slots C..J during the Miller loop
# FOLD: the GT fold kernels' compact team region (bn256_gtfold.h): slots F, A, B,
# then registers ZERO and ONE, then the pre-pass scratch
SCRATCH_CAP = MappingProxyType({"FE": 48, "ML": 96, "FOLD": 48})
KARATSUBA_MIN = 4   # jobs of this many products use Karatsuba (when check_xround allows)


@dataclass(frozen=True)
class Program:
    """One team program: a member of enum XProg, compiled by compile_all.
    Adding a program is one record here and one line in an instance list
    (layouts.py); every field a kernel depends on is stated on the record."""
    name: str
    ctx: str                # scratch context: a key of SCRATCH_CAP
    # The source: rounds, each a list of Lanes; or, for a Miller-loop program
    # whose rounds run beside another program's (see XRound), fused: per round
    # the one or two (program, round) jobs it is made of.
    rounds: list | None = None
    fused: tuple | None = None
    # lanes that evaluate the pre-pass values: 16, or 12 for programs whose
    # pre-pass values live on lanes 0..11 only, so that they also run in
    # 12-lane teams (five per wave: k_gt_chunks, make_team12)
    pre_lanes: int = 16
    # Karatsuba threshold (None: KARATSUBA_MIN). The default counts
    # instructions: a Karatsuba product saves 25 mads for 10 limb additions,
    # and the job's column combination (~55 plain instructions) is repaid from
    # four products on.
    ks_min: int | None = None
    # the linear-term rounds are reduced by bn256_redq.h's one-chain tail
    # (check_one_chain), which takes the round's quotient bound as a template
    # argument
    one_chain: bool = False
    # the rounds with linear terms leave their result in [0, 2p) (x_round's
    # LZ: no final conditional subtraction). Every reader of their output must
    # be a team program, which takes elements below 2p: in t12_pow_v_x and
    # team_final_exp (bn256_xprog.h, bn256_pairing.h) each squaring feeds the
    # next squaring or a MUL12, whose result is canonical.
    lazy: bool = False
    # REDC fusion (x_round's FU, bn256_xprog.h x_job): the job's last product
    # runs as a 100-mad schoolbook product with the REDC digits interleaved,
    # which hides the reduction's serial chain where a SIMD has one wave:
    # k_verify_sig's 16-lane rounds (layout S) and the final exponentiation's.
    # Not the GT fold's (several waves per SIMD hide the chain), not two-job
    # rounds, not the pk-side G2 steps (measured: config 2 0.5 % slower with
    # them, profiles/r03fuse_redc_ab.json). The 12-lane programs of
    # k_sig12_miller and k_sig12_fe always share their SIMD with a second wave,
    # which hides the chain as well, so they keep the products-then-REDC order
    # and every product of theirs is a 75-mad Karatsuba product (measured, with
    # the cyclotomic squaring's third product fused and not:
    # profiles/r07ks_levers_ab.json). Stated on every record: no default.
    redc_fuse: bool = field(kw_only=True)


def _split_addition(v):
    """PADD_v's three rounds as programs of their own, the second beside f * the G2Base line."""
    return [Program(f"PADD_{v}_1", "ML", fused=((f"PADD_{v}", 0),), redc_fuse=False),
            Program(f"MADD_{v}_2", "ML", fused=((("LINE_FIX", 0), (f"PADD_{v}", 1)),), redc_fuse=False),
            Program(f"PADD_{v}_3", "ML", fused=((f"PADD_{v}", 2),), redc_fuse=False)]


# f times a PAIR of consecutive lines in one round (team_miller_sig12's nonzero
# digits and its two Frobenius lines): the coefficients L0, L1, L2, L4 in the
# eight consecutive registers FBX, FCY, FB, FC, and y' in NSY
LINE2_REGS = ("FBX", "FCY", "FB", "FC")

# The order is enum XProg's and the order of the _S / _T / _V variants.
PROGRAM_TABLE = (
    # the pk-side G2 steps and k_verify's Miller loop: no REDC fusion (Program.redc_fuse)
    Program("PDBL", "ML", prog_double_proj(), redc_fuse=False),
    Program("PADD_POS", "ML", prog_add_proj("QX", "QY"), redc_fuse=False),
    Program("PADD_NEG", "ML", prog_add_proj("QX", "NQY"), redc_fuse=False),
    Program("PADD_F1", "ML", prog_add_proj("P1X", "P1Y"), redc_fuse=False),
    Program("PADD_F2", "ML", prog_add_proj("P2X", "QY"), redc_fuse=False),
    # Miller-loop programs whose rounds fuse two independent rounds (XRound):
    # f^2 beside the doubling's first round
    Program("MDBL_1", "ML", fused=((("SQR12", 0), ("PDBL", 0)),), redc_fuse=False),
    # f * G2Base line beside its second round
    Program("MDBL_2", "ML", fused=((("LINE_FIX", 0), ("PDBL", 1)),), redc_fuse=False),
    # first iteration (f = 1: no squaring)
    Program("PDBL_1", "ML", fused=(("PDBL", 0),), redc_fuse=False),
    *_split_addition("POS"), *_split_addition("NEG"), *_split_addition("F1"), *_split_addition("F2"),
    Program("SQR12", "ML", prog_sqr12(), redc_fuse=False),
    Program("LINE_PK", "ML", prog_line("LA", "LB", "LC"), redc_fuse=False),
    # The G2Base lines are normalised (a = 1): prog_line_n. REDC fusion as one
    # of k_verify_sig's programs (see SDBL).
    Program("LINE_FIX", "ML", prog_line_n("FB", "FC"), redc_fuse=True),
    # the final exponentiation's (one wave per SIMD in k_verify_sig and k_verify: REDC fusion)
    Program("CYC_SQR", "FE", prog_cyc_sqr(), redc_fuse=True),
    Program("MUL12", "FE", prog_mul12(), redc_fuse=True),
    Program("CYC_SQR_X", "FE", prog_cyc_sqr_x(), lazy=True, redc_fuse=True),
    # Sig-only Miller loop (bn256_sigteam.h team_miller_sig, run by k_verify_sig,
    # one wave per SIMD: REDC fusion): the G2Base line at -sig is evaluated on lanes
    # 12..15 beside f^2 (SDBL) or beside f * the previous line (LFEV), rounds
    # whose Fp12 jobs leave those lanes idle anyway; FEVAL alone.
    Program("FEVAL", "ML", [fixed_line_eval()], redc_fuse=True),
    Program("SDBL", "ML", [prog_sqr12()[0] + fixed_line_eval()], redc_fuse=True),
    Program("LFEV", "ML", [prog_line_n("FB", "FC")[0] + fixed_line_eval()], redc_fuse=True),
    # Fp12 product in the compact GT-fold team layout (context FOLD); several
    # waves per SIMD: no REDC fusion
    Program("MUL12F", "FOLD", prog_mul12(), pre_lanes=12, redc_fuse=False),
    # k_verify_sig12 (bn256_sig12.hip): the sig-only pairing on FIVE 12-lane teams
    # per wave (make_team12). The G2Base lines arrive evaluated at -sig
    # (k_sig_lines), so the Miller loop is f^2 (SQR12) and f * line (LINE_FIX)
    # with nothing beside them on lanes 12..15, and every pre-pass value lives on
    # lanes 0..11. Two waves per SIMD: no REDC fusion (Program.redc_fuse).
    Program("SQR12_12", "ML", prog_sqr12(), pre_lanes=12, redc_fuse=False),
    Program("LINE_FIX_12", "ML", prog_line_n("FB", "FC"), pre_lanes=12, one_chain=True, redc_fuse=False),
    Program("MUL12_12", "FE", prog_mul12(), pre_lanes=12, redc_fuse=False),
    # r06: 24 pre-pass values (two per lane). Its 3-product jobs do not save
    # instructions with Karatsuba (SQ_INSTS_VALU of k_sig12_fe: 160.5 M ->
    # 159.4 M per 4096 checks, with lever A), but the kernel is shorter with
    # them beside a second wave on the SIMD: the threshold 3 rests on the
    # interleaved A/B alone (profiles/r07ks_levers_ab.json, r07ks_ab.json), not
    # on a cycle price of the two instruction classes, which nobody has
    # measured in these kernels.
    Program("CYC_SQR_X_12", "FE", prog_cyc_sqr_x_shared(), pre_lanes=12, ks_min=3, one_chain=True, lazy=True,
            redc_fuse=False),
    # k_tor_chunks (bn256_gt.hip): a running product times a table entry in torus
    # form, in the GT-fold team layout, 12-lane teams. The fold's mixed product,
    # six products per lane: as for MUL12F the instruction count decides
    # (Karatsuba from four products on), and several waves per SIMD: no REDC fusion.
    Program("TORMULF", "FOLD", prog_tor_mul(), pre_lanes=12, ks_min=4, redc_fuse=False),
    Program("LINE2_FIX_12", "ML", prog_line2_n(*LINE2_REGS, "NSY"), pre_lanes=12, redc_fuse=False),
)
PROGRAM = MappingProxyType({p.name: p for p in PROGRAM_TABLE})
assert len(PROGRAM) == len(PROGRAM_TABLE) and all(p.ctx in SCRATCH_CAP for p in PROGRAM_TABLE)
assert all((p.rounds is None) != (p.fused is None) for p in PROGRAM_TABLE)


def _view(pick, value):
    return MappingProxyType({p.name: value(p) for p in PROGRAM_TABLE if pick(p)})


# Read-only views of the table under the names the tests and DESIGN.md know.
PROGRAMS = _view(lambda p: p.rounds is not None, lambda p: p.rounds)   # name -> source rounds
X_PROGRAMS = _view(lambda p: True, lambda p: p.ctx)                     # name -> scratch context
PRE_LANES = _view(lambda p: p.pre_lanes != 16, lambda p: p.pre_lanes)
KARATSUBA_MIN_PROG = _view(lambda p: p.ks_min is not None, lambda p: p.ks_min)
REDC_FUSE = _view(lambda p: True, lambda p: p.redc_fuse)
ONE_CHAIN_PROGRAMS = tuple(p.name for p in PROGRAM_TABLE if p.one_chain)
LAZY_PROGRAMS = tuple(p.name for p in PROGRAM_TABLE if p.lazy)


def round_jobs(p):
    """A program's rounds as (lanes, lanes2): the source lanes of each round's
    first job and of its second (None in a one-job round)."""
    if p.fused is None:
        return [(r, None) for r in p.rounds]
    out = []
    for jobs in p.fused:
        lanes = [PROGRAM[n].rounds[r] for n, r in (jobs if isinstance(jobs[0], tuple) else (jobs,))]
        out.append((lanes[0], lanes[1] if len(lanes) > 1 else None))
    return out


# ------------------------------------------------------------------ source-program interpreter
def run_program(prog, F):
    """Interprets a program on an index -> residue map (plain values mod p)."""
    for lanes in prog:
        out = {}
        for l in lanes:
            acc = 0
            for a, b in l.slots:
                va = sum(k * F[r] for r, k in a)
                vb = sum(k * F[r] for r, k in b)
                acc += va * vb
            out[l.dst] = acc % P
        F.update(out)
    return F


def load_oracle():
    sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", ".."))
    from oracle import bn256_oracle
    return bn256_oracle


def validate(seed=1):
    """The source programs of the Fp12 squarings against the oracle, lane by lane."""
    O = load_oracle()
    rng = random.Random(seed)
    for trial in range(3):
        F = {i: rng.randrange(P) for i in list(range(NREGS)) + list(range(SLOT_A, SLOT_A + 12))
             + list(range(SLOT_B, SLOT_B + 12))}
        F[REG["ZERO"]] = 0
        F[REG["ONE"]] = 1
        # Fp12 squarings: a random element, and a cyclotomic one
        f = [(rng.randrange(P), rng.randrange(P)) for _ in range(6)]
        cyc = O.f12_mul(O.f12_conj(f), O.f12_inv(f))
        cyc = O.f12_mul(cyc, O.f12_frob2(cyc))
        for prog, val in (("SQR12", f), ("CYC_SQR", cyc)):
            G = dict(F)
            for k in range(6):
                G[comp(f"A{k}", "x")], G[comp(f"A{k}", "y")] = val[k]
            G = run_program(PROGRAMS[prog], G)
            got = [(G[comp(f"D{k}", "x")], G[comp(f"D{k}", "y")]) for k in range(6)]
            assert got == O.f12_sqr(val), prog
    return True
