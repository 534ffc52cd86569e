"""Two-phase compilation (bn256_xprog.h): a source round becomes an XRound, a
pre-pass of shared linear combinations, then products and linear terms, with
the bounds the executor's arithmetic relies on checked at build time.

Operand space of a compiled round: 0..127 F, 128..143 slot A, 144..159 slot B,
160.. scratch."""

import copy
import random

from .field import (LAZY_LIMB, NEG_MULT, NONE, NREGS, ONE_CHAIN_QMAX_LIMIT, P, P2N, P_LIMB_TOP, R_BITS, REG, SLOT_A,
                    SLOT_B, comp)
from .limbs import to_limbs, xround_limbs
from .programs import KARATSUBA_MIN, LINE2_REGS, PROGRAM_TABLE, SCRATCH_CAP, load_oracle, round_jobs

X_SLOT_B = 144
X_SCR = 160


def _xsrc(r):
    """old register code -> new operand code"""
    if r >= SLOT_B:
        return X_SLOT_B + (r - SLOT_B)
    return r


class XRound:
    """A compiled round. Each lane runs one job (prod, lin -> dst) or, in a
    fused round, a second independent job (prod2, lin2 -> dst2) after the
    first: two programs' rounds share one pre-pass, table fetch and sync."""
    def __init__(self, nv, nt, np_, nl, lanes, name, np2=0, nl2=0):
        self.nv, self.nt, self.np, self.nl, self.lanes, self.name = nv, nt, np_, nl, lanes, name
        self.np2, self.nl2 = np2, nl2
        self.ks1 = self.ks2 = 0  # Karatsuba products per job (set by check_xround)
        self.ef = 0  # the first product's operands are plain elements (compile_round)
        # the linear-term job's REDC result is below (qmax + 1) p (check_xround);
        # one_chain: reduced by bn256_redq.h's one-chain tail, which takes qmax as
        # a template argument (Program.one_chain); lz: result left in [0, 2p)
        self.qmax, self.one_chain, self.lz = 0, False, 0

        def negk(terms):
            return sum(-k for _, k in terms if k < 0)
        self.kp = max([negk(t) for L in lanes for d, t in L["pre"] if d != NONE] or [0])
        self.kl1 = max([negk(L["lin"]) for L in lanes] or [0])
        self.kl2 = max([negk(L.get("lin2", [])) for L in lanes] or [0])

    def with_lanes(self, lanes):
        """This round, every attribute as it is, on other lanes (bind's translated ones)."""
        out = copy.copy(self)
        out.lanes = lanes
        return out

    @property
    def fused(self):
        return self.np2 > 0 or self.nl2 > 0

    def words(self):
        nhalves = self.nv * (1 + self.nt) + 2 * self.np + self.nl + 1
        if self.fused:
            nhalves += 2 * self.np2 + self.nl2 + 1
        return (nhalves + 1) // 2

    def lane_halves(self, t):
        """16-bit entries for bound rounds (bn256_xprog.h): operands/destinations
        as byte offsets (0xffff none), terms as element << 8 | int8 coef."""
        L = self.lanes[t]
        h = []
        off = lambda e: 0xFFFF if e == NONE else 40 * e  # noqa: E731
        for dst, terms in L["pre"]:
            h.append(off(dst))
            for src, c in terms:
                assert -128 <= c <= 127
                h.append((src << 8) | (c & 255))
        for u, v in L["prod"]:
            h += [off(u), off(v)]
        for src, c in L["lin"]:
            h.append((src << 8) | (c & 255))
        h.append(off(L["dst"]))
        if self.fused:
            for u, v in L["prod2"]:
                h += [off(u), off(v)]
            for src, c in L["lin2"]:
                h.append((src << 8) | (c & 255))
            h.append(off(L["dst2"]))
        h += [0] * (2 * self.words() - len(h))
        return h


def compile_round(lanes, name, scratch_cap, lanes2=None, pre_lanes=16, ks_min=None, one_chain=False, lazy=False):
    """pre_lanes, ks_min, one_chain, lazy: the fields of the round's Program
    record (programs.py); lanes2: the second job's source lanes in a fused round."""
    one_lc = [(REG["ONE"], 1)]
    values = {}      # canonical lincomb -> scratch code
    order = []

    def operand(lc):
        lc = [(r, k) for r, k in lc if k != 0] or [(REG["ZERO"], 1)]
        if len(lc) == 1 and lc[0][1] == 1:
            return _xsrc(lc[0][0])
        key = tuple(sorted((_xsrc(r), k) for r, k in lc))
        if key not in values:
            values[key] = X_SCR + len(order)
            order.append(key)
        return values[key]

    def jobs(ls):
        per = []
        for l in ls:
            prods, lins = [], []
            for a, b in l.slots:
                if list(b) == one_lc:
                    lins += [(_xsrc(r), k) for r, k in a if k != 0]
                elif list(a) == one_lc:
                    lins += [(_xsrc(r), k) for r, k in b if k != 0]
                else:
                    prods.append((operand(a), operand(b)))
            per.append((l.dst, prods, lins))
        assert len(per) <= 16, name
        return per

    per_lane = jobs(lanes)
    per_lane2 = jobs(lanes2) if lanes2 is not None else []
    # early first product (x_round's EF): when every lane has a product whose
    # operands are both plain elements (no pre-pass value), it goes first and
    # its operands are read together with the pre-pass's inputs, so the
    # products start without waiting for a second LDS round trip
    ef = int(lanes2 is None and any(p for _, p, _ in per_lane)
             and all(any(u < X_SCR and v < X_SCR for u, v in p) for _, p, _ in per_lane if p))
    if ef:
        for i, (d, p, q) in enumerate(per_lane):
            if p:
                k = next(j for j, (u, v) in enumerate(p) if u < X_SCR and v < X_SCR)
                per_lane[i] = (d, [p[k]] + p[:k] + p[k + 1:], q)
    if lanes2 is not None:
        # the first job's destinations are written after the second job reads: no overlap
        d1 = {d for d, _, _ in per_lane}
        for _, p2, l2 in per_lane2:
            assert not ({u for u, v in p2} | {v for u, v in p2} | {s for s, _ in l2}) & d1, name
    nvals = len(order)
    assert nvals <= scratch_cap, f"{name}: {nvals} pre-pass values > scratch {scratch_cap}"
    nv = (nvals + pre_lanes - 1) // pre_lanes
    nt = max([len(k) for k in order] or [0])
    np_ = max(len(p) for _, p, _ in per_lane)
    nl = max(len(q) for _, _, q in per_lane)
    np2 = max([len(p) for _, p, _ in per_lane2] or [0])
    nl2 = max([len(q) for _, _, q in per_lane2] or [0])
    if lanes2 is not None and np2 == 0 and nl2 == 0:
        nl2 = 1  # keep the fused layout
    zero = REG["ZERO"]
    out = []
    for t in range(16):
        pre = []
        for v in range(nv):
            vi = t + pre_lanes * v
            if t < pre_lanes and vi < nvals:
                terms = list(order[vi]) + [(zero, 0)] * (nt - len(order[vi]))
                pre.append((X_SCR + vi, terms))
            else:
                pre.append((NONE, [(zero, 0)] * nt))
        dst, prods, lins = per_lane[t] if t < len(per_lane) else (NONE, [], [])
        prods = prods + [(zero, zero)] * (np_ - len(prods))
        lins = lins + [(zero, 0)] * (nl - len(lins))
        L = {"pre": pre, "prod": prods, "lin": lins, "dst": dst}
        if lanes2 is not None:
            dst2, prods2, lins2 = per_lane2[t] if t < len(per_lane2) else (NONE, [], [])
            L["prod2"] = prods2 + [(zero, zero)] * (np2 - len(prods2))
            L["lin2"] = lins2 + [(zero, 0)] * (nl2 - len(lins2))
            L["dst2"] = dst2
        out.append(L)
    xr = XRound(nv, nt, np_, nl, out, name, np2, nl2)
    xr.ef = ef
    xr.one_chain = bool(one_chain and nl > 0)
    xr.lz = int(lazy and nl > 0)
    try:
        check_xround(xr, order, ks_min)
    except AssertionError:
        # the round-uniform correction overflows a bound: per-lane corrections
        xr.kp = xr.kl1 = xr.kl2 = -1
        check_xround(xr, order, ks_min)
    return xr


def check_xround(xr, order, ks_min=None):
    """Limb sums < 2^32, 64-bit columns < 2^64, REDC input < 800 p^2.
    ks_min: the program's Karatsuba threshold (default KARATSUBA_MIN)."""
    if ks_min is None:
        ks_min = KARATSUBA_MIN
    def src_bound(code):
        if code >= X_SCR:
            return vbound[code]
        return (2 * P, LAZY_LIMB)  # any element may be lazy (< 2p)

    # Every value of the pre-pass (and every lane's linear terms of a job) adds the
    # round-uniform correction K (2p)'' with K = the largest sum of negative
    # coefficients (xr.kp / kl1 / kl2): a compile-time constant in the executor.
    vbound = {}
    for i, key in enumerate(order):
        kp = xr.kp if xr.kp >= 0 else sum(-k for _, k in key if k < 0)  # -1: per-lane correction
        val, limbs = kp * NEG_MULT * P, [kp * x for x in P2N]
        for src, k in key:
            if k > 0:
                v, lb = src_bound(src)
                val += k * v
                limbs = [a + k * b for a, b in zip(limbs, lb)]
        assert max(limbs) < 1 << 32, f"{xr.name}: pre-pass limb overflow {key}"
        vbound[X_SCR + i] = (val, limbs)
    jobs = [(L["prod"], L["lin"], xr.kl1, xr.nl) for L in xr.lanes]
    if xr.fused:
        jobs += [(L["prod2"], L["lin2"], xr.kl2, xr.nl2) for L in xr.lanes]
    # Karatsuba per job (bn256_xprog.h x_products_ks): worth it from the
    # program's threshold on, valid while the 5-limb half sums stay 32-bit
    def ks_ok(prods):
        return len(prods) >= ks_min and all(
            max(lb[i] + lb[i + 5] for i in range(5)) < 1 << 32
            for u, v in prods for lb in (src_bound(u)[1], src_bound(v)[1]))
    xr.ks1 = int(all(ks_ok(L["prod"]) for L in xr.lanes))
    xr.ks2 = int(xr.fused and all(ks_ok(L["prod2"]) for L in xr.lanes))
    qmax1 = 0
    assert not (xr.one_chain and xr.fused), f"{xr.name}: a one-chain round is not fused"
    for prod, lin, kl, nl in jobs:
        L = {"prod": prod, "lin": lin}
        if kl < 0:
            kl = sum(-k for _, k in lin if k < 0)
        T, cols = 0, [0] * 21
        for u, v in L["prod"]:
            (bu, lu), (bv, lv) = src_bound(u), src_bound(v)
            T += bu * bv
            for i in range(10):
                for j in range(10):
                    cols[i + j] += lu[i] * lv[j]
        if nl > 0:
            T += kl * NEG_MULT * P * (1 << R_BITS)
            for i in range(10):
                cols[R_BITS // 26 + i] += kl * P2N[i]
        for src, k in L["lin"]:
            if k <= 0:
                continue
            b, lb = src_bound(src)
            T += k * b * (1 << R_BITS)
            for i in range(10):
                cols[R_BITS // 26 + i] += k * lb[i]
        # REDC adds up to 10 digit products (< 2^52 each) and a carry to every column
        assert max(cols) + 11 * (1 << 52) < 1 << 64, f"{xr.name}: column overflow"
        # REDC(T) < T/R + p with R = 2^286. Product-only rounds: T < p R gives a result
        # < 2p (acc_reduce, one conditional subtraction). Rounds with linear terms
        # (passed through REDC unchanged): result < T/R + p must stay below 31p, the
        # exact range of fp_reduce8 (q <= 30 keeps q * p_l inside int32).
        if nl > 0:
            assert T / (1 << R_BITS) + P < 30 * P, f"{xr.name}: REDC result {T / (1 << R_BITS) / P:.1f} p"
            # this job's own bound: V < T/R + p <= (q + 1) p
            q = ((T >> R_BITS) + 1 + P) // P
            qmax1 = max(qmax1, q)
            if xr.one_chain:
                check_one_chain(xr.name, q, max(cols[R_BITS // 26:]) + 11 * (1 << 52))
        else:
            assert T < P * (1 << R_BITS), f"{xr.name}: REDC input {T / P / P:.1f} p^2"
    xr.qmax = qmax1


def check_one_chain(name, qmax, cmax):
    """Fails the build unless redq_tail<qmax> is exact for a job whose REDC
    result is below (qmax + 1) p and whose columns 11..20 stay below cmax after
    the REDC digits (bn256_redq.h has the derivation)."""
    assert 1 <= qmax <= ONE_CHAIN_QMAX_LIMIT, f"{name}: quotient bound {qmax}"
    d = P_LIMB_TOP + 1
    # the chain's 64-bit sums: column + q (Z_j - p_j) + carry
    assert cmax + qmax * (1 << 26) + (1 << 39) < 1 << 64, f"{name}: one-chain column overflow"
    # the top limb and t in 32-bit arithmetic
    assert (qmax + 2) * d + (1 << 14) < 1 << 32, f"{name}: one-chain top limb"
    # 0 <= V - q p < (p9 + 1 + D + q) 2^234 with D = ceil(2 cmax / 2^52): below 2p
    D = (2 * cmax + (1 << 52) - 1) >> 52
    assert (P_LIMB_TOP + 1 + D + qmax) << 234 < 2 * P, f"{name}: one-chain result not below 2p"


def run_xround(xr, F, A, B, limbs=False):
    """Interprets a compiled round on plain residues; returns {dst: value}.
    limbs: F, A, B hold limb vectors of Montgomery representatives and the
    round runs limb for limb (xround_limbs), reduction tail included."""
    S = {}

    def get(code):
        if code >= X_SCR:
            return S[code]
        if code >= X_SLOT_B:
            return B[code - X_SLOT_B]
        if code >= SLOT_A:
            return A[code - SLOT_A]
        return F[code]

    if limbs:
        return xround_limbs(xr, get)[1]
    for L in xr.lanes:
        for dst, terms in L["pre"]:
            if dst != NONE:
                S[dst] = sum(k * get(src) for src, k in terms) % P
    out = {}
    for L in xr.lanes:
        for pk, lk, dk in (("prod", "lin", "dst"), ("prod2", "lin2", "dst2")):
            if dk not in L or L[dk] == NONE:
                continue
            acc = sum(get(u) * get(v) for u, v in L[pk]) + sum(k * get(src) for src, k in L[lk])
            assert L[dk] not in out, "two jobs write one destination"
            out[L[dk]] = acc % P
    return out


def compile_all():
    """name -> compiled rounds of every program of the table, in its order."""
    return {p.name: [compile_round(lanes, f"{p.name}[{i}]", SCRATCH_CAP[p.ctx], lanes2, pre_lanes=p.pre_lanes,
                                   ks_min=p.ks_min, one_chain=p.one_chain, lazy=p.lazy)
                     for i, (lanes, lanes2) in enumerate(round_jobs(p))]
            for p in PROGRAM_TABLE}


def run_xprogram(rounds, F, A=None, B=None, limbs=False):
    """F: register dict (mutated), A/B: slot element lists; returns the D slot (dict e -> v).
    limbs: see run_xround."""
    A = A or [to_limbs(0) if limbs else 0] * 12
    B = B or [to_limbs(0) if limbs else 0] * 12
    D = {}
    for xr in rounds:
        out = run_xround(xr, F, A, B, limbs)
        for dst, v in out.items():
            if dst < 128:
                F[dst] = v
            else:
                D[dst - 128] = v
    return D


def validate_x(seed=2):
    """The compiled programs against the oracle: the projective G2 steps and
    their lines against x/crypto's lineFunctionDouble / lineFunctionAdd, the
    Fp12 products and squarings against the tower arithmetic."""
    O = load_oracle()
    X = compile_all()
    rng = random.Random(seed)
    for trial in range(3):
        Q = O.g2_mul(O.G2_GEN, rng.randrange(1, O.ORDER))
        Hp = O.g1_mul(O.G1_GEN, rng.randrange(1, O.ORDER))
        Rj = O.jac_mul(O.FP2_OPS, O.to_jac(O.FP2_OPS, Q), rng.randrange(2, 1000))
        r = (Rj[0], Rj[1], Rj[2], O.f2_sqr(Rj[2]))
        F = {i: rng.randrange(P) for i in range(NREGS)}
        F[REG["ZERO"]] = 0
        F[REG["ONE"]] = 1
        F[REG["PX"]], F[REG["PY"]] = Hp

        def put(G, n, v):
            G[comp(n, "x")], G[comp(n, "y")] = v

        def getf(G, n):
            return (G[comp(n, "x")], G[comp(n, "y")])

        put(F, "QX", Q[0])
        put(F, "QY", Q[1])
        put(F, "NQY", O.f2_neg(Q[1]))
        # projective steps: R as (x Z : y Z : Z) with Z = xi W for a random W
        xi = (1, 3)
        aff = lambda j: (O.f2_mul(j[0], O.f2_inv(O.f2_sqr(j[2]))),  # noqa: E731
                         O.f2_mul(j[1], O.f2_inv(O.f2_mul(O.f2_sqr(j[2]), j[2]))))
        rx, ry = aff(Rj)
        Wr = (rng.randrange(1, P), rng.randrange(P))
        Zr = O.f2_mul(xi, Wr)
        put(F, "X", O.f2_mul(rx, Zr))
        put(F, "Y", O.f2_mul(ry, Zr))
        put(F, "Z", Wr)
        put(F, "P1X", O.f2_mul(Q[0], (rng.randrange(P), rng.randrange(P))))  # any affine point works
        put(F, "P1Y", (rng.randrange(P), rng.randrange(P)))

        def check_proj(G, want_r, want_line, name):
            zi = O.f2_inv(O.f2_mul(xi, getf(G, "Z")))
            got = (O.f2_mul(getf(G, "X"), zi), O.f2_mul(getf(G, "Y"), zi))
            assert got == aff(want_r), name + " point"
            la, lb, lc = (getf(G, n) for n in ("LA", "LB", "LC"))
            a, b, c = want_line
            mu = O.f2_mul(la, O.f2_inv(a))   # the lines agree up to an Fp2 factor
            assert mu != (0, 0) and (la, lb, lc) == tuple(O.f2_mul(mu, v) for v in (a, b, c)), name + " line"

        a, b, c, r_new = O._line_double(r, *Hp)
        G = dict(F)
        run_xprogram(X["PDBL"], G)
        check_proj(G, r_new, (a, b, c), "xPDBL")
        # fused Miller-loop programs: f^2 and the G2Base line beside the G2 step rounds
        f0 = [(rng.randrange(P), rng.randrange(P)) for _ in range(6)]
        flat0 = [z for pair in f0 for z in pair]
        # a normalised G2Base line (a = 1, k_g2_lines): c + b w + w^3
        fl_bx, fl_cy = (rng.randrange(P), rng.randrange(P)), (rng.randrange(P), rng.randrange(P))
        F[REG["SX"]], F[REG["NSY"]] = rng.randrange(P), rng.randrange(P)
        put(F, "FBX", fl_bx)
        put(F, "FCY", fl_cy)
        fix = (O.F2_ONE, O.f2_mul(fl_bx, (0, F[REG["SX"]])), O.f2_mul(fl_cy, (0, F[REG["NSY"]])))
        unfl = lambda D: [(D[2 * k], D[2 * k + 1]) for k in range(6)]  # noqa: E731
        G = dict(F)
        sq = run_xprogram(X["MDBL_1"], G, flat0)
        assert unfl(sq) == O.f12_sqr(f0), "xMDBL_1 square"
        d2 = run_xprogram(X["MDBL_2"], G, [sq[e] for e in range(12)])
        assert unfl(d2) == O._mul_line(O.f12_sqr(f0), *fix), "xMDBL_2 fixed line"
        check_proj(G, r_new, (a, b, c), "xMDBL")
        G = dict(F)
        run_xprogram(X["PDBL_1"], G)
        d2 = run_xprogram(X["MDBL_2"], G, flat0)
        assert unfl(d2) == O._mul_line(f0, *fix), "xPDBL_1/MDBL_2 fixed line"
        check_proj(G, r_new, (a, b, c), "xPDBL_1")
        for prog, pq in (("PADD_POS", (Q[0], Q[1])), ("PADD_NEG", (Q[0], O.f2_neg(Q[1]))),
                         ("PADD_F1", (getf(F, "P1X"), getf(F, "P1Y")))):
            a, b, c, r_new = O._line_add(r, pq, *Hp, O.f2_sqr(pq[1]))
            G = dict(F)
            run_xprogram(X[prog], G)
            check_proj(G, r_new, (a, b, c), "x" + prog)
            v = prog[5:]
            G = dict(F)
            run_xprogram(X[f"PADD_{v}_1"], G)
            d2 = run_xprogram(X[f"MADD_{v}_2"], G, flat0)
            run_xprogram(X[f"PADD_{v}_3"], G)
            assert unfl(d2) == O._mul_line(f0, *fix), "xMADD fixed line"
            check_proj(G, r_new, (a, b, c), "x" + prog + " split")
        # sig-only Miller rounds: f^2 / f * line with the next line's evaluation beside
        G = dict(F)
        sq = run_xprogram(X["SDBL"], G, flat0)
        assert unfl(sq) == O.f12_sqr(f0), "xSDBL square"
        assert (getf(G, "FB"), getf(G, "FC")) == fix[1:], "xSDBL line evaluation"
        G = dict(F)
        put(G, "FB", fix[1])
        put(G, "FC", fix[2])
        nbx, ncy = (rng.randrange(P), rng.randrange(P)), (rng.randrange(P), rng.randrange(P))
        put(G, "FBX", nbx)
        put(G, "FCY", ncy)
        d2 = run_xprogram(X["LFEV"], G, flat0)
        assert unfl(d2) == O._mul_line(f0, *fix), "xLFEV line"
        assert (getf(G, "FB"), getf(G, "FC")) == (O.f2_mul(nbx, (0, F[REG["SX"]])),
                                                  O.f2_mul(ncy, (0, F[REG["NSY"]]))), "xLFEV evaluation"
        G = dict(F)
        run_xprogram(X["FEVAL"], G)
        assert (getf(G, "FB"), getf(G, "FC")) == fix[1:], "xFEVAL"
        f = [(rng.randrange(P), rng.randrange(P)) for _ in range(6)]
        g = [(rng.randrange(P), rng.randrange(P)) for _ in range(6)]
        flat = lambda v: [z for pair in v for z in pair]  # noqa: E731
        unflat = lambda D: [(D[2 * k], D[2 * k + 1]) for k in range(6)]  # noqa: E731
        cyc = O.f12_mul(O.f12_conj(f), O.f12_inv(f))
        cyc = O.f12_mul(cyc, O.f12_frob2(cyc))
        assert unflat(run_xprogram(X["SQR12"], dict(F), flat(f))) == O.f12_sqr(f), "xSQR12"
        assert unflat(run_xprogram(X["CYC_SQR"], dict(F), flat(cyc))) == O.f12_sqr(cyc), "xCYC_SQR"
        assert unflat(run_xprogram(X["CYC_SQR_X"], dict(F), flat(cyc))) == O.f12_sqr(cyc), "xCYC_SQR_X"
        assert unflat(run_xprogram(X["MUL12"], dict(F), flat(f), flat(g))) == O.f12_mul(f, g), "xMUL12"
        assert unflat(run_xprogram(X["MUL12F"], dict(F), flat(f), flat(g))) == O.f12_mul(f, g), "xMUL12F"
        # the fold's mixed product: X * (alpha + w), alpha in elements 0..5 of
        # slot B (the other six are never read)
        al = [(rng.randrange(P), rng.randrange(P)) for _ in range(3)]
        aw = [al[0], (0, 1), al[1], (0, 0), al[2], (0, 0)]
        junk = [rng.randrange(P) for _ in range(6)]
        assert unflat(run_xprogram(X["TORMULF"], dict(F), flat(f), flat(al) + junk)) == O.f12_mul(f, aw), "xTORMULF"
        # the 12-lane (pre-pass on lanes 0..11) forms of k_verify_sig12
        assert unflat(run_xprogram(X["SQR12_12"], dict(F), flat(f))) == O.f12_sqr(f), "xSQR12_12"
        assert unflat(run_xprogram(X["CYC_SQR_X_12"], dict(F), flat(cyc))) == O.f12_sqr(cyc), "xCYC_SQR_X_12"
        assert unflat(run_xprogram(X["MUL12_12"], dict(F), flat(f), flat(g))) == O.f12_mul(f, g), "xMUL12_12"
        for name in ("SQR12_12", "LINE_FIX_12", "MUL12_12", "CYC_SQR_X_12"):
            for xr in X[name]:  # no pre-pass value on lanes 12..15
                assert all(d == NONE for L in xr.lanes[12:] for d, _ in L["pre"]), name
        G = dict(F)
        la, lb, lc = [(rng.randrange(P), rng.randrange(P)) for _ in range(3)]
        put(G, "LA", la)
        put(G, "LB", lb)
        put(G, "LC", lc)
        assert unflat(run_xprogram(X["LINE_PK"], G, flat(f))) == O._mul_line(f, la, lb, lc), "xLINE_PK"
        put(G, "FB", lb)
        put(G, "FC", lc)
        assert unflat(run_xprogram(X["LINE_FIX"], G, flat(f))) == O._mul_line(f, O.F2_ONE, lb, lc), "xLINE_FIX"
        assert unflat(run_xprogram(X["LINE_FIX_12"], G, flat(f))) == O._mul_line(f, O.F2_ONE, lb, lc), \
            "xLINE_FIX_12"
        # the pair form: f * (l0 + l1 w + l2 w^2 + y w^3 + l4 w^4), pre-pass values on lanes 0..11
        l4 = [(rng.randrange(P), rng.randrange(P)) for _ in range(4)]
        for n, v in zip(LINE2_REGS, l4):
            put(G, n, v)
        pair = [l4[0], l4[1], l4[2], (0, G[REG["NSY"]]), l4[3], (0, 0)]
        assert unflat(run_xprogram(X["LINE2_FIX_12"], G, flat(f))) == O.f12_mul(f, pair), "xLINE2_FIX_12"
        (xr2,) = X["LINE2_FIX_12"]
        assert (xr2.nv, xr2.np, xr2.nl) == (2, 9, 0) and xr2.ks1, "LINE2_FIX_12"
        assert all(d == NONE for L in xr2.lanes[12:] for d, _ in L["pre"]), "LINE2_FIX_12"
    return X
