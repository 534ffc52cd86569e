"""The limb-level interpreter: the executor's arithmetic word for word
(bn256_xprog.h x_round, bn256_fp.h, bn256_redq.h). Elements are Montgomery
representatives (x R mod p, or that plus p for a lazy element) held as ten
limbs, pre-pass values are 32-bit limb sums, a job is 21 64-bit columns, REDC
runs digit by digit, and the tail is the round's own form. Every intermediate
is asserted to fit its register."""

from .field import (NONE, ONE_CHAIN_COMPARE_Q, ONE_CHAIN_QMAX_LIMIT, P, P2N, P_LIMB_TOP, P_LIMBS, R_BITS, REDQ_Z)

R_MONT = 1 << R_BITS
P_INV26 = (-pow(P, -1, 1 << 26)) % (1 << 26)
MASK26 = (1 << 26) - 1
REDQ_D = P_LIMB_TOP + 1
REDQ_M = (1 << 53) // REDQ_D + 1


def to_limbs(v):
    """An integer below 2^266 as ten limbs (nine of 26 bits, the top one whole)."""
    return [(v >> (26 * j)) & MASK26 for j in range(9)] + [v >> 234]


def from_limbs(l):
    return sum(x << (26 * j) for j, x in enumerate(l))


def redq_tail_model(c, qmax, lazy):
    """redq_tail<qmax, lazy> on the columns 11..20 (ten 64-bit values)."""
    assert 1 <= qmax <= ONE_CHAIN_QMAX_LIMIT and all(0 <= x < 1 << 64 for x in c)
    t = ((c[9] & 0xFFFFFFFF) + ((c[8] >> 26) & 0xFFFFFFFF)) & 0xFFFFFFFF
    if qmax <= ONE_CHAIN_COMPARE_Q:
        q = sum(1 for k in range(1, qmax + 1) if t >= k * REDQ_D)
    else:
        assert t * REDQ_M < 1 << 64
        q = (t * REDQ_M) >> 53
    r, carry = [], 0
    for j in range(9):
        v = c[j] + q * (REDQ_Z[j] - P_LIMBS[j]) + carry
        assert v < 1 << 64, "one-chain column overflow"
        r.append(v & MASK26)
        carry = v >> 26
    r.append((((c[9] + carry) & 0xFFFFFFFF) - q * REDQ_D) & 0xFFFFFFFF)
    if not lazy and r[9] >= P_LIMBS[9]:
        s, br = [], 0
        for i in range(10):
            v = r[i] - P_LIMBS[i] - br
            br = 1 if v < 0 else 0
            s.append(v & MASK26)
        if br == 0:
            r = s
    return r


def reduce_wide_model(c, lazy):
    """acc_reduce_wide / acc_reduce_wide_lazy's tail (bn256_team.h) on columns 11..20."""
    x, carry = [], 0
    for j in range(10):
        v = (c[j] + carry) & ((1 << 64) - 1)
        x.append(v & MASK26 if j < 9 else v & 0xFFFFFFFF)
        carry = v >> 26
    q = x[9] // REDQ_D
    assert q <= 30
    y, cy = [], 0
    for i in range(10):
        v = x[i] - q * P_LIMBS[i] + cy
        assert -(1 << 31) <= v < 1 << 31
        y.append(v & MASK26 if i < 9 else v & 0xFFFFFFFF)
        cy = v >> 26
    return y if lazy else _csub_model(y, rare=False)


def _csub_model(x, rare):
    if rare and x[9] < P_LIMBS[9]:
        return list(x)
    s, br = [], 0
    for i in range(10):
        v = x[i] - P_LIMBS[i] - br
        br = 1 if v < 0 else 0
        s.append(v & MASK26)
    return list(x) if br else s


def _lincomb_model(terms, k, read):
    """x_lincomb_sum: 32-bit limb sums with the correction K (4p)''."""
    if k < 0:
        k = sum(-c for _, c in terms if c < 0)
    out = [k * z for z in P2N]
    for src, c in terms:
        x = read(src)
        out = [a + c * b for a, b in zip(out, x)]
    assert all(0 <= v < 1 << 32 for v in out), "limb sum outside 32 bits"
    return out


def xround_limbs(xr, read):
    """One round on limb vectors. read(code) -> the ten limbs of an operand
    that the pre-pass does not write. Returns (pre, out): the pre-pass values
    and the jobs' results, both {destination: limbs}."""
    pre = {}
    for L in xr.lanes:
        for dst, terms in L["pre"]:
            if dst != NONE:
                pre[dst] = _lincomb_model(terms, xr.kp, read)

    def rd(code):
        return pre[code] if code in pre else read(code)

    out = {}
    for L in xr.lanes:
        for pk, lk, dk, kl, second in (("prod", "lin", "dst", xr.kl1, False), ("prod2", "lin2", "dst2", xr.kl2, True)):
            if dk not in L or L[dk] == NONE:
                continue
            nl = xr.nl2 if second else xr.nl
            cols = [0] * 21
            if nl > 0:
                cols[11:21] = _lincomb_model(L[lk], kl, rd)
            for u, v in L[pk]:
                a, b = rd(u), rd(v)
                for i in range(10):
                    for j in range(10):
                        cols[i + j] += a[i] * b[j]
            for i in range(11):  # acc_redc_digit
                q = (cols[i] * P_INV26) & MASK26
                for j in range(10):
                    cols[i + j] += q * P_LIMBS[j]
                cols[i + 1] += cols[i] >> 26
            assert all(c < 1 << 64 for c in cols), "column overflow"
            if nl > 0 and xr.one_chain and not second:
                r = redq_tail_model(cols[11:], xr.qmax, bool(xr.lz))
            elif nl > 0:
                r = reduce_wide_model(cols[11:], bool(xr.lz) and not second)
            else:  # acc_reduce: acc_redc_limbs and fp_csub_rare
                x, carry = [], 0
                for j in range(10):
                    v = cols[11 + j] + carry
                    x.append(v & MASK26 if j < 9 else v & 0xFFFFFFFF)
                    carry = v >> 26
                r = _csub_model(x, rare=True)
            val = from_limbs(r)
            assert all(x <= MASK26 for x in r[:9]) and val < (2 * P if xr.lz else P), f"{xr.name}: result range"
            assert L[dk] not in out, "two jobs write one destination"
            out[L[dk]] = r
    return pre, out


def run_bound_limbs(rounds, mem):
    """run_bound limb for limb: mem holds limb vectors of Montgomery
    representatives (to_limbs(x R mod p), lazy ones plus p)."""
    for xr in rounds:
        pre, out = xround_limbs(xr, lambda code: mem[code])
        for d, v in list(pre.items()) + list(out.items()):
            mem[d] = v
