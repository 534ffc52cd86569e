"""The one-chain reduction tail of the linear-term rounds (handel_amd/csrc/
bn256_redq.h redq_tail<QMAX, LAZY>) on the CPU: tests/native/
reduce_wide_host.cpp compiles the header the device code includes, with
-fsanitize=address,undefined, and every result is compared with Python
integers — canonical forms return exactly V mod p, lazy forms a value in
[0, 2p) congruent to V with nine 26-bit low limbs — and, limb for limb, with
the generator's model of the same tail (tools/gen_g2_schedule.py
redq_tail_model), which is what its interpreter runs.

Cases per form: V = k p - 1, k p, k p + 1 for every k the form's bound admits
(V < (QMAX + 1) p), each as normalised columns, as columns pushed to the
largest magnitude check_one_chain admits and at a random spread; plus 10^5
random in-bound values per form at random spreads.
"""

import os
import random
import subprocess
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tools"))
import gen_g2_schedule as G  # noqa: E402

P = G.P
# compare forms (QMAX <= 2), division forms; 13 is what the generator emits
# today, 30 acc_reduce_wide's old range, 64 the forms' limit
QMAXES = (1, 2, 3, 13, 30, 64)
RANDOM_QMAXES = (2, 13, 64)  # 10^5 random values each, lazy and canonical
N_RANDOM = 100_000


def column_limit(qmax):
    """The largest column check_one_chain admits for this bound."""
    cmax = (1 << 64) - qmax * (1 << 26) - (1 << 39) - 1
    G.check_one_chain("test", qmax, cmax)
    with pytest.raises(AssertionError):
        G.check_one_chain("test", qmax, cmax + 1)
    return cmax


def spread(v, cmax, rng, mode):
    """Ten columns (each <= cmax) whose weighted sum is v. mode 0: normalised
    limbs; 1: as much as fits pushed into the lower columns; 2: random."""
    c = G.to_limbs(v)
    if mode == 0:
        return c
    for j in range(9, 0, -1):
        room = min(c[j], (cmax - c[j - 1]) >> 26)
        h = room if mode == 1 else rng.randrange(room + 1)
        c[j] -= h
        c[j - 1] += h << 26
    assert sum(x << (26 * j) for j, x in enumerate(c)) == v and max(c) <= cmax
    return c


@pytest.fixture(scope="module")
def harness(tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("redq") / "reduce_wide_host")
    subprocess.check_call(["g++", "-O1", "-g", "-std=c++17", "-fsanitize=address,undefined",
                           "-fno-sanitize-recover=all", "-I", os.path.join(ROOT, "handel_amd", "csrc"),
                           os.path.join(ROOT, "tests", "native", "reduce_wide_host.cpp"), "-o", exe])

    def run(cases):
        """cases: (qmax, lazy, columns) -> list of ten-limb results"""
        inp = "".join(f"{q} {int(lz)} " + " ".join(f"{x:x}" for x in c) + "\n" for q, lz, c in cases)
        r = subprocess.run([exe], input=inp, capture_output=True, text=True, timeout=300)
        assert r.returncode == 0, r.stderr[-2000:]
        assert r.stderr == "", r.stderr[-2000:]  # no sanitizer report
        out = [[int(x, 16) for x in line.split()] for line in r.stdout.splitlines()]
        assert len(out) == len(cases)
        return out

    return run


def check(cases, results):
    for (qmax, lazy, c), r in zip(cases, results):
        v = sum(x << (26 * j) for j, x in enumerate(c))
        got = G.from_limbs(r)
        assert len(r) == 10 and all(x < 1 << 26 for x in r[:9]), (qmax, lazy, v)
        if lazy:
            assert 0 <= got < 2 * P and (got - v) % P == 0, (qmax, lazy, v, got)
        else:
            assert got == v % P, (qmax, lazy, v, got)
        assert r == G.redq_tail_model(c, qmax, lazy), (qmax, lazy, v)


@pytest.mark.parametrize("qmax", QMAXES)
def test_multiples_of_p_and_their_neighbours(harness, qmax):
    rng = random.Random(qmax)
    cmax = column_limit(qmax)
    cases = []
    for lazy in (False, True):
        for k in range(qmax + 2):
            for v in (k * P - 1, k * P, k * P + 1):
                if 0 <= v < (qmax + 1) * P:
                    for mode in (0, 1, 2, 2):
                        cases.append((qmax, lazy, spread(v, cmax, rng, mode)))
    assert any(sum(x << (26 * j) for j, x in enumerate(c)) == (qmax + 1) * P - 1 for _, _, c in cases)
    assert any(max(c) > cmax - (1 << 27) for _, _, c in cases), "columns at the admitted magnitude"
    check(cases, harness(cases))


@pytest.mark.parametrize("lazy", [False, True], ids=["canonical", "lazy"])
@pytest.mark.parametrize("qmax", RANDOM_QMAXES)
def test_random_values_in_bound(harness, qmax, lazy):
    rng = random.Random(f"{qmax}{lazy}")
    cmax = column_limit(qmax)
    cases = []
    for i in range(N_RANDOM):
        v = rng.randrange((qmax + 1) * P)
        cases.append((qmax, lazy, spread(v, cmax, rng, 1 if i % 16 == 0 else 2)))
    check(cases, harness(cases))


def test_canonical_form_takes_the_rare_subtraction(harness):
    """Values just above a multiple of p leave V - q p in [p, p + eps): the
    guarded subtraction must run (the lazy form shows the unreduced value)."""
    cmax = column_limit(13)
    rng = random.Random(5)
    cases = [(13, True, spread(k * P + e, cmax, rng, 0)) for k in range(1, 14) for e in (0, 1, 12345)]
    lazy = harness(cases)
    assert any(G.from_limbs(r) >= P for r in lazy), "no case reaches the subtraction"
    canon = [(q, False, c) for q, _, c in cases]
    check(canon, harness(canon))
