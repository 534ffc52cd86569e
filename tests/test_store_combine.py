"""CPU suite: the host restatement of the store's outgoing multisignatures,
`partitioner.range_level_inverse` / `combine` / `combine_full` and
`Store.combined` / `full_signature`, on the cases of the reference's own tests
(partitioner_test.go:80-247,345-394; store_test.go:9-134) with a fake combine.
The device store (tests/test_gpu_store_merge.py) is tested against these."""

import pytest

from handel_amd import partitioner as P
from handel_amd import sigprocessing as S

FAKE = b"fake"


def fake_combine(a, b):
    return a  # util_test.go:97-99 fakeSig.Combine returns the receiver


def full_ms(level):
    """util_test.go:116-134 fullSig: every bit of a 2^(level-1)-bit set (1 bit at level 0)."""
    size = 1 << max(level - 1, 0)
    return S.MultiSig(size, (1 << size) - 1, FAKE)


def incoming(level, ms=None):
    return S.IncomingSig(-1, level, full_ms(level) if ms is None else ms)


def incomings(*levels):
    return [incoming(lv) for lv in levels]


def bits_of(*idx):
    v = 0
    for i in idx:
        v |= 1 << i
    return v


def all_bits(n):
    return (1 << n) - 1


@pytest.mark.parametrize("node,level,want", [
    # the lower part of the id space: whole powers of two
    (1, 0, (1, 2)), (1, 1, (1, 2)), (1, 2, (0, 2)), (1, 3, (0, 4)), (1, 4, (0, 8)), (1, 5, (0, 16)),
    (1, 6, (0, 17)),  # the whole id space
    (1, 7, None),
    # past the power of two: every range is the node itself
    (16, 0, (16, 17)), (16, 1, (16, 17)), (16, 2, (16, 17)), (16, 3, (16, 17)), (16, 4, (16, 17)),
    (16, 5, (16, 17)), (16, 6, (0, 17)), (16, 7, None),
])
def test_range_level_inverse(node, level, want):
    """partitioner_test.go:345-394 TestPartitionerBinTreeRangeAtInverse, N = 17."""
    if want is None:
        with pytest.raises(P.PartitionerError):
            P.range_level_inverse(node, 17, level)
    else:
        assert P.range_level_inverse(node, 17, level) == want


def test_range_level_inverse_is_the_aligned_block():
    """rangeLevelInverse(level + 1) is the 2^level block around the id, clipped
    at N: the alignment the device's Combined relies on."""
    for n in (9, 64, 200):
        for node in range(n):
            for level in range(P.log2_ceil(n)):
                lo = (node >> level) << level
                assert P.range_level_inverse(node, n, level + 1) == (lo, min(lo + (1 << level), n))


def test_partitioner_combine():
    """partitioner_test.go:80-152 TestPartitionerBinTreeCombine, N = 17."""
    n = 17
    with_holes = incomings(0, 2, 3)
    cases = [
        # from the last node
        (16, incomings(0), 1, (1, 1)),
        # a signature above the requested level
        (16, incomings(0, 5), 3, None),
        # the last node and every node before it
        (16, incomings(0, 5), 6, (n, all_bits(n))),
        # the first half
        (1, incomings(0, 1, 2, 3), 4, (8, all_bits(8))),
        # only one to combine: the level-2 bits of a 4-bit set
        (1, incomings(2), 3, (4, bits_of(2, 3))),
        (1, [], 0, None),
        # with holes: level 1 (id 0) is missing
        (1, with_holes, 4, (8, all_bits(8) & ~1)),
    ]
    for node, sigs, level, want in cases:
        got = P.combine(node, n, sigs, level, fake_combine)
        if want is None:
            assert got is None
        else:
            assert got == (want[0], want[1], FAKE), (node, level)


def test_partitioner_combine_full():
    """partitioner_test.go:154-246 TestPartitionerBinTreeCombineFull, N = 17."""
    n = 17
    holes = incomings(0, 1, 2, 3, 4)
    holes[4].ms.bits &= ~all_bits((1 << 3) - 1)  # level 4 keeps its last contribution only
    holes[3].ms.bits &= ~bits_of(1, 2)
    want_holes = all_bits(n) & ~bits_of(5, 6) & ~bits_of(*range(8, 15)) & ~bits_of(16)
    cases = [
        (16, incomings(0), bits_of(16)),
        (16, incomings(0, 5), all_bits(n)),
        (1, incomings(0, 1, 2, 3), all_bits(8)),
        (1, incomings(2), bits_of(2, 3)),
        (1, [], None),
        (1, holes, want_holes),
    ]
    for node, sigs, want in cases:
        got = P.combine_full(node, n, sigs, fake_combine)
        if want is None:
            assert got is None
        else:
            assert got == (n, want, FAKE), node


def test_combine_folds_signatures_in_order():
    seen = []

    def rec(a, b):
        seen.append((a, b))
        return a + b

    sigs = [S.IncomingSig(-1, lv, S.MultiSig(1 << max(lv - 1, 0), 1, bytes([lv]))) for lv in (0, 1, 2)]
    assert P.combine(1, 8, sigs, 3, rec) == (4, bits_of(1, 0, 2), b"\x00\x01\x02")
    assert seen == [(b"\x00", b"\x01"), (b"\x00\x01", b"\x02")]


def test_combine_refuses_bits_outside_the_range():
    # Combined(maxLevel) would place the top level below zero (the reference's bitset panics)
    with pytest.raises(P.PartitionerError):
        P.combine(0, 8, incomings(3), 3, fake_combine)


def test_store_combined():
    """store_test.go:9-47 TestStoreCombined, N = 9 (not a power of two)."""
    n = 9
    sig0, sig1, sig4 = incoming(0), incoming(1), incoming(4)
    cases = [
        (1, [sig0, sig1], 1, full_ms(2)),
        (1, [sig0], 0, full_ms(1)),
        (8, [sig0], 0, full_ms(1)),
        # combined with the rest: above the top level the whole id space
        (8, [sig0, sig4], 5, S.MultiSig(n, all_bits(n), FAKE)),
    ]
    for node, sigs, level, want in cases:
        st = S.Store(node, n, fake_combine)
        for sp in sigs:
            st.store(sp)
        assert st.combined(level) == want, (node, level)
    # the last case is the full-range result
    st = S.Store(8, n, fake_combine)
    st.store(sig0)
    st.store(sig4)
    assert st.combined(5) == st.full_signature()
    assert S.Store(3, n, fake_combine).combined(2) is None
    assert S.Store(3, n, fake_combine).full_signature() is None


def test_store_combined_every_level_n9():
    """N = 9: Combined(level) of a full store is the aligned block around the
    id, the levels node 8 does not have (1..3 are empty) left out."""
    n = 9
    for node in range(n):
        st = S.Store(node, n, fake_combine)
        st.store_own(FAKE)
        for lv in st.levels:
            size = st.size(lv)
            st.store(S.IncomingSig(-1, lv, S.MultiSig(size, all_bits(size), FAKE)))
        for level in range(st.max_level()):
            lo, hi = P.range_level_inverse(node, n, level + 1)
            assert st.combined(level) == S.MultiSig(hi - lo, all_bits(hi - lo), FAKE)
        assert st.full_signature() == S.MultiSig(n, all_bits(n), FAKE)


def test_store_full_signature():
    """store_test.go:49-67 TestStoreFullSignature: node 1's own signature is bit 1 of 8."""
    st = S.Store(1, 8, fake_combine)
    assert st.store_own(FAKE) == S.MultiSig(1, 1, FAKE)
    ms = st.full_signature()
    assert ms.bitlen == 8 and ms.bits == bits_of(1)
    assert st.best(0) == (S.MultiSig(1, 1, FAKE), True)


def test_store_unsafe_check_merge():
    """store_test.go:69-134 TestStoreUnsafeCheckMerge, node 0 of 8, level 3."""
    st = S.Store(0, 8, fake_combine)
    ind = S.IncomingSig(1, 3, S.MultiSig(4, bits_of(0), FAKE), ind=True, mapped_index=0)
    ms, keep = st._unsafe_check_merge(ind)
    assert keep and ms.bits == bits_of(0)
    st.store(ind)
    # again: it exists already
    assert st._unsafe_check_merge(ind) == (None, False)
    # a larger signature gets in
    two = S.IncomingSig(1, 3, S.MultiSig(4, bits_of(0, 2), FAKE))
    ms, keep = st._unsafe_check_merge(two)
    assert keep and ms.bits == bits_of(0, 2)
    st.store(two)
    assert st.best(3)[0].bits == bits_of(0, 2)
    # size 2 as well, but the individual signature complements it to 3
    other = S.IncomingSig(1, 3, S.MultiSig(4, bits_of(2, 3), FAKE))
    ms, keep = st._unsafe_check_merge(other)
    assert keep and ms.bits == bits_of(0, 2, 3)
