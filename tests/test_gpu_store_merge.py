"""The opt-in device store (hg_stores_enable_merge, hg_merge.hip): merging the
verified picks of an intake step where they lie and producing Combined /
FullSignature on the GPU. Expected bits and bytes always come from the host
`sigprocessing.Store` (store.go:82-262, pinned by tests/test_store_combine.py)
with `combine` = the CPU oracle's g1_add, which shares nothing with the kernels
under test. Signatures are real G1 points signed with distinct random scalars
(the merge never verifies), so a missing or doubled term changes a sum."""

import random

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

HG_OK, HG_ERR_SIG_INVALID, HG_ERR_ARG = 0, 1, 100
SKIPPED, STORED, DISCARDED, ERR_MISSING, ERR_INDIVIDUAL, ERR_ROW = range(6)
EMPTY, COMBINED_ERR_MISSING = 1, 2
HAS_BEST, BEST_SIG = 1, 2
FULL = 0xFFFFFFFF
OUTCOMES = ("first_best", "disjoint_merge", "overlap_replace", "discard", "individual", "complement")


def _engine(nreg: int, flavor: str = "go"):
    import bench
    from handel_amd.engine import Engine

    e = Engine(device=0, flavor=flavor)
    assert e.set_message(bench.LIB_MESSAGE) == 0
    assert not e.registry_load(e.keygen(bench.seeded_scalars(nreg, 77 + nreg))).any()
    return e


def _sig_pool(e, count: int, seed: int):
    """count distinct signatures: the message signed with distinct random scalars"""
    import bench

    sg = e.sign(bench.seeded_scalars(count, 9000 + seed))
    pool = [sg[64 * i:64 * i + 64] for i in range(count)]
    assert len(set(pool)) == count
    return pool


def _rand_bits(rng, size: int, density: float) -> int:
    bits = rng.random(size) < density
    return int.from_bytes(np.packbits(bits, bitorder="little").tobytes(), "little")


def _oracle_combine(a: bytes, b: bytes) -> bytes:
    from oracle import ref_lib as R

    return R.g1_add(a, b)


def _val(words) -> int:
    return int.from_bytes(np.ascontiguousarray(words).astype("<u8").tobytes(), "little")


class Entry:
    """One picked slot: a multisignature (or, individual, the one-bit set of
    `origin`) for (receiver, level), with its verdict."""

    def __init__(self, receiver, level, origin, bits, sig, individual=False, ok=True):
        self.receiver, self.level, self.origin, self.bits, self.sig = receiver, level, origin, bits, sig
        self.individual, self.ok = individual, ok

    def incoming(self, nreg):
        from handel_amd import partitioner as HP
        from handel_amd.sigprocessing import IncomingSig, MultiSig

        lo, hi = HP.range_level(self.receiver, nreg, self.level)
        return IncomingSig(self.origin, self.level, MultiSig(hi - lo, self.bits, self.sig), ind=self.individual,
                           mapped_index=self.origin - lo if self.individual else 0)


def _host_apply(host, nreg, entries):
    """The host Store fed the OK entries in order: (result per entry, changed
    (receiver, level) in the order of their first applied entry)."""
    results, first, changed = [], [], set()
    for en in entries:
        if not en.ok:
            results.append(SKIPPED)
            continue
        row = (en.receiver, en.level)
        if row not in first:
            first.append(row)
        kept = host[en.receiver].store(en.incoming(nreg))
        results.append(STORED if kept is not None else DISCARDED)
        if kept is not None:
            changed.add(row)
    return results, [row for row in first if row in changed]


def _run_merge(e, st, nreg, entries, fillers=3, use_count=True):
    """entries -> the parse-shaped arrays (entry i is packet i: slot i, or slot
    n + i when individual) -> hg_stores_merge_device: (results, changed rows)."""
    import torch

    from handel_amd.engine import PACKET_DTYPE

    n, stride = len(entries), st.stride
    pkts = np.zeros(n, dtype=PACKET_DTYPE)
    words = np.zeros(2 * n * stride, dtype=np.uint64)
    sigs = np.zeros((2 * n, 64), dtype=np.uint8)
    sel = np.full(n + fillers, 0xFFFFFFFF, dtype=np.uint32)
    vcodes = np.full(n + fillers, HG_OK, dtype=np.int32)  # a filler is told by its slot (or the count), not its verdict
    for i, en in enumerate(entries):
        pkts[i]["receiver"], pkts[i]["level"], pkts[i]["origin"] = en.receiver, en.level, en.origin
        slot = n + i if en.individual else i
        words[slot * stride:(slot + 1) * stride] = np.frombuffer(en.bits.to_bytes(8 * stride, "little"), dtype="<u8")
        sigs[slot] = np.frombuffer(en.sig, dtype=np.uint8)
        sel[i] = slot
        vcodes[i] = HG_OK if en.ok else HG_ERR_SIG_INVALID
    cap = n + fillers
    dev = torch.device("cuda", 0)
    up = lambda a: torch.from_numpy(np.ascontiguousarray(a).view(np.uint8).reshape(-1).copy()).to(dev)  # noqa: E731
    d_pkts, d_words, d_sigs, d_sel, d_vcodes = up(pkts), up(words), up(sigs), up(sel), up(vcodes)
    d_count = up(np.array([n], dtype=np.uint32))
    d_results = torch.full((cap,), -9, dtype=torch.int32, device=dev)
    d_changed = torch.full((2 * cap,), -9, dtype=torch.int32, device=dev)
    d_nchanged = torch.full((1,), -9, dtype=torch.int32, device=dev)
    s = torch.cuda.current_stream(dev).cuda_stream
    st.merge_device(d_pkts.data_ptr(), n, d_sel.data_ptr(), d_count.data_ptr() if use_count else 0, cap,
                    d_vcodes.data_ptr(), stride, d_words.data_ptr(), d_sigs.data_ptr(), d_results.data_ptr(),
                    d_changed.data_ptr(), d_nchanged.data_ptr(), s)
    torch.cuda.synchronize(dev)
    results = d_results.cpu().numpy()
    assert (results[n:] == SKIPPED).all()  # the filler
    nch = int(d_nchanged.cpu()[0])
    changed = [tuple(x) for x in d_changed.cpu().numpy()[:2 * nch].reshape(-1, 2).tolist()]
    return results[:n].tolist(), changed


def _assert_rows_equal(st, host, nreg, rows=None):
    """every level's best bits, best signature, flags and individual set on the device equal the host Store's"""
    for r, store in host.items():
        for lv in store.levels:
            if rows is not None and (r, lv) not in rows:
                continue
            best, sig, flags = st.read_best(r, lv)
            _, indiv, has = st.read(r, lv)
            want = store.m.get(lv)
            assert has == (want is not None) == bool(flags & HAS_BEST), (r, lv)
            if want is not None:
                assert flags & BEST_SIG, (r, lv)
                assert _val(best) == want.bits, (r, lv)
                assert sig == want.sig, (r, lv)
            assert _val(indiv) == store.indiv_verified[lv], (r, lv)


# ------------------------------------------------------------------ 1. reference vectors
def test_unsafe_check_merge_vectors():
    """store_test.go:69-134 TestStoreUnsafeCheckMerge at N = 8, node 0, level 3
    ([4, 8)): the individual {0}, the same again, {0, 2}, then {2, 3} which the
    individual complements to {0, 2, 3}."""
    from handel_amd.intake import DeviceStores
    from handel_amd.sigprocessing import Store

    e = _engine(8)
    try:
        p = _sig_pool(e, 3, 1)
        st = DeviceStores(e, [0], 16)
        st.enable_merge()
        host = {0: Store(0, 8, _oracle_combine)}
        sets = []
        for en, want in ((Entry(0, 3, 4, 0b0001, p[0], individual=True), STORED),
                         (Entry(0, 3, 4, 0b0001, p[0], individual=True), DISCARDED),
                         (Entry(0, 3, 4, 0b0101, p[1]), STORED),
                         (Entry(0, 3, 4, 0b1100, p[2]), STORED)):
            want_res, want_changed = _host_apply(host, 8, [en])
            assert want_res == [want]
            assert _run_merge(e, st, 8, [en]) == ([want], want_changed)
            _assert_rows_equal(st, host, 8)
            sets.append(_val(st.read_best(0, 3)[0]))
        assert sets == [0b0001, 0b0001, 0b0101, 0b1101]
        assert st.read_best(0, 3)[1] == _oracle_combine(p[0], p[2])
        st.close()
    finally:
        e.close()


# ------------------------------------------------------------------ 2. randomised parity
def _merge_case(nreg: int, n_stores: int, seed: int, n_entries: int = 256):
    """A seeded state and `n_entries` entries over the four largest levels of
    `n_stores` stores, generated against a simulated store so that every
    outcome of unsafeCheckMerge occurs. Signatures are indices into a pool.
    Returns (receivers, seeds, entries, outcome counts, pool size): seeds =
    (receiver, level, best bits or None, best sig, {index: sig}); entries =
    Entry with sig = pool index."""
    from handel_amd import partitioner as HP
    from handel_amd.sigprocessing import MultiSig, Store

    rnd = random.Random(seed)
    rng = np.random.default_rng(seed)
    receivers = rnd.sample(range(nreg), n_stores)
    nsig = [0]

    def new_sig():
        nsig[0] += 1
        return nsig[0] - 1

    sim, seeds, ind_sig, active = {}, [], {}, {}
    for r in receivers:
        s = Store(r, nreg, lambda a, b: a)
        active[r] = s.levels[-4:]
        for lv in active[r]:
            size = s.size(lv)
            best = None
            if rnd.random() < 0.4:
                best = _rand_bits(rng, size, rnd.choice([0.1, 0.4])) | 1 << rnd.randrange(size)
                s.m[lv] = MultiSig(size, best, new_sig())
            held, density = {}, rnd.choice([0.0, 0.03, 0.1])
            for idx in range(size):
                if rnd.random() < density:
                    held[idx] = ind_sig[(r, lv, idx)] = new_sig()
                    s.indiv_verified[lv] |= 1 << idx
                    s.indiv_sigs[lv][idx] = MultiSig(size, 1 << idx, held[idx])
            seeds.append((r, lv, best, s.m[lv].sig if best is not None else None, held))
        sim[r] = s
    entries, counts = [], dict.fromkeys(OUTCOMES, 0)
    for _ in range(n_entries):
        r = rnd.choice(receivers)
        s = sim[r]
        lv = rnd.choice(active[r])
        lo, hi = HP.range_level(r, nreg, lv)
        size, full = hi - lo, (1 << (hi - lo)) - 1
        cur = s.m.get(lv)
        best = cur.bits if cur is not None else 0
        kind = rnd.choice(["disjoint", "disjoint", "overlap", "overlap", "subset", "indiv", "indiv", "random"])
        origin = lo + rnd.randrange(size)
        if kind == "indiv":
            bits = 1 << (origin - lo)
            sig = ind_sig.setdefault((r, lv, origin - lo), new_sig())  # deterministic: one signature per signer
        else:
            if kind == "disjoint":
                bits = full & ~best & _rand_bits(rng, size, rnd.choice([0.1, 0.5]))
            elif kind == "overlap":
                bits = (best & _rand_bits(rng, size, 0.5)) | (full & ~best & _rand_bits(rng, size, 0.6))
            elif kind == "subset":
                bits = best & _rand_bits(rng, size, 0.7)
            else:
                bits = _rand_bits(rng, size, rnd.choice([0.05, 0.3, 0.9]))
            bits = bits or 1 << rnd.randrange(size)
            sig = new_sig()
        en = Entry(r, lv, origin, bits, sig, individual=kind == "indiv", ok=rnd.random() < 0.8)
        entries.append(en)
        if not en.ok:
            continue
        ivs = s.indiv_verified[lv] | (bits if en.individual else 0)
        counts["individual"] += en.individual
        if cur is None:
            counts["first_best"] += 1
        else:
            disjoint = not bits & best
            cand = bits | best if disjoint else bits
            i_s = ivs & ~cand
            if i_s.bit_count() + cand.bit_count() <= best.bit_count():
                counts["discard"] += 1
            else:
                counts["disjoint_merge" if disjoint else "overlap_replace"] += 1
                counts["complement"] += i_s != 0
        s.store(en.incoming(nreg))
    return receivers, seeds, entries, counts, nsig[0]


MERGE_CASES = [(64, 6, 11), (200, 4, 12), (4000, 8, 13)]


@pytest.mark.parametrize("flavor", ["go", "cf"])
@pytest.mark.parametrize("nreg,n_stores,seed", MERGE_CASES)
def test_merge_equals_host_store(nreg, n_stores, seed, flavor):
    """Strides 1, 2 and 32 words; 256 entries, several per (store, level),
    verdicts mixed, over a seeded state: every result, the changed list and
    every level's state equal the host Store's; each outcome of
    unsafeCheckMerge occurs at least 8 times."""
    from handel_amd.intake import DeviceStores
    from handel_amd.sigprocessing import MultiSig, Store

    receivers, seeds, entries, counts, npool = _merge_case(nreg, n_stores, seed)
    print("merge outcomes", nreg, counts)
    assert min(counts.values()) >= 8, counts
    e = _engine(nreg, flavor)
    try:
        assert e.packet_stride_words() == {64: 1, 200: 2, 4000: 32}[nreg]
        pool = _sig_pool(e, npool, seed)
        host = {r: Store(r, nreg, _oracle_combine) for r in receivers}
        for r, lv, best, best_sig, held in seeds:
            s = host[r]
            if best is not None:
                s.m[lv] = MultiSig(s.size(lv), best, pool[best_sig])
            for idx, sg in held.items():
                s.indiv_verified[lv] |= 1 << idx
                s.indiv_sigs[lv][idx] = MultiSig(s.size(lv), 1 << idx, pool[sg])
        st = DeviceStores(e, receivers, len(entries))
        st.enable_merge()
        st.mirror_many([(r, host[r], None) for r in receivers])  # hg_stores_update + hg_stores_update_sigs
        _assert_rows_equal(st, host, nreg)
        for en in entries:
            en.sig = pool[en.sig]
        want_res, want_changed = _host_apply(host, nreg, entries)
        got_res, got_changed = _run_merge(e, st, nreg, entries)
        bad = [i for i, (a, b) in enumerate(zip(got_res, want_res)) if a != b]
        assert not bad, (bad[:8], [got_res[i] for i in bad[:8]], [want_res[i] for i in bad[:8]])
        assert got_changed == want_changed
        _assert_rows_equal(st, host, nreg)
        st.close()
    finally:
        e.close()


# ------------------------------------------------------------------ 3. long complement
def test_long_complement():
    """N = 200, node 130, level 8 = [0, 128): 70 verified individual signatures
    held, a best of 20 others, then one multisignature disjoint from both: the
    lanes' loops over two words of the complement and the whole tree run."""
    from handel_amd import partitioner as HP
    from handel_amd.intake import DeviceStores
    from handel_amd.sigprocessing import MultiSig, Store

    nreg, r, lv = 200, 130, 8
    assert HP.range_level(r, nreg, lv) == (0, 128)
    e = _engine(nreg)
    try:
        pool = _sig_pool(e, 72, 3)
        rnd = random.Random(3)
        held = rnd.sample(range(128), 70)
        rest = [i for i in range(128) if i not in held]
        host = {r: Store(r, nreg, _oracle_combine)}
        s = host[r]
        for j, idx in enumerate(held):
            s.indiv_verified[lv] |= 1 << idx
            s.indiv_sigs[lv][idx] = MultiSig(128, 1 << idx, pool[j])
        s.m[lv] = MultiSig(128, sum(1 << i for i in rest[:20]), pool[70])
        st = DeviceStores(e, [r], 8)
        st.enable_merge()
        st.mirror(r, s)
        en = Entry(r, lv, rest[20], sum(1 << i for i in rest[20:40]), pool[71])
        assert _host_apply(host, nreg, [en]) == ([STORED], [(r, lv)])
        assert s.m[lv].cardinality() == 110
        assert _run_merge(e, st, nreg, [en], use_count=False) == ([STORED], [(r, lv)])
        _assert_rows_equal(st, host, nreg)
        st.close()
    finally:
        e.close()


# ------------------------------------------------------------------ 4. group-law edges
@pytest.mark.parametrize("flavor", ["go", "cf"])
def test_group_law_edges(flavor):
    """Two disjoint entries carrying the same point (the doubling branch of the
    addition) and a point with its negation (scalars s and r - s: infinity):
    the bytes are the oracle's g1_add's."""
    import bench
    from handel_amd.intake import DeviceStores
    from handel_amd.sigprocessing import Store

    nreg = 64
    e = _engine(nreg, flavor)
    try:
        s = 0x1234567 + 99
        sg = e.sign(s.to_bytes(32, "big") + (bench.ORDER - s).to_bytes(32, "big"))
        pt, neg = sg[:64], sg[64:]
        assert _oracle_combine(pt, neg) == bytes(64) and _oracle_combine(pt, pt) not in (pt, bytes(64))
        host = {5: Store(5, nreg, _oracle_combine)}
        st = DeviceStores(e, [5], 8)
        st.enable_merge()
        entries = [Entry(5, 6, 40, 0b0011, pt), Entry(5, 6, 42, 0b1100, pt),      # level 6 = [32, 64): doubling
                   Entry(5, 5, 20, 0b0001, pt), Entry(5, 5, 21, 0b0110, neg)]     # level 5 = [16, 32): infinity
        want = _host_apply(host, nreg, entries)
        assert want[0] == [STORED] * 4
        assert _run_merge(e, st, nreg, entries) == want
        _assert_rows_equal(st, host, nreg)
        assert st.read_best(5, 6)[1] == _oracle_combine(pt, pt)
        assert st.read_best(5, 5)[1] == bytes(64)
        # infinity is a term like any other afterwards
        more = [Entry(5, 5, 24, 0b1000 << 5, pt)]
        assert _run_merge(e, st, nreg, more) == _host_apply(host, nreg, more)
        assert st.read_best(5, 5)[1] == pt
        _assert_rows_equal(st, host, nreg)
        st.close()
    finally:
        e.close()


# ------------------------------------------------------------------ 5. missing signature
def test_missing_signature_is_an_error():
    """Bits set with plain hg_stores_update and no signature given: a merge
    that needs them gets the error, its row stays as it was, and the rest of
    the batch is applied."""
    from handel_amd.engine import STORE_UPDATE_DTYPE
    from handel_amd.intake import DeviceStores
    from handel_amd.sigprocessing import Store

    nreg = 64
    e = _engine(nreg)
    try:
        p = _sig_pool(e, 6, 5)
        st = DeviceStores(e, [5, 9], 8)
        st.enable_merge()
        # receiver 5: level 6 has a best {0, 1} without signature; level 5 a verified individual {3} without signature
        ups = np.array([(5, 6, HAS_BEST, 0, 1), (5, 5, 0, 1, 2)], dtype=STORE_UPDATE_DTYPE)
        st.update(ups, np.array([0b0011, 0, 0b1000], dtype=np.uint64))
        host = {9: Store(9, nreg, _oracle_combine)}
        entries = [Entry(9, 6, 40, 0b0101, p[0]),
                   Entry(5, 6, 40, 0b1100, p[1]),           # disjoint from the best: needs its signature
                   Entry(5, 5, 17, 0b0001, p[2]),           # first best: needs nothing
                   Entry(5, 5, 18, 0b0110, p[3]),           # disjoint, and {3} complements it: its signature is missing
                   Entry(5, 6, 40, 0b0111, p[4]),           # overlaps {0, 1} and is larger: a plain replace
                   Entry(9, 6, 44, 0b1010 << 4, p[5])]
        res, changed = _run_merge(e, st, nreg, entries)
        assert res == [STORED, ERR_MISSING, STORED, ERR_MISSING, STORED, STORED]
        assert changed == [(9, 6), (5, 6), (5, 5)]
        _host_apply(host, nreg, [entries[0], entries[5]])
        _assert_rows_equal(st, host, nreg)
        best, sig, flags = st.read_best(5, 5)
        assert (_val(best), sig, flags) == (0b0001, p[2], HAS_BEST | BEST_SIG)
        assert _val(st.read(5, 5)[1]) == 0b1000
        best, sig, flags = st.read_best(5, 6)
        assert (_val(best), sig, flags) == (0b0111, p[4], HAS_BEST | BEST_SIG)
        # an individual slot whose set is not its one bit changes nothing either
        bad = [Entry(9, 5, 17, 0b0011, p[1], individual=True), Entry(9, 5, 18, 0b0001, p[1], individual=True)]
        assert _run_merge(e, st, nreg, bad) == ([ERR_INDIVIDUAL, ERR_INDIVIDUAL], [])
        assert st.read_best(9, 5)[2] == 0 and _val(st.read(9, 5)[1]) == 0
        st.close()
    finally:
        e.close()


# ------------------------------------------------------------------ 6. Combined and FullSignature
def _random_store(rnd, rng, r, nreg, pool, nxt):
    from handel_amd.sigprocessing import MultiSig, Store

    s = Store(r, nreg, _oracle_combine)
    if rnd.random() < 0.8:
        s.store_own(pool[next(nxt)])
    for lv in s.levels:
        if rnd.random() < 0.7:
            size = s.size(lv)
            s.m[lv] = MultiSig(size, _rand_bits(rng, size, rnd.choice([0.1, 0.5, 1.0])) | 1 << rnd.randrange(size),
                               pool[next(nxt)])
    return s


@pytest.mark.parametrize("nreg", [9, 64, 200, 4000])
def test_combined_equals_host_store(nreg):
    """Every (receiver, level < maxLevel) and the full query against
    Store.combined / full_signature; N = 9 has empty levels (node 8) and
    clipped ranges, 4000 a ragged 1952-id level."""
    import itertools

    import torch

    from handel_amd import partitioner as HP
    from handel_amd.engine import STORE_QUERY_DTYPE, STORE_UPDATE_DTYPE
    from handel_amd.intake import DeviceStores

    rnd = random.Random(600 + nreg)
    rng = np.random.default_rng(600 + nreg)
    receivers = list(range(nreg)) if nreg == 9 else rnd.sample(range(nreg), 8)
    top = HP.log2_ceil(nreg)
    e = _engine(nreg)
    try:
        pool = _sig_pool(e, len(receivers) * (top + 1), nreg)
        nxt = itertools.count()
        host = {r: _random_store(rnd, rng, r, nreg, pool, nxt) for r in receivers}
        from handel_amd.sigprocessing import Store

        host[receivers[-1]] = Store(receivers[-1], nreg, _oracle_combine)  # one store holds nothing
        st = DeviceStores(e, receivers, 8)
        st.enable_merge()
        st.mirror_many([(r, host[r], None) for r in receivers])
        queries = [(r, lv) for r in receivers for lv in list(range(top)) + [FULL]]
        want = [host[r].full_signature() if lv == FULL else host[r].combined(lv) for r, lv in queries]
        assert sum(w is None for w in want) >= top + 1 and sum(w is not None for w in want) > len(receivers)
        ws = (nreg + 63) // 64
        codes, bitlens, words, sigs = st.combined(queries)

        def check(codes, bitlens, words, sigs, queries, want):
            for q, ms in enumerate(want):
                if ms is None:
                    assert codes[q] == EMPTY and bitlens[q] == 0, queries[q]
                    assert not words[q].any() and not sigs[q].any()
                else:
                    assert codes[q] == HG_OK, queries[q]
                    assert (int(bitlens[q]), _val(words[q]), sigs[q].tobytes()) == (ms.bitlen, ms.bits, ms.sig), queries[q]

        check(codes, bitlens, words, sigs, queries, want)
        # the device form agrees with the host-pointer form
        dev = torch.device("cuda", 0)
        m = len(queries)
        d_q = torch.from_numpy(np.array(queries, dtype=STORE_QUERY_DTYPE).view(np.uint8).copy()).to(dev)
        d_codes = torch.full((m,), -9, dtype=torch.int32, device=dev)
        d_bitlens = torch.full((m,), -9, dtype=torch.int32, device=dev)
        d_words = torch.full((m * ws,), -1, dtype=torch.int64, device=dev)
        d_sigs = torch.full((m * 64,), 0x55, dtype=torch.uint8, device=dev)
        st.combined_device(d_q.data_ptr(), m, ws, d_codes.data_ptr(), d_bitlens.data_ptr(), d_words.data_ptr(),
                           d_sigs.data_ptr(), torch.cuda.current_stream(dev).cuda_stream)
        torch.cuda.synchronize(dev)
        assert np.array_equal(d_codes.cpu().numpy(), codes)
        assert np.array_equal(d_bitlens.cpu().numpy().view(np.uint32), bitlens)
        assert np.array_equal(d_words.cpu().numpy().view(np.uint64).reshape(m, ws), words)
        assert np.array_equal(d_sigs.cpu().numpy().reshape(m, 64), sigs)
        # a level at or above maxLevel is refused for that query only
        r0 = receivers[0]
        mixed = [(r0, top), (r0, 0), (r0, top + 3), (r0, FULL)]
        codes, bitlens, words, sigs = st.combined(mixed)
        assert codes[0] == codes[2] == HG_ERR_ARG and not words[0].any() and not sigs[2].any()
        check(codes[[1, 3]], bitlens[[1, 3]], words[[1, 3]], sigs[[1, 3]], [mixed[1], mixed[3]],
              [host[r0].combined(0), host[r0].full_signature()])
        # hg_stores_update replaces a bitset: its signature is no longer known
        r1, lv1 = next((r, lv) for r in receivers for lv in host[r].levels if lv in host[r].m and lv < top)
        size = host[r1].size(lv1)
        nw = (size + 63) // 64
        full_words = np.frombuffer(((1 << size) - 1).to_bytes(8 * nw, "little"), dtype="<u8")
        st.update(np.array([(r1, lv1, HAS_BEST, 0, nw)], dtype=STORE_UPDATE_DTYPE),
                  np.concatenate([full_words, np.zeros(nw, dtype=np.uint64)]))
        assert st.read_best(r1, lv1)[2] == HAS_BEST
        below = [(r1, lv) for lv in range(lv1)]
        above = [(r1, lv) for lv in range(lv1, top)] + [(r1, FULL)]
        codes, bitlens, words, sigs = st.combined(below + above)
        assert (codes[len(below):] == COMBINED_ERR_MISSING).all() and not sigs[len(below):].any()
        check(codes[:len(below)], bitlens, words, sigs, below, [host[r1].combined(lv) for lv in range(lv1)])
        st.close()
    finally:
        e.close()


# ------------------------------------------------------------------ 7. the chain
def test_device_merge_intake_equals_host_pipeline():
    """test_gpu_intake.test_device_intake_equals_host_pipeline's shape (N = 64,
    8 receivers, k = 4, three steps of 100 real packets, 1/8 invalid) with
    DeviceIntake(device_merge=True): the same picks and verdicts, and after
    each step every level's best, individual set and Combined on the device
    equal the host pipeline's stores; the device's multisignatures verify."""
    import bench
    from handel_amd import partitioner as HP
    from handel_amd.engine import Engine, REQ_DTYPE
    from handel_amd.intake import DeviceIntake
    from handel_amd.packets import Packet
    from handel_amd.sigprocessing import (BatchedEvaluatorProcessing, EvaluatorStore, IncomingSig, MultiSig, Store,
                                          bits_to_int, int_to_words)

    nreg, k = 64, 4
    top = HP.log2_ceil(nreg)
    e = Engine(device=0, flavor="go")
    try:
        assert e.set_message(bench.LIB_MESSAGE) == 0
        kb = bench.seeded_scalars(nreg, 321)
        assert not e.registry_load(e.keygen(kb)).any()
        ks = [int.from_bytes(kb[32 * i:32 * i + 32], "big") for i in range(nreg)]
        own = e.sign(kb)
        rnd = random.Random(66)
        receivers = rnd.sample(range(nreg), 8)

        def make_step(count):
            metas, scalars = [], bytearray()
            for _ in range(count):
                r = rnd.choice(receivers)
                lv, lo, hi = rnd.choice(HP.level_sizes(r, nreg))
                size = hi - lo
                bits = [rnd.random() < rnd.uniform(0.2, 1.0) for _ in range(size)]
                origin = lo + rnd.randrange(size)
                bits[origin - lo] = True
                agg = sum(ks[lo + j] for j in range(size) if bits[j]) % bench.ORDER
                has_ind = rnd.random() < 0.5
                scalars += ((agg + (rnd.random() < 0.125)) % bench.ORDER or 1).to_bytes(32, "big")
                scalars += ((ks[origin] + (rnd.random() < 0.125)) % bench.ORDER or 1).to_bytes(32, "big")
                metas.append((r, lv, lo, size, bits, origin, has_ind))
            sg = e.sign(bytes(scalars))
            pkts, recv, incoming = [], [], []
            for i, (r, lv, lo, size, bits, origin, has_ind) in enumerate(metas):
                ms_sig, ind_sig = sg[128 * i:128 * i + 64], sg[128 * i + 64:128 * i + 128]
                pkts.append(Packet(origin, lv, HP.multisig_marshal(bits, ms_sig), ind_sig if has_ind else None))
                recv.append(r)
                sps = [IncomingSig(origin, lv, MultiSig(size, bits_to_int(bits), ms_sig))]
                if has_ind:
                    sps.append(IncomingSig(origin, lv, MultiSig(size, 1 << (origin - lo), ind_sig), ind=True,
                                           mapped_index=origin - lo))
                incoming.append(sps)
            return pkts, recv, incoming

        def host_verify(r, sps):
            reqs, words = np.zeros(len(sps), dtype=REQ_DTYPE), []
            for j, sp in enumerate(sps):
                lo, hi = HP.range_level(r, nreg, sp.level)
                reqs[j] = (lo, sp.ms.bitlen, hi - lo, len(words))
                words += list(int_to_words(sp.ms.bits, sp.ms.bitlen))
            codes = e.verify_aggregate(reqs, np.array(words, dtype=np.uint64), b"".join(sp.ms.sig for sp in sps))
            return [None if c == 0 else e.processing_error_string(int(c)) for c in codes]

        host = {r: Store(r, nreg, _oracle_combine) for r in receivers}
        procs = {r: BatchedEvaluatorProcessing(lambda sps, r=r: host_verify(r, sps), EvaluatorStore(host[r]), batch=k)
                 for r in receivers}
        di = DeviceIntake(e, receivers, k, max_packets=1024, device_merge=True)
        for r in receivers:
            host[r].store_own(own[64 * r:64 * r + 64])
            di.set_own(r, own[64 * r:64 * r + 64])
        key = lambda sp: (sp.origin, sp.level, sp.ind, sp.ms.bits, sp.ms.sig)  # noqa: E731
        stored = 0
        for step in range(3):
            pkts, recv, incoming = make_step(100)
            results, unselected = di.step(pkts, recv)
            for r, sps in zip(recv, incoming):
                for sp in sps:
                    procs[r].add(sp)
            want, want_res, want_changed = [], [], []
            for r in receivers:
                if not procs[r].todos:
                    continue
                done, best = procs[r].read_todos()
                assert not done
                for sp, err in zip(best, host_verify(r, best) if best else []):
                    want.append((r, key(sp), err))
                    if err is None:
                        kept = host[r].store(sp)
                        want_res.append(STORED if kept is not None else DISCARDED)
                        if kept is not None and (r, sp.level) not in want_changed:
                            want_changed.append((r, sp.level))
                    else:
                        want_res.append(SKIPPED)
            assert [(r, key(sp), err) for r, sp, err in results] == want, step
            assert di.last_results == want_res, step
            assert sorted(di.last_changed) == sorted(want_changed), step
            stored += want_res.count(STORED)
            assert len(unselected) == sum(len(procs[r].todos) for r in receivers) == len(di.pending)
            assert not any(di.host[r].m for r in receivers)  # the host stores of the intake are not used
            vreqs, vwords, vsigs = [], [], b""
            for r in receivers:
                for lv in [0] + host[r].levels:
                    assert di.best(r, lv) == host[r].best(lv)[0], (step, r, lv)
                    if lv:
                        assert _val(di.stores.read(r, lv)[1]) == host[r].indiv_verified[lv], (step, r, lv)
                for lv in list(range(top)) + [None]:
                    ms = di.combined(r, lv)
                    assert ms == (host[r].full_signature() if lv is None else host[r].combined(lv)), (step, r, lv)
                    # what the peers of level lv + 1 verify: their level's range is this block
                    lo = 0 if lv is None else HP.range_level_inverse(r, nreg, lv + 1)[0]
                    vreqs.append((lo, ms.bitlen, ms.bitlen, len(vwords)))
                    vwords += list(int_to_words(ms.bits, ms.bitlen))
                    vsigs += ms.sig
            codes = e.verify_aggregate(np.array(vreqs, dtype=REQ_DTYPE), np.array(vwords, dtype=np.uint64), vsigs)
            assert not codes.any(), step
        assert stored > 20 and di.pending
        di.close()
    finally:
        e.close()


# ------------------------------------------------------------------ 8. not enabled
def test_not_enabled_is_refused_and_scoring_is_unchanged():
    """Without hg_stores_enable_merge the new entry points return HG_ERR_ARG
    before any pointer is used; an enabled set scores and selects as before."""
    import torch

    from handel_amd._lib import HandelGPUError
    from handel_amd.engine import PACKET_DTYPE, REQ_DTYPE, STORE_SIG_DTYPE
    from handel_amd.intake import DeviceStores
    from handel_amd.sigprocessing import MultiSig, Store

    nreg, n, k = 200, 64, 3
    e = _engine(nreg)
    try:
        rnd = random.Random(8)
        rng = np.random.default_rng(8)
        receivers = rnd.sample(range(nreg), 4)
        plain = DeviceStores(e, receivers, n)
        z = np.zeros(64, dtype=np.uint64)
        p = z.ctypes.data
        for call in (lambda: plain.merge_device(p, 1, p, p, 1, p, plain.stride, p, p, p, p, p),
                     lambda: plain.combined([(receivers[0], 0)]),
                     lambda: plain.combined_device(p, 1, 4, p, p, p, p),
                     lambda: plain.read_best(receivers[0], 1),
                     lambda: plain.update_sigs(np.array([(receivers[0], 0, 0, 0)], dtype=STORE_SIG_DTYPE), bytes(64))):
            with pytest.raises(HandelGPUError, match="code 100"):
                call()
        merged = DeviceStores(e, receivers, n)
        merged.enable_merge()
        merged.enable_merge()  # idempotent
        host = {}
        for r in receivers:
            s = Store(r, nreg, _oracle_combine)
            for lv in s.levels:
                size = s.size(lv)
                if rnd.random() < 0.6:
                    s.m[lv] = MultiSig(size, _rand_bits(rng, size, 0.4) | 1, bytes(64))
                s.indiv_verified[lv] = _rand_bits(rng, size, 0.2)
            host[r] = s
        stride = plain.stride
        pkts = np.zeros(n, dtype=PACKET_DTYPE)
        words = np.zeros(2 * n * stride, dtype=np.uint64)
        codes = np.zeros(2 * n, dtype=np.int32)
        for i in range(n):
            r = rnd.choice(receivers)
            lv = rnd.choice(host[r].levels)
            size = host[r].size(lv)
            pkts[i]["receiver"], pkts[i]["level"], pkts[i]["origin"] = r, lv, 0
            bits = _rand_bits(rng, size, 0.5) | 1
            words[i * stride:(i + 1) * stride] = np.frombuffer(bits.to_bytes(8 * stride, "little"), dtype="<u8")
            words[(n + i) * stride] = 1
        dev = torch.device("cuda", 0)
        up = lambda a: torch.from_numpy(a.view(np.uint8).reshape(-1).copy()).to(dev)  # noqa: E731
        outs = []
        for st in (plain, merged):
            st.mirror_many([(r, host[r], None) for r in receivers])
            scores = st.evaluate(pkts, words, codes)
            cap = st.select_capacity(n, k)
            d_sel = torch.zeros(cap, dtype=torch.int32, device=dev)
            d_count = torch.zeros(1, dtype=torch.int32, device=dev)
            d_oreqs = torch.zeros(cap * REQ_DTYPE.itemsize, dtype=torch.uint8, device=dev)
            d_osigs = torch.zeros(cap * 64, dtype=torch.uint8, device=dev)
            d_reqs = torch.zeros(2 * n * REQ_DTYPE.itemsize, dtype=torch.uint8, device=dev)
            d_sigs = torch.zeros(2 * n * 64, dtype=torch.uint8, device=dev)
            st.select_device(up(pkts).data_ptr(), n, up(scores).data_ptr(), k, d_reqs.data_ptr(), d_sigs.data_ptr(),
                             d_sel.data_ptr(), d_count.data_ptr(), d_oreqs.data_ptr(), d_osigs.data_ptr(),
                             torch.cuda.current_stream(dev).cuda_stream)
            torch.cuda.synchronize(dev)
            outs.append((scores, int(d_count.cpu()[0]), d_sel.cpu().numpy()))
        assert (outs[0][0] > 0).sum() > 16
        assert np.array_equal(outs[0][0], outs[1][0]) and outs[0][1] == outs[1][1] > 0
        assert np.array_equal(outs[0][2], outs[1][2])
        plain.close()
        merged.close()
    finally:
        e.close()
