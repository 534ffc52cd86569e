"""Scoring and selection of parsed packet slots on the GPU (hg_stores_*,
handel_amd/intake.py). The expected scores always come from
sigprocessing.Store._unsafe_evaluate (store.go:111-183, pinned by the
reference's TestStoreReplace numbers), the expected picks from read_todos'
rule (intake.select_slots, checked against read_todos in test_intake.py)."""

import random

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

HG_OK, HG_PKT_NO_IND, HG_ERR_LEVEL, HG_ERR_PKT_BITSET_SIZE = 0, 29, 3, 26

CLASSES = ("completed", "indiv_seen", "superset", "nobest_adds", "nobest_completes", "replace_adds",
           "replace_completes", "replace_zero", "indiv_one", "merge_adds", "merge_completes")


def _engine(nreg: int):
    import bench
    from handel_amd.engine import Engine

    e = Engine(device=0, flavor="go")
    assert not e.registry_load(e.keygen(bench.seeded_scalars(nreg, 77 + nreg))).any()
    return e


def _rand_bits(rng, size: int, density: float) -> int:
    bits = rng.random(size) < density
    return int.from_bytes(np.packbits(bits, bitorder="little").tobytes(), "little")


def _has_range(node: int, nreg: int, level: int):
    from handel_amd import partitioner as HP

    if node >= nreg or level < 1 or level > HP.log2_ceil(nreg):
        return None
    try:
        return HP.range_level(node, nreg, level)
    except HP.PartitionerError:
        return None


def _classify(store, sp) -> str:
    """Which outcome of store.go:111-183 a slot is (the branch taken, not the mark)."""
    size = store.size(sp.level)
    cur = store.m.get(sp.level)
    ivs = store.indiv_verified.get(sp.level, 0)
    if cur is not None and size == cur.cardinality():
        return "completed"
    if sp.individual() and (ivs >> sp.mapped_index) & 1:
        return "indiv_seen"
    if cur is not None and not sp.individual() and (sp.ms.bits & ~cur.bits) == 0:
        return "superset"
    wi = sp.ms.bits | ivs
    if cur is None:
        branch, total, added = "nobest", wi.bit_count(), wi.bit_count()
    elif sp.ms.bits & cur.bits:
        branch, total, added = "replace", wi.bit_count(), wi.bit_count() - cur.cardinality()
    else:
        branch, total = "merge", (wi | cur.bits).bit_count()
        added = total - cur.cardinality()
    if added <= 0:
        return "indiv_one" if sp.individual() else branch + "_zero"
    return branch + ("_completes" if total == size else "_adds")


def _expected_scores(nreg, host, pkts, slot_bits, codes, live):
    """The contract of hg_stores_evaluate with Store._unsafe_evaluate as the
    scorer: (scores, outcome class per slot or None)."""
    from handel_amd.sigprocessing import IncomingSig, MultiSig

    n = len(pkts)
    scores, classes = [], []
    for slot in range(2 * n):
        p = pkts[slot % n]
        score, cls = 0, None
        rng_ = _has_range(int(p["receiver"]), nreg, int(p["level"]))
        if codes[slot] != HG_OK or (live is not None and not live[slot]) or rng_ is None:
            score = 0
        elif int(p["receiver"]) not in host:
            score = -1
        else:
            lo, hi = rng_
            ind = slot >= n
            bits = slot_bits[slot]
            sp = IncomingSig(int(p["origin"]), int(p["level"]), MultiSig(hi - lo, bits, b""), ind=ind,
                             mapped_index=bits.bit_length() - 1 if ind else 0)
            store = host[int(p["receiver"])]
            score = store._unsafe_evaluate(sp)
            cls = _classify(store, sp)
        scores.append(score)
        classes.append(cls)
    return np.array(scores, dtype=np.int32), classes


def _slot_words(slot_bits, stride):
    out = np.zeros(len(slot_bits) * stride, dtype=np.uint64)
    for s, v in enumerate(slot_bits):
        if v:
            w = np.frombuffer(v.to_bytes(8 * stride, "little"), dtype="<u8")
            out[s * stride:(s + 1) * stride] = w
    return out


# ------------------------------------------------------------------ 1. reference vectors
def test_reference_vectors_store_replace():
    """store_test.go:136-195 TestStoreReplace at n = 8, node 1: the full
    signatures of levels 1, 2, 3 score 999990, 999980, 999970 on an empty
    store; the level-2 one scores 0 once it is the level's best."""
    from handel_amd.engine import PACKET_DTYPE
    from handel_amd.intake import DeviceStores
    from handel_amd.sigprocessing import IncomingSig, MultiSig, Store

    e = _engine(8)
    try:
        st = DeviceStores(e, [1], 16)
        assert st.stride == 1
        sizes = {1: 1, 2: 2, 3: 4}  # node 1: [0, 1), [2, 4), [4, 8)
        pkts = np.zeros(3, dtype=PACKET_DTYPE)
        for i, lv in enumerate((1, 2, 3)):
            pkts[i]["receiver"], pkts[i]["level"], pkts[i]["origin"] = 1, lv, 0
        words = np.zeros(6, dtype=np.uint64)
        words[:3] = [(1 << sizes[lv]) - 1 for lv in (1, 2, 3)]
        codes = np.array([0, 0, 0, HG_PKT_NO_IND, HG_PKT_NO_IND, HG_PKT_NO_IND], dtype=np.int32)
        assert list(st.evaluate(pkts, words, codes)) == [999990, 999980, 999970, 0, 0, 0]
        host = Store(1, 8, lambda a, b: a)
        sig2 = IncomingSig(2, 2, MultiSig(2, 3, bytes(64)))
        assert host.evaluate(sig2) == 999980
        host.store(sig2)
        st.mirror(1, host)
        assert host.evaluate(sig2) == 0
        assert list(st.evaluate(pkts, words, codes)) == [999990, 0, 999970, 0, 0, 0]
        best, indiv, has = st.read(1, 2)
        assert (int(best[0]), int(indiv[0]), has) == (3, 0, True)
        st.close()
    finally:
        e.close()


# ------------------------------------------------------------------ 2. randomised parity
def _parity_case(nreg: int):
    """Stores in every state and 1024 slots of every kind for an nreg-key
    registry: (receivers, host stores, pkts, slot bits, codes, live)."""
    from handel_amd import partitioner as HP
    from handel_amd.engine import PACKET_DTYPE
    from handel_amd.sigprocessing import MultiSig, Store

    rnd = random.Random(1000 + nreg)
    rng = np.random.default_rng(2000 + nreg)
    receivers = rnd.sample(range(nreg), min(nreg, 256))
    hosted = set(receivers)
    host = {}
    for r in receivers:
        s = Store(r, nreg, lambda a, b: a)
        for lv in s.levels:
            size = s.size(lv)
            state = rnd.choice(["none", "complete", 0.05, 0.5, 0.95])
            if state == "complete":
                s.m[lv] = MultiSig(size, (1 << size) - 1, b"")
            elif state != "none":
                s.m[lv] = MultiSig(size, _rand_bits(rng, size, state) | 1 << rnd.randrange(size), b"")
            s.indiv_verified[lv] = _rand_bits(rng, size, rnd.choice([0.0, 0.02, 0.3]))
        host[r] = s
    n = 512
    top = HP.log2_ceil(nreg)
    pkts = np.zeros(n, dtype=PACKET_DTYPE)
    slot_bits = [0] * (2 * n)
    codes = np.zeros(2 * n, dtype=np.int32)
    live = np.ones(2 * n, dtype=np.uint8)
    unhosted = [r for r in range(nreg) if r not in hosted]  # none at nreg = 200: every id is hosted there
    for i in range(n):
        r = rnd.choice(receivers)
        s = host[r]
        lv = rnd.choice(s.levels)
        odd = rnd.randrange(32)
        if odd == 0 and unhosted:
            r = rnd.choice(unhosted)
            lv = rnd.choice([l for l in range(1, top + 1) if _has_range(r, nreg, l)])
        elif odd == 1:  # a level outside the receiver's levels: 0, above the top, or an empty one
            empty = [l for l in range(1, top + 1) if _has_range(r, nreg, l) is None]
            lv = rnd.choice([0, top + 1, top + 7] + empty)
        pkts[i]["receiver"], pkts[i]["level"] = r, lv
        rg = _has_range(r, nreg, lv)
        lo, hi = rg if rg else (0, 64)
        size = hi - lo
        full = (1 << size) - 1
        cur = host[r].m.get(lv) if r in host else None
        best = cur.bits if cur is not None else 0
        kind = rnd.choice(["subset", "complement", "half", "full", "random", "random"])
        if kind == "subset":
            bits = best & _rand_bits(rng, size, 0.5)
        elif kind == "complement":
            bits = full & ~best
        elif kind == "half":
            bits = full & ~best & _rand_bits(rng, size, 0.5)
        elif kind == "full":
            bits = full
        else:
            bits = _rand_bits(rng, size, rnd.choice([0.05, 0.3, 0.7, 0.95]))
        slot_bits[i] = bits or 1 << rnd.randrange(size)
        pkts[i]["origin"] = lo + rnd.randrange(size)
        if rnd.random() < 0.6:  # the individual signature: one bit at the origin's index
            slot_bits[n + i] = 1 << (int(pkts[i]["origin"]) - lo)
        else:
            codes[n + i] = HG_PKT_NO_IND
        if odd == 2:
            codes[i] = codes[n + i] = HG_ERR_PKT_BITSET_SIZE
        elif odd == 3:
            live[i if rnd.random() < 0.5 else n + i] = 0
    return receivers, host, pkts, slot_bits, codes, live


@pytest.mark.parametrize("nreg", [200, 4000, 8200])
def test_scores_equal_unsafe_evaluate(nreg):
    """Strides 2, 32 and 128 words (a team far narrower than a wave, a
    half-wave team, the stride > 64 loop; level 12 of 4000 keys has 1952 ids:
    a ragged last word). All 2n scores through the device and the host entry
    point; every outcome class of unsafeEvaluate occurs at least 8 times."""
    import torch

    from handel_amd.intake import DeviceStores

    receivers, host, pkts, slot_bits, codes, live = _parity_case(nreg)
    want, classes = _expected_scores(nreg, host, pkts, slot_bits, codes, live)
    counts = {c: classes.count(c) for c in CLASSES}
    print("outcome classes", nreg, counts, "fixed", classes.count(None))
    assert min(counts.values()) >= 8, counts
    n = len(pkts)
    e = _engine(nreg)
    try:
        stride = e.packet_stride_words()
        assert stride == {200: 2, 4000: 32, 8200: 128}[nreg]
        st = DeviceStores(e, receivers, n)
        st.mirror_many([(r, host[r], None) for r in receivers])
        words = _slot_words(slot_bits, stride)
        got_host = st.evaluate(pkts, words, codes, live)
        bad = np.flatnonzero(got_host != want)
        assert len(bad) == 0, (bad[:8], got_host[bad[:8]], want[bad[:8]], [classes[i] for i in bad[:8]])
        dev = torch.device("cuda", 0)
        up = lambda a: torch.from_numpy(a.view(np.uint8).reshape(-1).copy()).to(dev)  # noqa: E731
        d_pkts, d_words, d_codes, d_live = up(pkts), up(words), up(codes), up(live)
        d_scores = torch.full((2 * n,), -7, dtype=torch.int32, device=dev)
        s = torch.cuda.current_stream(dev).cuda_stream
        st.evaluate_device(d_pkts.data_ptr(), n, stride, d_words.data_ptr(), d_codes.data_ptr(), d_live.data_ptr(),
                           d_scores.data_ptr(), s)
        torch.cuda.synchronize(dev)
        assert np.array_equal(d_scores.cpu().numpy(), want)
        # without a live mask the cleared slots are scored like the others
        want_all, _ = _expected_scores(nreg, host, pkts, slot_bits, codes, None)
        assert np.array_equal(st.evaluate(pkts, words, codes), want_all)
        st.close()
    finally:
        e.close()


# ------------------------------------------------------------------ 3. update / read
def test_update_read_round_trip_and_refusals():
    from handel_amd import partitioner as HP
    from handel_amd._lib import HG_STORE_HAS_BEST, HandelGPUError
    from handel_amd.engine import PACKET_DTYPE, STORE_UPDATE_DTYPE, Stores

    import bench

    nreg = 200
    e = _engine(nreg)
    try:
        with pytest.raises(HandelGPUError):
            Stores(e, [3, 9, 3], 8)  # duplicate receivers
        with pytest.raises(HandelGPUError):
            Stores(e, [3, nreg], 8)  # not a registry id
        receivers = [5, 130, 199]
        st = Stores(e, receivers, 8)
        stride = st.stride
        rng = np.random.default_rng(3)
        ups, words, want = [], [], {}
        for r in receivers:
            for lv, lo, hi in HP.level_sizes(r, nreg):
                size, lw = hi - lo, (hi - lo + 63) // 64
                has = bool(rng.integers(2))
                raw = rng.integers(0, 2**63, size=2 * lw, dtype=np.uint64) * np.uint64(2) + np.uint64(1)  # bits everywhere
                ups.append((r, lv, HG_STORE_HAS_BEST if has else 0, len(words), len(words) + lw))
                words += list(raw)
                mask = (1 << size) - 1
                val = lambda ws: sum(int(x) << (64 * j) for j, x in enumerate(ws)) & mask  # noqa: E731
                want[(r, lv)] = (val(raw[:lw]) if has else 0, val(raw[lw:]), has)
        st.update(np.array(ups, dtype=STORE_UPDATE_DTYPE), np.array(words, dtype=np.uint64))
        for (r, lv), (b, iv, has) in want.items():
            best, indiv, got_has = st.read(r, lv)
            assert len(best) == stride
            val = lambda ws: sum(int(x) << (64 * j) for j, x in enumerate(ws))  # noqa: E731
            assert (val(best), val(indiv), got_has) == (b, iv, has), (r, lv)  # bits at or above the size cleared
        one = np.array(ups[:1] * 2, dtype=STORE_UPDATE_DTYPE)
        with pytest.raises(HandelGPUError):  # a (receiver, level) named twice
            st.update(one, np.array(words, dtype=np.uint64))
        with pytest.raises(HandelGPUError):  # words outside the array
            st.update(one[:1], np.zeros(1, dtype=np.uint64))
        with pytest.raises(HandelGPUError):  # not a hosted receiver
            st.read(6, 1)
        # a second registry load: the stores belong to the first one
        assert not e.registry_load(e.keygen(bench.seeded_scalars(nreg, 5))).any()
        pkts = np.zeros(1, dtype=PACKET_DTYPE)
        z = np.zeros(2 * stride, dtype=np.uint64)
        for call in (lambda: st.update(one[:1], np.array(words, dtype=np.uint64)),
                     lambda: st.read(5, 1),
                     lambda: st.evaluate(pkts, z, np.zeros(2, dtype=np.int32)),
                     lambda: st.evaluate_device(z.ctypes.data, 1, stride, z.ctypes.data, z.ctypes.data, 0,
                                                z.ctypes.data),
                     lambda: st.select_device(z.ctypes.data, 1, z.ctypes.data, 1, z.ctypes.data, z.ctypes.data,
                                              z.ctypes.data, z.ctypes.data, z.ctypes.data, z.ctypes.data)):
            with pytest.raises(HandelGPUError):  # refused before any pointer is used
                call()
        st.close()
        st2 = Stores(e, receivers, 8)  # a new set on the new registry works
        assert st2.read(5, 1)[2] is False
        st2.close()
    finally:
        e.close()


# ------------------------------------------------------------------ 4. selection
@pytest.fixture(scope="module")
def select_case():
    """N = 200, 16 stores, 600 packets, scores with many ties."""
    from handel_amd.engine import PACKET_DTYPE, REQ_DTYPE

    nreg, n = 200, 600
    rnd = random.Random(44)
    rng = np.random.default_rng(44)
    receivers = rnd.sample(range(nreg), 16)
    pkts = np.zeros(n, dtype=PACKET_DTYPE)
    others = [r for r in range(nreg) if r not in receivers]
    for i in range(n):
        pkts[i]["receiver"] = rnd.choice(receivers) if rnd.random() < 0.9 else rnd.choice(others + [nreg + 5])
    scores = np.array([rnd.choice([-1, 0, 0, 1, 1, 1, 99760, 99760, 99770, 999980, rnd.randrange(1, 6)])
                       for _ in range(2 * n)], dtype=np.int32)
    reqs = np.frombuffer(rng.bytes(2 * n * REQ_DTYPE.itemsize), dtype=REQ_DTYPE).copy()
    sigs = np.frombuffer(rng.bytes(2 * n * 64), dtype=np.uint8).copy()
    e = _engine(nreg)
    yield e, receivers, pkts, scores, reqs, sigs
    e.close()


@pytest.mark.parametrize("k", [1, 3, 64])
def test_selection_equals_read_todos(select_case, k):
    import torch

    from handel_amd.engine import REQ_DTYPE
    from handel_amd.intake import DeviceStores, select_slots

    e, receivers, pkts, scores, reqs, sigs = select_case
    n = len(pkts)
    index = {r: i for i, r in enumerate(receivers)}
    store_of_slot = [index.get(int(pkts[s % n]["receiver"]), -1) for s in range(2 * n)]
    want, _ = select_slots(store_of_slot, scores, n, k, len(receivers))
    assert 0 < len(want) <= 16 * k
    st = DeviceStores(e, receivers, n)
    try:
        cap = st.select_capacity(n, k)
        assert cap == min(2 * n, 16 * k)
        dev = torch.device("cuda", 0)
        up = lambda a: torch.from_numpy(a.view(np.uint8).reshape(-1).copy()).to(dev)  # noqa: E731
        d_pkts, d_scores, d_reqs, d_sigs = up(pkts), up(scores), up(reqs), up(sigs)
        s = torch.cuda.current_stream(dev).cuda_stream
        runs = []
        for _ in range(2):
            d_sel = torch.full((cap,), 7, dtype=torch.int32, device=dev)
            d_count = torch.full((1,), -1, dtype=torch.int32, device=dev)
            d_oreqs = torch.full((cap * REQ_DTYPE.itemsize,), 0x55, dtype=torch.uint8, device=dev)
            d_osigs = torch.full((cap * 64,), 0x55, dtype=torch.uint8, device=dev)
            st.select_device(d_pkts.data_ptr(), n, d_scores.data_ptr(), k, d_reqs.data_ptr(), d_sigs.data_ptr(),
                             d_sel.data_ptr(), d_count.data_ptr(), d_oreqs.data_ptr(), d_osigs.data_ptr(), s)
            torch.cuda.synchronize(dev)
            runs.append((int(d_count.cpu()[0]), d_sel.cpu().numpy().view(np.uint32),
                         np.frombuffer(d_oreqs.cpu().numpy().tobytes(), dtype=REQ_DTYPE),
                         d_osigs.cpu().numpy().reshape(cap, 64)))
        count, sel, oreqs, osigs = runs[0]
        assert count == len(want) and list(sel[:count]) == want
        assert np.array_equal(oreqs[:count], reqs[want])
        assert np.array_equal(osigs[:count], sigs.reshape(2 * n, 64)[want])
        # the filler: a request that fails the level check and a zero signature
        assert (sel[count:] == 0xFFFFFFFF).all() and not osigs[count:].any()
        assert (oreqs[count:]["bitlen"] == 0).all() and (oreqs[count:]["level_size"] == 1).all()
        assert (oreqs[count:]["offset"] == 0).all() and (oreqs[count:]["word_offset"] == 0).all()
        for a, b in zip(runs[0], runs[1]):
            assert np.array_equal(a, b)
    finally:
        st.close()


# ------------------------------------------------------------------ 5. the chain in HBM
def test_chain_parse_evaluate_select_verify():
    """test_device_parse_feeds_verification's batch through parse -> evaluate
    -> select (k large) -> verify on device arrays: a third of the packets
    find a superset as their level's best and are never verified; the others'
    codes are the verdicts the batch was built with."""
    import torch

    import bench
    from handel_amd import partitioner as HP
    from handel_amd.engine import Engine, REQ_DTYPE
    from handel_amd.intake import DeviceStores, select_slots
    from handel_amd.packets import Packet, pack_packets
    from handel_amd.sigprocessing import MultiSig, Store, bits_to_int

    e = Engine(device=0, flavor="go")
    try:
        assert e.set_message(bench.LIB_MESSAGE) == 0
        n_reg, n = 4000, 512
        reqs, words, sigs, expect, _, _ = bench.make_aggregate_batch(e, n_reg, n, seed=91)
        rnd = random.Random(5)
        pkts, recv, host, slot_bits = [], [], {}, []
        for i, r in enumerate(reqs):
            lo, size = int(r["offset"]), int(r["level_size"])
            nw = (size + 63) // 64
            bits = HP.words_to_bits(words[int(r["word_offset"]):int(r["word_offset"]) + nw], size)
            rv, lv = next((lo ^ (1 << k), k + 1) for k in range(12)
                          if _has_range(lo ^ (1 << k), n_reg, k + 1) == (lo, lo + size))
            pkts.append(Packet(rnd.randrange(lo, lo + size), lv, HP.multisig_marshal(bits, sigs[64 * i:64 * i + 64])))
            recv.append(rv)
            slot_bits.append(bits_to_int(bits))
            store = host.setdefault(rv, Store(rv, n_reg, lambda a, b: a))
            if i % 3 == 0:  # the level's best covers this packet, one more id, and what it covered before
                before = store.m[lv].bits if lv in store.m else 0
                store.m[lv] = MultiSig(size, before | slot_bits[i] | 1 << rnd.randrange(size), b"")
        receivers = sorted(host)
        pool, recs = pack_packets(pkts, recv)
        pcodes_want = np.array([HG_OK] * n + [HG_PKT_NO_IND] * n, dtype=np.int32)
        want_scores, _ = _expected_scores(n_reg, host, recs, slot_bits + [0] * n, pcodes_want, None)
        index = {r: j for j, r in enumerate(receivers)}
        want_sel, _ = select_slots([index[r] for r in recv] * 2, want_scores, n, 2 * n, len(receivers))
        assert n // 3 <= n - len(want_sel) and len(want_sel) >= n // 3 and all(s < n for s in want_sel)
        assert all(want_scores[i] == 0 for i in range(0, n, 3))
        st = DeviceStores(e, receivers, n)
        st.mirror_many([(r, host[r], None) for r in receivers])
        stride = e.packet_stride_words()
        cap = st.select_capacity(n, 2 * n)
        assert cap == 2 * n
        dev = torch.device("cuda", 0)
        d_pool = torch.from_numpy(np.frombuffer(pool, dtype=np.uint8).copy()).to(dev)
        d_pkts = torch.from_numpy(recs.view(np.uint8).copy()).to(dev)
        d_reqs = torch.zeros(2 * n * REQ_DTYPE.itemsize, dtype=torch.uint8, device=dev)
        d_words = torch.zeros(2 * n * stride, dtype=torch.int64, device=dev)
        d_sigs = torch.zeros(2 * n * 64, dtype=torch.uint8, device=dev)
        d_pcodes = torch.full((2 * n,), -1, dtype=torch.int32, device=dev)
        d_scores = torch.full((2 * n,), -7, dtype=torch.int32, device=dev)
        d_sel = torch.zeros(cap, dtype=torch.int32, device=dev)
        d_count = torch.zeros(1, dtype=torch.int32, device=dev)
        d_oreqs = torch.zeros(cap * REQ_DTYPE.itemsize, dtype=torch.uint8, device=dev)
        d_osigs = torch.zeros(cap * 64, dtype=torch.uint8, device=dev)
        d_codes = torch.full((cap,), -1, dtype=torch.int32, device=dev)
        s = torch.cuda.current_stream(dev).cuda_stream
        e.parse_packets_device(d_pool.data_ptr(), len(pool), d_pkts.data_ptr(), n, stride, d_reqs.data_ptr(),
                               d_words.data_ptr(), d_sigs.data_ptr(), d_pcodes.data_ptr(), s)
        st.evaluate_device(d_pkts.data_ptr(), n, stride, d_words.data_ptr(), d_pcodes.data_ptr(), 0,
                           d_scores.data_ptr(), s)
        st.select_device(d_pkts.data_ptr(), n, d_scores.data_ptr(), 2 * n, d_reqs.data_ptr(), d_sigs.data_ptr(),
                         d_sel.data_ptr(), d_count.data_ptr(), d_oreqs.data_ptr(), d_osigs.data_ptr(), s)
        # the whole capacity, without reading the count back first
        e.verify_aggregate_device(d_oreqs.data_ptr(), cap, d_words.data_ptr(), d_osigs.data_ptr(), d_codes.data_ptr(),
                                  stream=s)
        torch.cuda.synchronize(dev)
        assert np.array_equal(d_pcodes.cpu().numpy(), pcodes_want)
        assert np.array_equal(d_scores.cpu().numpy(), want_scores)
        count = int(d_count.cpu()[0])
        sel = d_sel.cpu().numpy()[:count].tolist()
        assert sel == want_sel  # exactly the packets no best dominates
        codes = d_codes.cpu().numpy()
        assert np.array_equal(codes[:count], expect[sel])  # tampered ones included
        assert expect[sel].any() and not expect[sel].all()
        assert (codes[count:] == HG_ERR_LEVEL).all()  # the filler
        st.close()
    finally:
        e.close()


# ------------------------------------------------------------------ 6. DeviceIntake against the host pipeline
def test_device_intake_equals_host_pipeline():
    """N = 64, 8 receivers, three steps of about 100 packets with real
    signatures (1/8 of them invalid): DeviceIntake picks, publishes and stores
    what one read_todos(batch = k) per receiver per step with EvaluatorStore on
    a host Store does."""
    import bench
    from handel_amd import partitioner as HP
    from handel_amd.engine import Engine, REQ_DTYPE
    from handel_amd.intake import DeviceIntake
    from handel_amd.packets import Packet
    from handel_amd.sigprocessing import (BatchedEvaluatorProcessing, EvaluatorStore, IncomingSig, MultiSig, Store,
                                          bits_to_int, int_to_words)

    nreg, k = 64, 4
    e = Engine(device=0, flavor="go")
    try:
        assert e.set_message(bench.LIB_MESSAGE) == 0
        kb = bench.seeded_scalars(nreg, 321)
        assert not e.registry_load(e.keygen(kb)).any()
        ks = [int.from_bytes(kb[32 * i:32 * i + 32], "big") for i in range(nreg)]
        rnd = random.Random(66)
        receivers = rnd.sample(range(nreg), 8)
        combine = lambda a, b: e.combine_g1(a, b)[0]  # noqa: E731

        def make_step(count):
            """packets, their receivers, and (multisig, individual) IncomingSigs as the parse yields them"""
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
                # an invalid signature: a valid point signed by another scalar
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

        host = {r: Store(r, nreg, combine) for r in receivers}
        procs = {r: BatchedEvaluatorProcessing(lambda sps, r=r: host_verify(r, sps), EvaluatorStore(host[r]), batch=k)
                 for r in receivers}
        di = DeviceIntake(e, receivers, k, max_packets=1024)
        key = lambda sp: (sp.origin, sp.level, sp.ind, sp.ms.bits, sp.ms.sig)  # noqa: E731
        published_host, published_dev, invalid = [], [], 0
        for step in range(3):
            pkts, recv, incoming = make_step(100)
            results, unselected = di.step(pkts, recv)
            for r, sps in zip(recv, incoming):
                for sp in sps:
                    procs[r].add(sp)
            want = []
            for r in receivers:  # the device's output is grouped by store in this order
                if not procs[r].todos:
                    continue
                done, best = procs[r].read_todos()
                assert not done
                for sp, err in zip(best, host_verify(r, best) if best else []):
                    want.append((r, key(sp), err))
                    if err is None:
                        host[r].store(sp)
                        published_host.append((r, key(sp)))
            got = [(r, key(sp), err) for r, sp, err in results]
            assert got == want, step  # the same picks with the same verdicts, in the same order
            published_dev += [(r, key(sp)) for r, sp, err in results if err is None]
            invalid += sum(err is not None for _, _, err in results)
            assert len(unselected) == sum(len(procs[r].todos) for r in receivers) == len(di.pending)
        assert published_dev == published_host and len(published_dev) > 20 and invalid > 0
        assert di.pending  # k = 4 leaves a queue behind: the later steps re-present it
        for r in receivers:
            for lv, lo, hi in HP.level_sizes(r, nreg):
                a, b = host[r].m.get(lv), di.host[r].m.get(lv)
                assert (a is None) == (b is None), (r, lv)
                best, indiv, has = di.stores.read(r, lv)
                assert has == (a is not None)
                if a is not None:
                    assert (a.bits, a.sig) == (b.bits, b.sig), (r, lv)
                    assert int(best[0]) == a.bits
                assert int(indiv[0]) == host[r].indiv_verified[lv] == di.host[r].indiv_verified[lv]
        di.close()
    finally:
        e.close()
