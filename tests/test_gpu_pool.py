"""The standing queue on the GPU (hg_stores_pool_*, handel_amd/csrc/hg_pool.hip)
against intake.PoolModel (held to read_todos in tests/test_pool_host.py), with
Store._unsafe_evaluate as the scorer; the step's output as a parsed batch; and
DeviceIntake(device_pool=True) against DeviceIntake(device_pool=False)."""

import random

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

HG_OK, HG_PKT_NO_IND, HG_ERR_LEVEL, HG_ERR_PKT_BITSET_SIZE = 0, 29, 3, 26
HG_PKT_HAS_IND = 1
STRIDES = {200: 2, 4000: 32, 8200: 128}
POOL_SLOTS, MAX_PACKETS, N_STEP = 512, 256, 48


def _engine(nreg: int):
    import bench
    from handel_amd.engine import Engine

    e = Engine(device=0, flavor="go")
    assert not e.registry_load(e.keygen(bench.seeded_scalars(nreg, 77 + nreg))).any()
    return e


@pytest.fixture(scope="module", params=[200, 4000, 8200])
def sized_engine(request):
    e = _engine(request.param)
    yield request.param, e
    e.close()


def _has_range(node: int, nreg: int, level: int):
    from handel_amd import partitioner as HP

    if node >= nreg or level < 1 or level > HP.log2_ceil(nreg):
        return None
    try:
        return HP.range_level(node, nreg, level)
    except HP.PartitionerError:
        return None


def _rand_bits(rng, size: int, density: float) -> int:
    bits = rng.random(size) < density
    return int.from_bytes(np.packbits(bits, bitorder="little").tobytes(), "little")


def _slot_words(slot_bits, stride):
    out = np.zeros(len(slot_bits) * stride, dtype=np.uint64)
    for s, v in enumerate(slot_bits):
        if v:
            out[s * stride:(s + 1) * stride] = np.frombuffer(v.to_bytes(8 * stride, "little"), dtype="<u8")
    return out


def _receivers(nreg, rnd):
    """three hosted receivers and one without a store"""
    ids = rnd.sample(range(nreg), 4)
    return ids[:3], ids[3]


def _make_step(nreg, hosted, unhosted, rnd, rng, n=N_STEP):
    """The outputs of a parse of n synthetic packets: (pkts, reqs, slot bits,
    sigs, codes, live, reasons). Every packet arrives two or three times, so
    equal marks are common. reasons counts why slots are not admitted."""
    from handel_amd import partitioner as HP
    from handel_amd.engine import PACKET_DTYPE, REQ_DTYPE

    top = HP.log2_ceil(nreg)
    base = []
    while len(base) < n:
        odd = rnd.randrange(12)
        r = unhosted if odd == 0 else rnd.choice(hosted)
        levels = [lv for lv in range(1, top + 1) if _has_range(r, nreg, lv)]
        lv = rnd.choice([0, top + 1, top + 5]) if odd == 1 else rnd.choice(levels)
        rg = _has_range(r, nreg, lv)
        lo, hi = rg if rg else (0, 64)
        size = hi - lo
        origin = lo + rnd.randrange(size)
        bits = _rand_bits(rng, size, rnd.choice([0.1, 0.5, 0.9])) | 1 << (origin - lo)
        pkt = (r, lv, lo, size, origin, bits, rnd.random() < 0.6, odd, rnd.random() < 0.5)
        base += [pkt] * rnd.choice([2, 3])
    base = base[:n]
    rnd.shuffle(base)
    pkts = np.zeros(n, dtype=PACKET_DTYPE)
    reqs = np.zeros(2 * n, dtype=REQ_DTYPE)
    slot_bits = [0] * (2 * n)
    codes = np.zeros(2 * n, dtype=np.int32)
    live = np.ones(2 * n, dtype=np.uint8)
    sigs = np.frombuffer(rng.bytes(2 * n * 64), dtype=np.uint8).copy()
    reasons = dict(bad_code=0, no_ind=0, live0=0, no_range=0, no_store=0)
    for i, (r, lv, lo, size, origin, bits, has_ind, odd, first) in enumerate(base):
        pkts[i] = (origin, r, lv, HG_PKT_HAS_IND if has_ind else 0, 7 * i, 11, 13 * i, 64 if has_ind else 0)
        reqs[i] = reqs[n + i] = (lo, size, size, 0)
        slot_bits[i] = bits
        if has_ind:
            slot_bits[n + i] = 1 << (origin - lo)
        else:
            codes[n + i] = HG_PKT_NO_IND
            reasons["no_ind"] += 1
        if odd == 2:
            codes[i] = codes[n + i] = HG_ERR_PKT_BITSET_SIZE
            reasons["bad_code"] += 2
        elif odd in (3, 4):
            live[i if first else n + i] = 0
            reasons["live0"] += 1
        elif odd == 1:
            reasons["no_range"] += 1 + has_ind
        elif odd == 0:
            reasons["no_store"] += 1 + has_ind
    for s in range(2 * n):
        reqs[s]["word_offset"] = s  # the pool recomputes it
    return pkts, reqs, slot_bits, sigs, codes, live, reasons


def _admit(model, nreg, pkts, reqs, slot_bits, sigs, codes, live):
    """hg_stores_pool_append_device's rule on the model, in Handel's queue order"""
    n = len(pkts)
    for q in range(2 * n):
        slot = (q >> 1) + (n if q & 1 else 0)
        p = pkts[q >> 1]
        if codes[slot] != HG_OK or not live[slot]:
            continue
        if _has_range(int(p["receiver"]), nreg, int(p["level"])) is None:
            continue
        item = (int(p["origin"]), int(p["receiver"]), int(p["level"]), int(p["flags"]), slot >= n,
                tuple(int(reqs[slot][f]) for f in ("offset", "bitlen", "level_size")), slot_bits[slot],
                sigs[64 * slot:64 * slot + 64].tobytes())
        model.append(int(p["receiver"]), item)


def _mark(host, r, item):
    from handel_amd.sigprocessing import IncomingSig, MultiSig

    origin, _, level, _, ind, (lo, _, size), bits, _ = item
    sp = IncomingSig(origin, level, MultiSig(size, bits, b""), ind=ind, mapped_index=origin - lo if ind else 0)
    return host[r]._unsafe_evaluate(sp)


def _mutate(host, hosted, picks, rnd):
    """The picks are stored, and one more level per receiver completes."""
    from handel_amd.sigprocessing import IncomingSig, MultiSig

    for r, item, _ in picks:
        origin, _, level, _, ind, (lo, _, size), bits, _ = item
        host[r].store(IncomingSig(origin, level, MultiSig(size, bits, b""), ind=ind,
                                  mapped_index=origin - lo if ind else 0))
    for r in hosted:
        lv = rnd.choice(host[r].levels)
        size = host[r].size(lv)
        host[r].m[lv] = MultiSig(size, (1 << size) - 1, b"")


class _Device:
    """the pool under test and the arrays of one step"""

    def __init__(self, e, hosted):
        import torch

        from handel_amd.engine import Pool
        from handel_amd.intake import DeviceStores

        self.torch, self.e = torch, e
        self.dev = torch.device("cuda", 0)
        self.st = DeviceStores(e, hosted, MAX_PACKETS)
        self.pool = Pool(self.st, POOL_SLOTS)
        self.stride = self.st.stride
        self.s = torch.cuda.current_stream(self.dev).cuda_stream

    def close(self):
        self.pool.close()
        self.st.close()

    def up(self, a):
        return self.torch.from_numpy(np.ascontiguousarray(a).view(np.uint8).reshape(-1).copy()).to(self.dev)

    def append(self, pool, pkts, reqs, slot_bits, sigs, codes, live):
        keep = [self.up(pkts), self.up(reqs), self.up(_slot_words(slot_bits, self.stride)), self.up(sigs),
                self.up(codes), self.up(live)]
        pool.append_device(keep[0].data_ptr(), len(pkts), self.stride, keep[1].data_ptr(), keep[2].data_ptr(),
                           keep[3].data_ptr(), keep[4].data_ptr(), keep[5].data_ptr(), self.s)
        self.torch.cuda.synchronize(self.dev)

    def step(self, pool, k):
        """(cap, count, sel, pkts, reqs, words[2cap, stride], sigs[2cap, 64], marks, device tensors)"""
        from handel_amd.engine import PACKET_DTYPE, REQ_DTYPE

        torch, dev, stride = self.torch, self.dev, self.stride
        cap = pool.select_capacity(k)
        fill = lambda nbytes: torch.full((nbytes,), 0x55, dtype=torch.uint8, device=dev)  # noqa: E731
        t = dict(pkts=fill(cap * PACKET_DTYPE.itemsize), sel=fill(4 * cap), count=fill(4),
                 reqs=fill(cap * REQ_DTYPE.itemsize), words=fill(2 * cap * stride * 8), sigs=fill(2 * cap * 64),
                 marks=fill(4 * cap))
        pool.step_device(k, cap, t["pkts"].data_ptr(), t["sel"].data_ptr(), t["count"].data_ptr(),
                         t["reqs"].data_ptr(), t["words"].data_ptr(), t["sigs"].data_ptr(), t["marks"].data_ptr(),
                         self.s)
        torch.cuda.synchronize(dev)
        host = {name: v.cpu().numpy() for name, v in t.items()}
        return (cap, int(host["count"].view(np.uint32)[0]), host["sel"].view(np.uint32),
                host["pkts"].view(PACKET_DTYPE), host["reqs"].view(REQ_DTYPE),
                host["words"].view(np.uint64).reshape(2 * cap, stride), host["sigs"].reshape(2 * cap, 64),
                host["marks"].view(np.int32), t)


def _check_step(out, stride, picks):
    """the step's output against the model's picks, filler included"""
    cap, count, sel, opkts, oreqs, owords, osigs, omarks, _ = out
    assert count == len(picks) <= cap
    for e, (r, item, mark) in enumerate(picks):
        origin, recv, level, flags, ind, (lo, bitlen, size), bits, sig = item
        slot = cap + e if ind else e
        assert sel[e] == slot, e
        assert tuple(opkts[e]) == (origin, recv, level, flags, 0, 0, 0, 0), e
        assert tuple(oreqs[e]) == (lo, bitlen, size, slot * stride), e
        assert int.from_bytes(owords[slot].astype("<u8").tobytes(), "little") == bits, e
        assert osigs[e].tobytes() == sig, e
        if ind:
            assert osigs[slot].tobytes() == sig, e
        assert omarks[e] == mark, e
    assert (sel[count:] == 0xFFFFFFFF).all() and not osigs[count:cap].any() and not omarks[count:].any()
    assert not opkts[count:].view(np.uint8).any()
    f = oreqs[count:]
    assert (f["offset"] == 0).all() and (f["bitlen"] == 0).all() and (f["level_size"] == 1).all()
    assert (f["word_offset"] == 0).all()


def _drive(nreg, k, e=None, seed=901):
    """Four steps of the model and, with an engine, of the pool in lockstep.
    Returns the fixture's statistics."""
    from handel_amd.intake import PoolModel
    from handel_amd.sigprocessing import Store

    rnd = random.Random(seed + nreg)
    rng = np.random.default_rng(seed + nreg)
    hosted, unhosted = _receivers(nreg, rnd)
    host = {r: Store(r, nreg, lambda a, b: a) for r in hosted}
    model = PoolModel(hosted)
    d = _Device(e, hosted) if e is not None else None
    stats = dict(bad_code=0, no_ind=0, live0=0, no_range=0, no_store=0, picked=0)
    try:
        if d is not None:
            assert d.stride == STRIDES[nreg]
        for step in range(4):
            pkts, reqs, slot_bits, sigs, codes, live, reasons = _make_step(nreg, hosted, unhosted, rnd, rng)
            for name, v in reasons.items():
                stats[name] += v
            _admit(model, nreg, pkts, reqs, slot_bits, sigs, codes, live)
            if d is not None:
                d.append(d.pool, pkts, reqs, slot_bits, sigs, codes, live)
                assert d.pool.count() == model.count(), step
            picks = model.step(k, lambda r, item: _mark(host, r, item))
            stats["picked"] += len(picks)
            if d is not None:
                _check_step(d.step(d.pool, k), d.stride, picks)
                assert d.pool.count() == model.count(), step
                for r in hosted:
                    p, ind, marks = d.pool.read(r)
                    got = [(int(a["origin"]), int(a["receiver"]), int(a["level"]), int(a["flags"]), bool(b), int(c))
                           for a, b, c in zip(p, ind, marks)]
                    want = [(it[0], it[1], it[2], it[3], it[4], mk) for it, mk in model.queue(r)]
                    assert got == want, (step, r)
                    assert not any(int(a[f]) for a in p for f in ("ms_off", "ms_len", "ind_off", "ind_len"))
            _mutate(host, hosted, picks, rnd)
            if d is not None:
                d.st.mirror_many([(r, host[r], None) for r in hosted])
    finally:
        if d is not None:
            d.close()
    stats["dropped"], stats["disordered"], stats["left"] = model.dropped, model.disordered, model.count()
    return stats


@pytest.mark.parametrize("k", [1, 3, 64])
def test_pool_equals_model(sized_engine, k):
    """N = 200, 4000, 8200 (strides 2, 32, 128), three receivers and one
    without a store, four steps of 48 synthetic packets with tied marks, the
    stores changing between steps. After every step the picks (slots, records,
    requests, words, signatures, marks), the filler, every receiver's queue
    read back and the count equal the model's. Every reason for not being
    admitted and for leaving occurs at least 8 times."""
    nreg, e = sized_engine
    stats = _drive(nreg, k, e)
    print("pool fixture", nreg, k, stats)
    for name in ("bad_code", "no_ind", "live0", "no_range", "no_store", "picked", "dropped"):
        assert stats[name] >= 8, (name, stats)
    if k < 64:
        assert stats["disordered"] >= 8 and stats["left"] > 0, stats


def test_step_output_is_a_parsed_batch(sized_engine):
    """hg_stores_evaluate_device on the step's (packets, capacity, words), the
    stores unchanged, gives the marks the step reported for the picks."""
    from handel_amd.intake import PoolModel
    from handel_amd.sigprocessing import MultiSig, Store

    nreg, e = sized_engine
    rnd = random.Random(31 + nreg)
    rng = np.random.default_rng(31 + nreg)
    hosted, unhosted = _receivers(nreg, rnd)
    host = {r: Store(r, nreg, lambda a, b: a) for r in hosted}
    for r in hosted:  # stores in mixed states
        for lv in host[r].levels:
            size = host[r].size(lv)
            if rnd.random() < 0.6:
                host[r].m[lv] = MultiSig(size, _rand_bits(rng, size, 0.3) | 1, b"")
            host[r].indiv_verified[lv] = _rand_bits(rng, size, 0.05)
    d = _Device(e, hosted)
    try:
        d.st.mirror_many([(r, host[r], None) for r in hosted])
        model = PoolModel(hosted)
        for _ in range(2):
            args = _make_step(nreg, hosted, unhosted, rnd, rng)[:6]
            _admit(model, nreg, *args)
            d.append(d.pool, *args)
        k = 16
        picks = model.step(k, lambda r, item: _mark(host, r, item))
        out = d.step(d.pool, k)
        _check_step(out, d.stride, picks)
        cap, count, sel, _, _, _, _, omarks, t = out
        assert count >= 24
        codes = np.full(2 * cap, HG_PKT_NO_IND, dtype=np.int32)
        codes[sel[:count]] = HG_OK
        d_codes = d.up(codes)
        d_scores = d.torch.full((2 * cap,), -7, dtype=d.torch.int32, device=d.dev)
        d.st.evaluate_device(t["pkts"].data_ptr(), cap, d.stride, t["words"].data_ptr(), d_codes.data_ptr(), 0,
                             d_scores.data_ptr(), d.s)
        d.torch.cuda.synchronize(d.dev)
        scores = d_scores.cpu().numpy()
        assert np.array_equal(scores[sel[:count]], omarks[:count]) and (omarks[:count] > 0).all()
        rest = np.ones(2 * cap, dtype=bool)
        rest[sel[:count]] = False
        assert not scores[rest].any()
    finally:
        d.close()


@pytest.mark.parametrize("merge", [False, True], ids=["host_store", "device_merge"])
def test_pooled_intake_equals_unpooled(merge):
    """test_device_intake_equals_host_pipeline's setting (N = 64, 8 receivers,
    k = 4, three steps of about 100 packets with real signatures, 1/8
    invalid): DeviceIntake(device_pool=True) gives the results, verdicts and
    order of DeviceIntake(device_pool=False) every step, the same changed
    levels and in the end the same stores, having uploaded the new packets
    alone."""
    import bench
    from handel_amd import partitioner as HP
    from handel_amd.engine import Engine
    from handel_amd.intake import DeviceIntake
    from handel_amd.packets import Packet

    nreg, k = 64, 4
    e = Engine(device=0, flavor="go")
    try:
        assert e.set_message(bench.LIB_MESSAGE) == 0
        kb = bench.seeded_scalars(nreg, 321)
        assert not e.registry_load(e.keygen(kb)).any()
        ks = [int.from_bytes(kb[32 * i:32 * i + 32], "big") for i in range(nreg)]
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
                metas.append((r, lv, bits, origin, has_ind))
            sg = e.sign(bytes(scalars))
            pkts, recv = [], []
            for i, (r, lv, bits, origin, has_ind) in enumerate(metas):
                ms_sig, ind_sig = sg[128 * i:128 * i + 64], sg[128 * i + 64:128 * i + 128]
                pkts.append(Packet(origin, lv, HP.multisig_marshal(bits, ms_sig), ind_sig if has_ind else None))
                recv.append(r)
            return pkts, recv

        ref = DeviceIntake(e, receivers, k, max_packets=1024, device_merge=merge)
        pooled = DeviceIntake(e, receivers, k, max_packets=1024, device_merge=merge, device_pool=True)
        own = e.sign(b"".join(kb[32 * r:32 * r + 32] for r in receivers))
        for j, r in enumerate(receivers):
            ref.set_own(r, own[64 * j:64 * j + 64])
            pooled.set_own(r, own[64 * j:64 * j + 64])
        key = lambda sp: (sp.origin, sp.level, sp.ind, sp.mapped_index, sp.ms.bitlen, sp.ms.bits, sp.ms.sig)  # noqa: E731
        invalid = 0
        for step in range(3):
            pkts, recv = make_step(100)
            want, unselected = ref.step(pkts, recv)
            got, left = pooled.step(pkts, recv)
            assert [(r, key(sp), err) for r, sp, err in got] == [(r, key(sp), err) for r, sp, err in want], step
            assert len(want) > 0
            invalid += sum(err is not None for _, _, err in want)
            assert pooled.last_uploaded == len(pkts) and not pooled.pending
            assert left == len(unselected) == len(ref.pending) and left > 0, step
            assert sum(len(pooled.pending_view(r)) for r in receivers) == left
            assert pooled.last_changed == ref.last_changed and pooled.last_results == ref.last_results
            if merge:
                assert ref.last_changed
        assert invalid > 0
        val = lambda m: None if m is None else (m.bitlen, m.bits, m.sig)  # noqa: E731
        for r in receivers:
            assert val(pooled.full_signature(r)) == val(ref.full_signature(r)), r
            for lv, _, _ in HP.level_sizes(r, nreg):
                assert val(pooled.best(r, lv)) == val(ref.best(r, lv)), (r, lv)
                assert val(pooled.combined(r, lv - 1)) == val(ref.combined(r, lv - 1)), (r, lv)
        pooled.close()
        ref.close()
    finally:
        e.close()


def test_pool_edges():
    """An empty pool, a full one, refused arguments, clear, two pools on one
    store set, and a pool whose registry was replaced."""
    import bench
    from handel_amd import partitioner as HP
    from handel_amd._lib import HandelGPUError
    from handel_amd.engine import PACKET_DTYPE, REQ_DTYPE, Pool

    nreg = 200
    e = _engine(nreg)
    try:
        hosted = [5, 130, 199]
        d = _Device(e, hosted)
        d.pool.close()
        with pytest.raises(HandelGPUError):
            Pool(d.st, 0)
        pool = Pool(d.st, 32)
        other = Pool(d.st, 32)
        assert pool.select_capacity(4) == 12 and pool.select_capacity(64) == 32 and pool.bytes() > 0
        # a step on an empty pool: count 0, all filler
        _check_step(d.step(pool, 4), d.stride, [])
        assert pool.count() == 0
        # ten packets, each with an individual signature, on empty stores: twenty slots of positive mark
        n = 10
        pkts = np.zeros(n, dtype=PACKET_DTYPE)
        reqs = np.zeros(2 * n, dtype=REQ_DTYPE)
        slot_bits = [0] * (2 * n)
        for i in range(n):
            r = hosted[i % 3]
            # the receiver's two largest levels (at least 32 ids each at N = 200)
            lv, lo, hi = sorted(HP.level_sizes(r, nreg), key=lambda t: t[1] - t[2])[(i // 3) % 2]
            assert hi - lo >= 32
            origin = lo + 2 * i
            pkts[i] = (origin, r, lv, HG_PKT_HAS_IND, 0, 0, 0, 0)
            reqs[i] = reqs[n + i] = (lo, hi - lo, hi - lo, 0)
            slot_bits[i] = 1 << (origin - lo) | 1 << (origin - lo + 1)
            slot_bits[n + i] = 1 << (origin - lo)
        sigs = np.arange(2 * n * 64, dtype=np.uint32).astype(np.uint8)
        codes, live = np.zeros(2 * n, dtype=np.int32), np.ones(2 * n, dtype=np.uint8)
        batch = (pkts, reqs, slot_bits, sigs, codes, live)
        d.append(pool, *batch)
        assert pool.count() == 20 and other.count() == 0  # the second pool sees none of it
        before = [tuple(x.tolist() for x in pool.read(r)) for r in hosted]
        assert sum(len(b[0]) for b in before) == 20
        with pytest.raises(HandelGPUError):  # 20 + 20 slots do not fit 32
            d.append(pool, *batch)
        assert pool.count() == 20
        assert [tuple(x.tolist() for x in pool.read(r)) for r in hosted] == before
        for bad_k in (0, 65):
            with pytest.raises(HandelGPUError):
                d.step(pool, bad_k)
        t = d.torch.zeros(4096, dtype=d.torch.uint8, device=d.dev).data_ptr()
        with pytest.raises(HandelGPUError):  # the capacity of k = 4 is 12
            pool.step_device(4, 11, t, t, t, t, t, t, t, d.s)
        assert pool.count() == 20
        out = d.step(pool, 4)
        assert out[1] == 12 and pool.count() == 8  # twelve picks left, room for twenty more
        d.append(pool, *batch)
        assert pool.count() == 28
        d.append(other, *batch)
        assert other.count() == 20 and pool.count() == 28
        pool.clear()
        assert pool.count() == 0 and other.count() == 20 and all(len(pool.read(r)[0]) == 0 for r in hosted)
        _check_step(d.step(pool, 4), d.stride, [])
        # a second registry load: the pool belongs to the first one
        assert not e.registry_load(e.keygen(bench.seeded_scalars(nreg, 5))).any()
        for call in (lambda: d.append(other, *batch), lambda: d.step(other, 4), other.count, other.clear,
                     lambda: other.read(5), lambda: Pool(d.st, 8)):
            with pytest.raises(HandelGPUError):
                call()
        other.close()
        pool.close()
        d.st.close()
    finally:
        e.close()


def test_closing_the_engine_closes_pools_first():
    """Engine.close closes its stores and they their pools, so a pool that is
    still referenced afterwards is already closed and its later release does
    nothing."""
    from handel_amd.engine import Pool
    from handel_amd.intake import DeviceStores

    e = _engine(200)
    st = DeviceStores(e, [5, 130], 8)
    pool = Pool(st, 16)
    assert pool.count() == 0
    e.close()
    assert pool.h is None and st.h is None
    pool.close()
    st.close()
