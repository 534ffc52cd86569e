"""Packet intake with the scoring step on the GPU: parse -> evaluate -> select
-> verify over arrays that stay in HBM.

Handel scores every queued signature against its store and verifies only the
best (processing.go:171-220 readTodos over store.go:101-183 Evaluate).
`DeviceStores` keeps the scoring state of the hosted Handel instances on the
device (hg_stores_*); by default the host `sigprocessing.Store` stays
authoritative: `Store.store` / unsafeCheckMerge run on the host once per
verified signature and `mirror` pushes the levels that changed. `DeviceIntake`
is one intake step for a batch of raw packets of several instances. With
`DeviceIntake(device_merge=True)` the store is complete on the device
(hg_stores_enable_merge): the step ends with hg_stores_merge_device on the
same stream, and `best` / `combined` read the device's multisignatures.

`select_reference` / `select_slots` restate the selection rule on plain
integers (the picks and the order the rest goes back to the queue in); they
are what the device selection is tested against and what `DeviceIntake` orders
its pending queue with.
"""

from __future__ import annotations

from typing import Callable, Dict, Iterable, List, Optional, Sequence, Tuple

import numpy as np

from . import partitioner as part
from ._lib import (HG_COMBINED_EMPTY, HG_MERGE_DISCARDED, HG_MERGE_STORED, HG_OK, HG_STORE_BEST_SIG,
                   HG_STORE_HAS_BEST, HG_STORE_LEVEL_FULL, HG_STORE_SIG_BEST, HandelGPUError)
from .engine import PACKET_DTYPE, REQ_DTYPE, STORE_SIG_DTYPE, STORE_UPDATE_DTYPE, Engine, Pool, Stores
from .packets import Packet, pack_packets
from .sigprocessing import IncomingSig, IndividualSigFilter, MultiSig, Store, bits_to_int, int_to_words


def queue_position(slot: int, n: int) -> int:
    """Handel's queue order of the 2n slots of a parsed batch: packet index
    first, a packet's multisignature (slot i) before its individual signature
    (slot n + i) (handel.go:145-149)."""
    return 2 * (slot % n) + (1 if slot >= n else 0)


def select_reference(marks: Sequence[int], k: int) -> Tuple[List[int], List[int]]:
    """BatchedEvaluatorProcessing.read_todos on bare marks given in queue
    order: (indices picked, best first; indices with a positive mark that go
    back to the queue, in the order read_todos re-queues them)."""
    slots: List[Tuple[int, int]] = []
    requeued: List[int] = []
    for idx, mark in enumerate(marks):
        if mark <= 0:
            continue
        if len(slots) == k and mark <= slots[-1][0]:
            requeued.append(idx)
            continue
        if len(slots) == k:
            requeued.append(slots.pop()[1])
        j = len(slots)
        while j > 0 and slots[j - 1][0] < mark:
            j -= 1
        slots.insert(j, (mark, idx))
    return [i for _, i in slots], requeued


def select_slots(store_of_slot: Sequence[int], scores: Sequence[int], n: int, k: int,
                 n_stores: int) -> Tuple[List[int], List[int]]:
    """hg_stores_select_device's contract on the host: the picked slots grouped
    by store (in store order; inside a store by score descending, then queue
    position), and the slots of positive score that were not picked, per store
    in read_todos' re-queue order. store_of_slot[slot] < 0: no store."""
    per_store: List[List[int]] = [[] for _ in range(n_stores)]
    for slot in sorted(range(2 * n), key=lambda s: queue_position(s, n)):
        st = int(store_of_slot[slot])
        if 0 <= st < n_stores:
            per_store[st].append(slot)
    picked: List[int] = []
    rest: List[int] = []
    for slots in per_store:
        p, r = select_reference([int(scores[s]) for s in slots], k)
        picked += [slots[i] for i in p]
        rest += [slots[i] for i in r]
    return picked, rest


class PoolModel:
    """The standing queue on plain Python lists: one queue per receiver, one
    `select_reference` per receiver and step. What hg_stores_pool_* is tested
    against. An item is whatever the caller queues; `step` asks `evaluate` for
    its mark."""

    def __init__(self, receivers: Sequence[int]):
        self.receivers = [int(r) for r in receivers]
        self.queues: Dict[int, List[list]] = {r: [] for r in self.receivers}  # [item, mark of the last step]
        self.disordered = 0  # (receiver, step) queues whose re-queued order was not their arrival order
        self.dropped = 0     # slots that left with a mark <= 0

    def append(self, receiver: int, item) -> bool:
        """Queues an admitted item behind the receiver's queue; False: the receiver has no store."""
        if receiver not in self.queues:
            return False
        self.queues[receiver].append([item, 0])
        return True

    def count(self) -> int:
        return sum(len(q) for q in self.queues.values())

    def queue(self, receiver: int) -> List[Tuple[object, int]]:
        return [(it, mk) for it, mk in self.queues[receiver]]

    def step(self, k: int, evaluate: Callable[[int, object], int]) -> List[Tuple[int, object, int]]:
        """One readTodos pass per receiver, in receiver order: the picks as
        (receiver, item, mark), best first inside a receiver."""
        picks: List[Tuple[int, object, int]] = []
        for r in self.receivers:
            q = self.queues[r]
            marks = [int(evaluate(r, it)) for it, _ in q]
            p, rest = select_reference(marks, k)
            picks += [(r, q[i][0], marks[i]) for i in p]
            self.disordered += rest != sorted(rest)
            self.dropped += sum(m <= 0 for m in marks)
            self.queues[r] = [[q[i][0], marks[i]] for i in rest]
        return picks


class DeviceStores(Stores):
    """hg_stores of the receivers a process hosts, fed from host `Store`s."""

    def __init__(self, engine: Engine, receivers: Sequence[int], max_packets: int, n_registry: Optional[int] = None):
        super().__init__(engine, receivers, max_packets)
        self.n = int(engine.L.hg_registry_size(engine.ctx)) if n_registry is None else int(n_registry)
        self.merge_enabled = False
        self._pushed: Dict[Tuple[int, int], set] = {}  # (receiver, level) -> individual signatures on the device

    def enable_merge(self) -> None:
        super().enable_merge()
        self.merge_enabled = True

    def mirror(self, receiver: int, store: Store, levels: Optional[Iterable[int]] = None) -> None:
        """Pushes `store`'s state of `levels` (default: every level) to the
        device store of `receiver`: the best bitset, whether there is one, and
        the verified individual signatures."""
        self.mirror_many([(receiver, store, levels)])

    def mirror_many(self, items: Sequence[Tuple[int, Store, Optional[Iterable[int]]]]) -> None:
        """`mirror` for several stores in one hg_stores_update."""
        ups, words, nw = [], [], 0
        recs, sigs = [], []  # merge-enabled sets also get the signatures
        for receiver, store, levels in items:
            if self.merge_enabled and (levels is None or 0 in levels):
                with store.lock:
                    own = store.m.get(0)
                if own is not None:
                    recs.append((receiver, 0, 0, len(sigs)))
                    sigs.append(own.sig[:64])
                if levels is not None:
                    levels = [lv for lv in levels if lv != 0]
            for level in (store.levels if levels is None else sorted(set(levels))):
                size = store.size(level)
                if size <= 0:
                    continue
                with store.lock:
                    best = store.m.get(level)
                    indiv = store.indiv_verified.get(level, 0)
                    held = dict(store.indiv_sigs.get(level, {})) if self.merge_enabled else {}
                if self.merge_enabled:
                    if best is not None:
                        recs.append((receiver, level, HG_STORE_SIG_BEST, len(sigs)))
                        sigs.append(best.sig[:64])
                    pushed = self._pushed.setdefault((receiver, level), set())
                    for idx in sorted(set(held) - pushed):
                        recs.append((receiver, level, idx, len(sigs)))
                        sigs.append(held[idx].sig[:64])
                        pushed.add(idx)
                lw = (size + 63) // 64
                best_off = nw
                if best is not None:
                    words.append(int_to_words(best.bits, size))
                    nw += lw
                words.append(int_to_words(indiv, size))
                ups.append((receiver, level, HG_STORE_HAS_BEST if best is not None else 0, best_off, nw))
                nw += lw
        if ups:
            self.update(np.array(ups, dtype=STORE_UPDATE_DTYPE), np.concatenate(words))
        if recs:  # after the update: it clears a level's "best signature known" bit
            self.update_sigs(np.array(recs, dtype=STORE_SIG_DTYPE), b"".join(sigs))


class DeviceIntake:
    """One intake step for raw packets of the hosted receivers: pack -> upload
    -> hg_parse_packets_device -> hg_stores_evaluate_device ->
    hg_stores_select_device (k per receiver) -> hg_verify_aggregate_device,
    every array staying in HBM; only the pick count, the picks, their verdicts
    and the 2n scores and parse codes come back. The valid picks then go
    through the host `Store.store` (merges through `Engine.combine_g1`) in
    selection order, and the levels that changed are pushed back to the
    device. The engine needs its registry and message set.

    Slots of positive score that were not picked stay queued here and are
    presented again, in read_todos' order, in front of the next step's packets
    (each as an entry of its own whose packet is parsed again; a pool of parsed
    slots kept in HBM across steps is not part of this). Each receiver has the reference's
    IndividualSigFilter (processing.go:299-325): an origin's individual
    signature is presented once.

    device_merge=True: the picks are merged where they lie
    (hg_stores_merge_device, on the same stream, after the verification); no
    `Store.store`, no `combine_g1`, no `mirror`. Only the merge results, the
    verdicts, scores, parse codes and the list of changed levels come back
    (`last_results`, `last_changed`); the host stores in `host` stay empty, and
    `best` / `combined` / `full_signature` read the device.

    device_pool=True: the queue lives in HBM (hg_stores_pool_*, `pool_slots`
    slots, default 4 * max_packets). A step packs, uploads and parses only the
    new packets, appends their admitted slots to the pool, and one
    hg_stores_pool_step_device scores the whole queue, hands out the picks as a
    parsed batch (verified and, with device_merge, merged as it is) and
    re-queues the rest on the device. Only the picks (records, bitsets,
    signatures, verdicts) and the new packets' parse codes come back; no
    `Packet` of an earlier step is kept and `select_slots` does not run. `step`
    then returns the pool's count in place of `unselected`; `pending_view`
    reads a receiver's queue back."""

    def __init__(self, engine: Engine, receivers: Sequence[int], k: int, max_packets: int = 4096,
                 combine: Optional[Callable[[bytes, bytes], bytes]] = None, device_merge: bool = False,
                 device_pool: bool = False, pool_slots: Optional[int] = None):
        if k < 1:
            raise ValueError("k must be >= 1")
        if device_pool and k > 64:
            raise ValueError("the device pool picks at most 64 slots per receiver")
        self.engine, self.k, self.max_packets = engine, int(k), int(max_packets)
        self.receivers = [int(r) for r in receivers]
        self.n = int(engine.L.hg_registry_size(engine.ctx))
        self.stores = DeviceStores(engine, self.receivers, self.max_packets, self.n)
        self.stride = self.stores.stride
        self.device_merge = bool(device_merge)
        if self.device_merge:
            self.stores.enable_merge()
        self.last_results: List[int] = []               # HG_MERGE_* per pick of the last step
        self.last_changed: List[Tuple[int, int]] = []   # (receiver, level) whose best the last step changed
        combine = combine or (lambda a, b: engine.combine_g1(a, b)[0])
        self.host: Dict[int, Store] = {r: Store(r, self.n, combine) for r in self.receivers}
        self.filters: Dict[int, IndividualSigFilter] = {r: IndividualSigFilter() for r in self.receivers}
        self.index = {r: i for i, r in enumerate(self.receivers)}
        # (packet, receiver, multisignature still queued, individual signature still queued)
        self.pending: List[Tuple[Packet, int, bool, bool]] = []
        self.device_pool = bool(device_pool)
        self.pool: Optional[Pool] = None
        self.last_uploaded = 0  # packets the last pooled step packed and uploaded
        if self.device_pool:
            self.pool = Pool(self.stores, int(pool_slots) if pool_slots else 4 * self.max_packets)

    def close(self):
        if self.pool is not None:
            self.pool.close()
            self.pool = None
        self.stores.close()

    def pending_view(self, receiver: int) -> List[Tuple[int, int, bool, int]]:
        """device_pool: the receiver's queue as (origin, level, individual, last mark), in queue order."""
        if self.pool is None:
            raise HandelGPUError("pending_view needs device_pool=True")
        pkts, ind, marks = self.pool.read(receiver)
        return [(int(p["origin"]), int(p["level"]), bool(i), int(m)) for p, i, m in zip(pkts, ind, marks)]

    def set_own(self, receiver: int, sig: bytes) -> None:
        """The receiver's own signature, its level 0 (handel.go:116)."""
        if self.device_merge:
            self.stores.update_sigs(np.array([(receiver, 0, 0, 0)], dtype=STORE_SIG_DTYPE), bytes(sig[:64]))
        else:
            self.host[receiver].store_own(sig)

    def best(self, receiver: int, level: int) -> Optional[MultiSig]:
        """store.go:231-236 Best of one level (0: the own signature)."""
        if not self.device_merge:
            return self.host[receiver].best(level)[0]
        words, sig, flags = self.stores.read_best(receiver, level)
        if not flags & HG_STORE_HAS_BEST:
            return None
        if not flags & HG_STORE_BEST_SIG:
            raise HandelGPUError("the level's best signature is not on the device")
        lo, hi = part.range_level(receiver, self.n, level)
        return MultiSig(hi - lo, int.from_bytes(words.astype("<u8").tobytes(), "little"), sig)

    def combined(self, receiver: int, level: int) -> Optional[MultiSig]:
        """store.go:248-262 Combined(level); level None: FullSignature (:238-246)."""
        if not self.device_merge:
            st = self.host[receiver]
            return st.full_signature() if level is None else st.combined(level)
        codes, bitlens, words, sigs = self.stores.combined(
            [(receiver, HG_STORE_LEVEL_FULL if level is None else level)])
        if codes[0] == HG_COMBINED_EMPTY:
            return None
        if codes[0] != HG_OK:
            raise HandelGPUError(f"hg_stores_combined: query code {int(codes[0])}")
        return MultiSig(int(bitlens[0]), int.from_bytes(words[0].astype("<u8").tobytes(), "little"), sigs[0].tobytes())

    def full_signature(self, receiver: int) -> Optional[MultiSig]:
        return self.combined(receiver, None)

    def _incoming(self, pkt: Packet, receiver: int, individual: bool) -> IncomingSig:
        lo, hi = part.range_level(receiver, self.n, pkt.level)
        if individual:
            ms = MultiSig(hi - lo, 1 << (pkt.origin - lo), bytes(pkt.individual[:64]))
            return IncomingSig(pkt.origin, pkt.level, ms, ind=True, mapped_index=pkt.origin - lo)
        bits, sig = part.multisig_unmarshal(pkt.multisig)
        return IncomingSig(pkt.origin, pkt.level, MultiSig(len(bits), bits_to_int(bits), bytes(sig[:64])))

    def step(self, packets: Sequence[Packet], receivers: Sequence[int]):
        """Returns (results, unselected): results holds (receiver, IncomingSig,
        error text or None) per picked slot in selection order; unselected the
        slots of positive score that were not picked (indices into this step's
        2n slots, queued slots first), which stay queued for the next step."""
        import torch

        if len(packets) != len(receivers):
            raise ValueError("one receiver per packet")
        if self.device_pool:
            return self._step_pool(packets, receivers)
        batch = list(self.pending) + [(p, int(r), True, p.individual is not None) for p, r in zip(packets, receivers)]
        n, n_old = len(batch), len(self.pending)
        if n == 0:
            return [], []
        if n > self.max_packets:
            raise ValueError(f"{n} packets (queued ones included) exceed max_packets = {self.max_packets}")
        live = np.zeros(2 * n, dtype=np.uint8)
        fresh_ind = []  # new packets whose individual signature passed the filter now
        for i, (p, r, want_ms, want_ind) in enumerate(batch):
            live[i] = want_ms
            if i >= n_old and want_ind and r in self.filters:
                # the filter sees a signature once its packet parsed (handel.go:127-152): undone below if it did not
                want_ind = self.filters[r].accept(IncomingSig(p.origin, p.level, None, ind=True))
                if want_ind:
                    fresh_ind.append(i)
            live[n + i] = want_ind
        pool, recs = pack_packets([b[0] for b in batch], [b[1] for b in batch])
        eng, st, stride = self.engine, self.stores, self.stride
        dev = torch.device("cuda", eng.device)
        up = lambda a: torch.from_numpy(np.ascontiguousarray(a).view(np.uint8).reshape(-1).copy()).to(dev)  # noqa: E731
        d_pool, d_pkts, d_live = up(np.frombuffer(pool, dtype=np.uint8)), up(recs), up(live)
        cap = st.select_capacity(n, self.k)
        d_reqs = torch.empty(2 * n * REQ_DTYPE.itemsize, dtype=torch.uint8, device=dev)
        d_words = torch.empty(2 * n * stride, dtype=torch.int64, device=dev)
        d_sigs = torch.empty(2 * n * 64, dtype=torch.uint8, device=dev)
        d_pcodes = torch.empty(2 * n, dtype=torch.int32, device=dev)
        d_scores = torch.empty(2 * n, dtype=torch.int32, device=dev)
        d_sel = torch.empty(cap, dtype=torch.int32, device=dev)
        d_count = torch.zeros(1, dtype=torch.int32, device=dev)
        d_oreqs = torch.empty(cap * REQ_DTYPE.itemsize, dtype=torch.uint8, device=dev)
        d_osigs = torch.empty(cap * 64, dtype=torch.uint8, device=dev)
        d_vcodes = torch.empty(cap, dtype=torch.int32, device=dev)
        s = torch.cuda.current_stream(dev).cuda_stream
        eng.parse_packets_device(d_pool.data_ptr(), len(pool), d_pkts.data_ptr(), n, stride, d_reqs.data_ptr(),
                                 d_words.data_ptr(), d_sigs.data_ptr(), d_pcodes.data_ptr(), s)
        st.evaluate_device(d_pkts.data_ptr(), n, stride, d_words.data_ptr(), d_pcodes.data_ptr(), d_live.data_ptr(),
                           d_scores.data_ptr(), s)
        st.select_device(d_pkts.data_ptr(), n, d_scores.data_ptr(), self.k, d_reqs.data_ptr(), d_sigs.data_ptr(),
                         d_sel.data_ptr(), d_count.data_ptr(), d_oreqs.data_ptr(), d_osigs.data_ptr(), s)
        # the whole capacity without reading the count first: the filler fails the level check
        eng.verify_aggregate_device(d_oreqs.data_ptr(), cap, d_words.data_ptr(), d_osigs.data_ptr(),
                                    d_vcodes.data_ptr(), stream=s)
        if self.device_merge:
            d_results = torch.empty(cap, dtype=torch.int32, device=dev)
            d_changed = torch.empty(2 * cap, dtype=torch.int32, device=dev)
            d_nchanged = torch.zeros(1, dtype=torch.int32, device=dev)
            st.merge_device(d_pkts.data_ptr(), n, d_sel.data_ptr(), d_count.data_ptr(), cap, d_vcodes.data_ptr(),
                            stride, d_words.data_ptr(), d_sigs.data_ptr(), d_results.data_ptr(),
                            d_changed.data_ptr(), d_nchanged.data_ptr(), s)
        torch.cuda.synchronize(dev)
        count = int(d_count.cpu().numpy()[0])
        sel = d_sel.cpu().numpy()[:count].astype(np.int64)
        vcodes = d_vcodes.cpu().numpy()[:count]
        scores = d_scores.cpu().numpy()
        pcodes = d_pcodes.cpu().numpy()
        for i in fresh_ind:  # a packet that failed to parse never reached the filter
            if pcodes[i] != HG_OK:
                self.filters[batch[i][1]].seen.pop(batch[i][0].origin, None)
        results, changed = [], {}
        if self.device_merge:
            merged = d_results.cpu().numpy()[:count]
            nch = int(d_nchanged.cpu().numpy()[0])
            self.last_results = merged.tolist()
            self.last_changed = [tuple(x) for x in d_changed.cpu().numpy()[:2 * nch].reshape(-1, 2).tolist()]
        for e, (slot, code) in enumerate(zip(sel.tolist(), vcodes.tolist())):
            p, r = batch[slot % n][0], batch[slot % n][1]
            sp = self._incoming(p, r, slot >= n)
            err = None if code == HG_OK else eng.processing_error_string(int(code))
            if self.device_merge:
                if err is None and merged[e] not in (HG_MERGE_STORED, HG_MERGE_DISCARDED):
                    err = f"device merge: result {int(merged[e])}"
            elif err is None:
                self.host[r].store(sp)
                changed.setdefault(r, set()).add(sp.level)
            results.append((r, sp, err))
        if changed:
            st.mirror_many([(r, self.host[r], lv) for r, lv in changed.items()])
        store_of_slot = [self.index.get(batch[slot % n][1], -1) for slot in range(2 * n)]
        picked, rest = select_slots(store_of_slot, scores, n, self.k, len(self.receivers))
        if picked != sel.tolist():
            raise HandelGPUError("device selection differs from read_todos' rule")
        # the queue of the next step: one entry per waiting slot, in read_todos' order
        self.pending = [(batch[slot % n][0], batch[slot % n][1], slot < n, slot >= n) for slot in rest]
        return results, rest

    def _step_pool(self, packets: Sequence[Packet], receivers: Sequence[int]):
        """`step` with the queue in HBM: (results, slots left in the pool)."""
        import torch

        n = len(packets)
        if n > self.max_packets:
            raise ValueError(f"{n} packets exceed max_packets = {self.max_packets}")
        eng, st, pool, stride = self.engine, self.stores, self.pool, self.stride
        dev = torch.device("cuda", eng.device)
        s = torch.cuda.current_stream(dev).cuda_stream
        up = lambda a: torch.from_numpy(np.ascontiguousarray(a).view(np.uint8).reshape(-1).copy()).to(dev)  # noqa: E731
        recv = [int(r) for r in receivers]
        fresh_ind = []  # new packets whose individual signature passed the filter now
        d_pcodes = None
        self.last_uploaded = n
        if n:
            live = np.ones(2 * n, dtype=np.uint8)
            for i, (p, r) in enumerate(zip(packets, recv)):
                want_ind = p.individual is not None
                if want_ind and r in self.filters:
                    want_ind = self.filters[r].accept(IncomingSig(p.origin, p.level, None, ind=True))
                    if want_ind:
                        fresh_ind.append(i)
                live[n + i] = want_ind
            wire, recs = pack_packets(list(packets), recv)
            d_wire, d_pkts, d_live = up(np.frombuffer(wire, dtype=np.uint8)), up(recs), up(live)
            d_reqs = torch.empty(2 * n * REQ_DTYPE.itemsize, dtype=torch.uint8, device=dev)
            d_words = torch.empty(2 * n * stride, dtype=torch.int64, device=dev)
            d_sigs = torch.empty(2 * n * 64, dtype=torch.uint8, device=dev)
            d_pcodes = torch.empty(2 * n, dtype=torch.int32, device=dev)
            eng.parse_packets_device(d_wire.data_ptr(), len(wire), d_pkts.data_ptr(), n, stride, d_reqs.data_ptr(),
                                     d_words.data_ptr(), d_sigs.data_ptr(), d_pcodes.data_ptr(), s)
            try:
                pool.append_device(d_pkts.data_ptr(), n, stride, d_reqs.data_ptr(), d_words.data_ptr(),
                                   d_sigs.data_ptr(), d_pcodes.data_ptr(), d_live.data_ptr(), s)
            except HandelGPUError:
                for i in fresh_ind:  # nothing was queued: the filter has not seen these
                    self.filters[recv[i]].seen.pop(packets[i].origin, None)
                raise
        cap = pool.select_capacity(self.k)
        d_opkts = torch.empty(cap * PACKET_DTYPE.itemsize, dtype=torch.uint8, device=dev)
        d_sel = torch.empty(cap, dtype=torch.int32, device=dev)
        d_count = torch.zeros(1, dtype=torch.int32, device=dev)
        d_oreqs = torch.empty(cap * REQ_DTYPE.itemsize, dtype=torch.uint8, device=dev)
        d_owords = torch.empty(2 * cap * stride, dtype=torch.int64, device=dev)
        d_osigs = torch.empty(2 * cap * 64, dtype=torch.uint8, device=dev)
        d_marks = torch.empty(cap, dtype=torch.int32, device=dev)
        d_vcodes = torch.empty(cap, dtype=torch.int32, device=dev)
        pool.step_device(self.k, cap, d_opkts.data_ptr(), d_sel.data_ptr(), d_count.data_ptr(), d_oreqs.data_ptr(),
                         d_owords.data_ptr(), d_osigs.data_ptr(), d_marks.data_ptr(), s)
        # the whole capacity without reading the count first: the filler fails the level check
        eng.verify_aggregate_device(d_oreqs.data_ptr(), cap, d_owords.data_ptr(), d_osigs.data_ptr(),
                                    d_vcodes.data_ptr(), stream=s)
        if self.device_merge:
            d_results = torch.empty(cap, dtype=torch.int32, device=dev)
            d_changed = torch.empty(2 * cap, dtype=torch.int32, device=dev)
            d_nchanged = torch.zeros(1, dtype=torch.int32, device=dev)
            st.merge_device(d_opkts.data_ptr(), cap, d_sel.data_ptr(), d_count.data_ptr(), cap, d_vcodes.data_ptr(),
                            stride, d_owords.data_ptr(), d_osigs.data_ptr(), d_results.data_ptr(),
                            d_changed.data_ptr(), d_nchanged.data_ptr(), s)
        torch.cuda.synchronize(dev)
        count = int(d_count.cpu().numpy()[0])
        sel = d_sel[:count].cpu().numpy().astype(np.int64)
        vcodes = d_vcodes[:count].cpu().numpy()
        opkts = np.frombuffer(d_opkts[:count * PACKET_DTYPE.itemsize].cpu().numpy().tobytes(), dtype=PACKET_DTYPE)
        oreqs = np.frombuffer(d_oreqs[:count * REQ_DTYPE.itemsize].cpu().numpy().tobytes(), dtype=REQ_DTYPE)
        owords = d_owords.view(2 * cap, stride).index_select(0, d_sel[:count].long()).cpu().numpy().view(np.uint64)
        osigs = d_osigs[:count * 64].cpu().numpy().reshape(count, 64)
        if d_pcodes is not None:
            pcodes = d_pcodes.cpu().numpy()
            for i in fresh_ind:  # a packet that failed to parse never reached the filter
                if pcodes[i] != HG_OK:
                    self.filters[recv[i]].seen.pop(packets[i].origin, None)
        results, changed = [], {}
        if self.device_merge:
            merged = d_results.cpu().numpy()[:count]
            nch = int(d_nchanged.cpu().numpy()[0])
            self.last_results = merged.tolist()
            self.last_changed = [tuple(x) for x in d_changed.cpu().numpy()[:2 * nch].reshape(-1, 2).tolist()]
        for e in range(count):
            r, origin, level = int(opkts[e]["receiver"]), int(opkts[e]["origin"]), int(opkts[e]["level"])
            sig = osigs[e].tobytes()
            if sel[e] >= cap:
                lo, hi = part.range_level(r, self.n, level)
                sp = IncomingSig(origin, level, MultiSig(hi - lo, 1 << (origin - lo), sig), ind=True,
                                 mapped_index=origin - lo)
            else:
                bits = int.from_bytes(owords[e].astype("<u8").tobytes(), "little")
                sp = IncomingSig(origin, level, MultiSig(int(oreqs[e]["bitlen"]), bits, sig))
            code = int(vcodes[e])
            err = None if code == HG_OK else eng.processing_error_string(code)
            if self.device_merge:
                if err is None and merged[e] not in (HG_MERGE_STORED, HG_MERGE_DISCARDED):
                    err = f"device merge: result {int(merged[e])}"
            elif err is None:
                self.host[r].store(sp)
                changed.setdefault(r, set()).add(sp.level)
            results.append((r, sp, err))
        if changed:
            st.mirror_many([(r, self.host[r], lv) for r, lv in changed.items()])
        return results, pool.count()
