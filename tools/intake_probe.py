#!/usr/bin/env python3
"""Times the device scoring step (hg_stores_evaluate_device) and scoring plus
selection (hg_stores_select_device) on 2 x 4096 parsed slots of a 4000-key
registry with 250 hosted receivers, against the host loop it replaces
(sigprocessing.Store.evaluate per slot) on the same machine, and the verify
step the selection feeds. One process; HIP events around back-to-back calls on
one stream, several windows after a warm-up.

  python tools/intake_probe.py [--out profiles/intake_probe.json] [--reps 200] [--windows 5]

Bytes are the algorithm's: 3 x stride x 8 per slot that is scored against a
store (the slot's bitset, the level's best, its verified individual
signatures).

The same run also times the opt-in device store at this shape
(hg_stores_enable_merge): (a) hg_stores_merge_device over the selection with
every pick verified, each timed call on the freshly mirrored state (a repeated
call on the merged state, where nearly every entry is discarded, is given
beside it); (b) the host tail it replaces on the default DeviceIntake path,
Store.store with Engine.combine_g1 for every pick plus mirror_many of the
changed levels; (c) hg_stores_combined_device for all receivers x levels
against Store.combined in a host loop. Device and host states, and every
Combined, are asserted equal before anything is reported. Needs a GPU: there is
no fallback.
"""

import argparse
import json
import os
import random
import statistics
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

N_REG, N_RECV, N_PKTS, K = 4000, 250, 4096, 8


def rand_bits(rng, size, density):
    return int.from_bytes(np.packbits(rng.random(size) < density, bitorder="little").tobytes(), "little")


def make_case(seed=7):
    """Random store states and Handel-shaped slots: every packet a hosted
    receiver's level with a multisignature of density U[0.05, 1]; half carry
    an individual signature."""
    from handel_amd import partitioner as HP
    from handel_amd.engine import PACKET_DTYPE, REQ_DTYPE
    from handel_amd.sigprocessing import IncomingSig, MultiSig, Store

    rnd, rng = random.Random(seed), np.random.default_rng(seed)
    receivers = rnd.sample(range(N_REG), N_RECV)
    host = {}
    for r in receivers:
        s = Store(r, N_REG, lambda a, b: a)
        for lv in s.levels:
            size = s.size(lv)
            state = rnd.choice(["none", 0.05, 0.5, 0.95])
            if state != "none":
                s.m[lv] = MultiSig(size, rand_bits(rng, size, state) | 1, b"")
            s.indiv_verified[lv] = rand_bits(rng, size, rnd.choice([0.0, 0.02, 0.3]))
        host[r] = s
    n = N_PKTS
    stride = (2 ** (HP.log2_ceil(N_REG) - 1) + 63) // 64
    pkts = np.zeros(n, dtype=PACKET_DTYPE)
    reqs = np.zeros(2 * n, dtype=REQ_DTYPE)
    words = np.zeros(2 * n * stride, dtype=np.uint64)
    codes = np.zeros(2 * n, dtype=np.int32)
    sps = [None] * (2 * n)
    for i in range(n):
        r = rnd.choice(receivers)
        lv, lo, hi = rnd.choice(HP.level_sizes(r, N_REG))
        size = hi - lo
        origin = lo + rnd.randrange(size)
        pkts[i] = (origin, r, lv, 0, 0, 0, 0, 0)
        bits = rand_bits(rng, size, rnd.uniform(0.05, 1.0)) | 1 << (origin - lo)
        slots = [(i, bits, False)]
        if rnd.random() < 0.5:
            slots.append((n + i, 1 << (origin - lo), True))
        else:
            codes[n + i] = 29  # HG_PKT_NO_IND
        for slot, b, ind in slots:
            words[slot * stride:(slot + 1) * stride] = np.frombuffer(b.to_bytes(8 * stride, "little"), dtype="<u8")
            sps[slot] = (r, IncomingSig(origin, lv, MultiSig(size, b, b""), ind=ind, mapped_index=origin - lo))
        reqs[i] = reqs[n + i] = (lo, size, size, 0)
        reqs[i]["word_offset"], reqs[n + i]["word_offset"] = i * stride, (n + i) * stride
    return receivers, host, pkts, reqs, words, codes, sps, stride


def merge_probe(a, e, st, host, receivers, pkts, words, sps, stride, d_pkts, d_words, d_sel, d_count, cap, dev, stream,
                timed, up):
    """(a), (b), (c) of the module text on the selection d_sel / d_count holds;
    `st` (the default, scoring-only set) takes the host tail's mirror."""
    import torch

    import bench
    from handel_amd import partitioner as HP
    from handel_amd._lib import HG_MERGE_DISCARDED, HG_MERGE_STORED, HG_STORE_BEST_SIG, HG_STORE_HAS_BEST
    from handel_amd.engine import STORE_QUERY_DTYPE
    from handel_amd.intake import DeviceStores
    from handel_amd.sigprocessing import IncomingSig, MultiSig, Store

    n, s = N_PKTS, stream.cuda_stream
    top = HP.log2_ceil(N_REG)
    # real, distinct points: every slot its own, the seeded state's drawn from a pool by position
    slot_sigs = e.sign(bench.seeded_scalars(2 * n, 4001))
    pool_b = e.sign(bench.seeded_scalars(4096, 4002))
    pool = [pool_b[64 * i:64 * i + 64] for i in range(4096)]
    own = e.sign(bench.seeded_scalars(N_REG, 4000))
    combine = lambda x, y: e.combine_g1(x, y)[0]  # noqa: E731
    host2 = {}
    for r in receivers:
        h = Store(r, N_REG, combine)
        h.store_own(own[64 * r:64 * r + 64])
        for lv in h.levels:
            size = h.size(lv)
            cur = host[r].m.get(lv)
            if cur is not None:
                h.m[lv] = MultiSig(size, cur.bits, pool[(r * 31 + lv) % 4096])
            iv = host[r].indiv_verified[lv]
            h.indiv_verified[lv] = iv
            for idx in range(size):
                if (iv >> idx) & 1:
                    h.indiv_sigs[lv][idx] = MultiSig(size, 1 << idx, pool[(r * 131 + lv * 17 + idx) % 4096])
        host2[r] = h
    stm = DeviceStores(e, receivers, n)
    stm.enable_merge()
    count = int(d_count.cpu()[0])
    sel = d_sel.cpu().numpy().view(np.uint32)[:count].tolist()
    d_sigs2 = up(np.frombuffer(slot_sigs, dtype=np.uint8))
    d_ok = torch.zeros(cap, dtype=torch.int32, device=dev)  # every pick verified: the most merge work
    d_results = torch.zeros(cap, dtype=torch.int32, device=dev)
    d_changed = torch.zeros(2 * cap, dtype=torch.int32, device=dev)
    d_nchanged = torch.zeros(1, dtype=torch.int32, device=dev)

    def merge():
        stm.merge_device(d_pkts.data_ptr(), n, d_sel.data_ptr(), d_count.data_ptr(), cap, d_ok.data_ptr(), stride,
                         d_words.data_ptr(), d_sigs2.data_ptr(), d_results.data_ptr(), d_changed.data_ptr(),
                         d_nchanged.data_ptr(), s)

    # (a) one call per window on the mirrored pre-state (a merged state would discard nearly everything)
    first_ms = []
    for w in range(a.windows + 1):  # the first window is the warm-up
        stm.mirror_many([(r, host2[r], None) for r in receivers])
        torch.cuda.synchronize(dev)
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record(stream)
        merge()
        e1.record(stream)
        e1.synchronize()
        if w:
            first_ms.append(e0.elapsed_time(e1))
    results = d_results.cpu().numpy()[:count].tolist()
    nchanged = int(d_nchanged.cpu()[0])
    # the device state after that one merge, read before anything else touches it
    as_int = lambda w: int.from_bytes(w.astype("<u8").tobytes(), "little")  # noqa: E731
    device_rows = {}
    for r in receivers:
        for lv in host2[r].levels:
            best, sig, flags = stm.read_best(r, lv)
            device_rows[(r, lv)] = (as_int(best), sig, flags, as_int(stm.read(r, lv)[1]))

    # (c) Combined of every receiver and level, on the same state
    queries = np.array([(r, lv) for r in receivers for lv in range(top)], dtype=STORE_QUERY_DTYPE)
    m, ws = len(queries), (N_REG + 63) // 64
    d_q = up(queries)
    d_qcodes = torch.zeros(m, dtype=torch.int32, device=dev)
    d_qbits = torch.zeros(m, dtype=torch.int32, device=dev)
    d_qwords = torch.zeros(m * ws, dtype=torch.int64, device=dev)
    d_qsigs = torch.zeros(m * 64, dtype=torch.uint8, device=dev)

    def combined():
        stm.combined_device(d_q.data_ptr(), m, ws, d_qcodes.data_ptr(), d_qbits.data_ptr(), d_qwords.data_ptr(),
                            d_qsigs.data_ptr(), s)

    for _ in range(3):
        combined()
    comb_ms = timed(combined, max(20, a.reps // 10))
    torch.cuda.synchronize(dev)
    qcodes, qbits = d_qcodes.cpu().numpy(), d_qbits.cpu().numpy()
    qwords = d_qwords.cpu().numpy().view(np.uint64).reshape(m, ws)
    qsigs = d_qsigs.cpu().numpy().reshape(m, 64)

    # the same entries again: the merged state discards nearly all of them (the call's floor)
    repeat_ms = timed(merge, max(20, a.reps // 10))
    torch.cuda.synchronize(dev)

    # (b) the host tail of the default path on the same picks
    t0 = time.perf_counter()
    changed, want_results = {}, []
    for slot in sel:
        r, sp = sps[slot]
        sp = IncomingSig(sp.origin, sp.level, MultiSig(sp.ms.bitlen, sp.ms.bits, slot_sigs[64 * slot:64 * slot + 64]),
                         ind=sp.ind, mapped_index=sp.mapped_index)
        kept = host2[r].store(sp)
        want_results.append(HG_MERGE_STORED if kept is not None else HG_MERGE_DISCARDED)
        changed.setdefault(r, set()).add(sp.level)
    t1 = time.perf_counter()
    st.mirror_many([(r, host2[r], lv) for r, lv in changed.items()])
    t2 = time.perf_counter()
    states_equal = results == want_results
    for r in receivers:
        for lv in host2[r].levels:
            best, sig, flags, indiv = device_rows[(r, lv)]
            want = host2[r].m.get(lv)
            ok = bool(flags & HG_STORE_HAS_BEST) == (want is not None)
            if ok and want is not None:
                ok = bool(flags & HG_STORE_BEST_SIG) and sig == want.sig and best == want.bits
            states_equal = states_equal and ok and indiv == host2[r].indiv_verified[lv]
    t3 = time.perf_counter()
    want_comb = [host2[int(r)].combined(int(lv)) for r, lv in queries]
    t4 = time.perf_counter()
    combined_equal = all(
        qcodes[q] == 0 and (int(qbits[q]), int.from_bytes(qwords[q].astype("<u8").tobytes(), "little"),
                            qsigs[q].tobytes()) == (ms.bitlen, ms.bits, ms.sig)
        for q, ms in enumerate(want_comb))  # every store holds its own signature: never empty
    stm.close()
    fm, rm, cm = statistics.median(first_ms), statistics.median(repeat_ms), statistics.median(comb_ms)
    rec = {
        "merge_what": "hg_stores_merge_device over the selection, every pick verified; hg_stores_combined_device for all "
                      "receivers x levels; host: Store.store / Store.combined with Engine.combine_g1",
        "merge_entries": count, "merge_stored": results.count(HG_MERGE_STORED),
        "merge_discarded": results.count(HG_MERGE_DISCARDED), "merge_rows_changed": nchanged,
        "merge_states_equal_host": bool(states_equal),
        "merge_first_ms": {"median": fm, "min": min(first_ms), "max": max(first_ms), "calls_per_window": 1},
        "merge_repeat_ms": {"median": rm, "min": min(repeat_ms), "max": max(repeat_ms)},
        "host_tail_s": {"store": t1 - t0, "mirror_many": t2 - t1, "total": t2 - t0},
        "merge_device_over_host_tail": (t2 - t0) * 1e3 / fm,
        "combined_queries": m, "combined_equal_host": bool(combined_equal),
        "combined_ms": {"median": cm, "min": min(comb_ms), "max": max(comb_ms)},
        "host_combined_s": t4 - t3,
        "combined_device_over_host": (t4 - t3) * 1e3 / cm,
    }
    if not (states_equal and combined_equal):
        print(json.dumps(rec))
        sys.exit("device store differs from the host Store")
    return rec


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "intake_probe.json"))
    ap.add_argument("--reps", type=int, default=200)
    ap.add_argument("--windows", type=int, default=5)
    a = ap.parse_args()
    if a.reps < 100:
        ap.error("--reps must be at least 100")

    import torch

    import bench
    from handel_amd.engine import REQ_DTYPE, Engine
    from handel_amd.intake import DeviceStores

    receivers, host, pkts, reqs, words, codes, sps, stride = make_case()
    n = N_PKTS
    scored = [s for s in range(2 * n) if sps[s] is not None]

    # the host loop this replaces: Store.evaluate per queued signature
    host_s = []
    for _ in range(3):
        t0 = time.perf_counter()
        want = [host[sps[s][0]].evaluate(sps[s][1]) for s in scored]
        host_s.append(time.perf_counter() - t0)
    want_all = np.zeros(2 * n, dtype=np.int32)
    want_all[scored] = want

    e = Engine(device=0, flavor="go")
    assert e.set_message(bench.LIB_MESSAGE) == 0
    kb = bench.seeded_scalars(N_REG, 4000)
    assert not e.registry_load(e.keygen(kb)).any()
    e.set_aggregate_level(1)  # the 8-key GT tables: built in milliseconds
    e.prepare_aggregate()
    st = DeviceStores(e, receivers, n)
    st.mirror_many([(r, host[r], None) for r in receivers])
    sig = e.sign(kb[:32])  # one valid curve point for every slot: the verdicts are not the subject
    dev = torch.device("cuda", 0)
    up = lambda x: torch.from_numpy(np.ascontiguousarray(x).view(np.uint8).reshape(-1).copy()).to(dev)  # noqa: E731
    d_pkts, d_reqs, d_words, d_codes = up(pkts), up(reqs), up(words), up(codes)
    d_sigs = up(np.frombuffer(sig * (2 * n), dtype=np.uint8))
    d_scores = torch.zeros(2 * n, dtype=torch.int32, device=dev)
    cap = st.select_capacity(n, K)
    d_sel = torch.zeros(cap, dtype=torch.int32, device=dev)
    d_count = torch.zeros(1, dtype=torch.int32, device=dev)
    d_oreqs = torch.zeros(cap * REQ_DTYPE.itemsize, dtype=torch.uint8, device=dev)
    d_osigs = torch.zeros(cap * 64, dtype=torch.uint8, device=dev)
    d_vcodes = torch.zeros(cap, dtype=torch.int32, device=dev)
    # a stream of the probe's own: handle 0 (torch's default stream) would mean
    # the context's stream to the engine, outside the events below
    stream = torch.cuda.Stream(dev)
    s = stream.cuda_stream
    assert s != 0

    def evaluate():
        st.evaluate_device(d_pkts.data_ptr(), n, stride, d_words.data_ptr(), d_codes.data_ptr(), 0,
                           d_scores.data_ptr(), s)

    def select():
        st.select_device(d_pkts.data_ptr(), n, d_scores.data_ptr(), K, d_reqs.data_ptr(), d_sigs.data_ptr(),
                         d_sel.data_ptr(), d_count.data_ptr(), d_oreqs.data_ptr(), d_osigs.data_ptr(), s)

    def verify():
        e.verify_aggregate_device(d_oreqs.data_ptr(), cap, d_words.data_ptr(), d_osigs.data_ptr(),
                                  d_vcodes.data_ptr(), stream=s)

    def both():
        evaluate()
        select()

    def timed(fn, reps):
        """ms per call: HIP events around `reps` back-to-back calls, per window"""
        out = []
        for _ in range(a.windows):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record(stream)
            for _ in range(reps):
                fn()
            e1.record(stream)
            e1.synchronize()
            out.append(e0.elapsed_time(e1) / reps)
        return out

    for fn in (evaluate, both, verify):  # warm-up: code objects, workspaces
        for _ in range(10):
            fn()
    torch.cuda.synchronize(dev)
    scores_equal = bool(np.array_equal(d_scores.cpu().numpy(), want_all))
    count = int(d_count.cpu()[0])
    ev_ms, both_ms = timed(evaluate, a.reps), timed(both, a.reps)
    ver_ms = timed(verify, max(20, a.reps // 10))
    torch.cuda.synchronize(dev)

    merge_rec = merge_probe(a, e, st, host, receivers, pkts, words, sps, stride, d_pkts, d_words, d_sel, d_count, cap,
                            dev, stream, timed, up)

    ev, bo, ve, hs = statistics.median(ev_ms), statistics.median(both_ms), statistics.median(ver_ms), min(host_s)
    nbytes = len(scored) * 3 * stride * 8
    rec = {
        "what": "hg_stores_evaluate_device / + hg_stores_select_device, HIP events around back-to-back calls on one stream",
        "registry": N_REG, "receivers": N_RECV, "packets": n, "slots": 2 * n, "slots_scored": len(scored),
        "stride_words": stride, "k": K, "reps_per_window": a.reps, "windows": a.windows,
        "scores_equal_host": scores_equal,
        "evaluate_ms": {"median": ev, "min": min(ev_ms), "max": max(ev_ms)},
        "evaluate_slots_per_s": 2 * n / (ev / 1e3),
        "evaluate_bytes": nbytes, "evaluate_bytes_per_s": nbytes / (ev / 1e3),
        "evaluate_select_ms": {"median": bo, "min": min(both_ms), "max": max(both_ms)},
        "evaluate_select_slots_per_s": 2 * n / (bo / 1e3),
        "selected": count, "select_capacity": cap,
        "verify_capacity_ms": {"median": ve, "min": min(ver_ms), "max": max(ver_ms)},
        "verify_table_level": e.aggregate_tables(),
        "host_evaluate_s": {"best": hs, "all": host_s},
        "host_slots_per_s": len(scored) / hs,
        "device_over_host": (hs * 1e3) / ev,
        "device_select_over_host": (hs * 1e3) / bo,
    }
    rec.update(merge_rec)
    st.close()
    e.close()
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(rec, f, indent=1)
        f.write("\n")
    print(json.dumps(rec))
    if not scores_equal:
        sys.exit("device scores differ from Store.evaluate")


if __name__ == "__main__":
    main()
