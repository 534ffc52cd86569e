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
signatures). Needs a GPU: there is no fallback.
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
