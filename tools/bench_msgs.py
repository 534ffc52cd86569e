#!/usr/bin/env python3
"""Cost of giving every check its own message (hg_verify_batch_msgs_device)
against the one-message batch it extends. Prints ONE JSON line.

  (a) hg_verify_batch_msgs_device: N checks on N distinct hashable 32-byte messages
  (b) hg_verify_batch_device: the same N checks' work on one message (the floor)
  (c) the route without the multi-message entry: hg_verify_batch_msg with
      n = 1 per message, on LOOP messages (host calls, wall clock), scaled to N
  (d) the hash kernels alone: the SUBMIT - VERIFY phase time of (a) minus that
      of (b) (hg_timing_read_phase: events around the whole submission and
      around the pairing kernels), and hg_hash_messages as a host call

(a) and (b) are device-resident calls timed with HIP events on one stream,
warm, REPS times each, interleaved, in the one-kernel and the split form
(hg_set_verify_split); the medians are reported. Every signature is valid and
the codes are checked.

  python tools/bench_msgs.py [--n 4096] [--reps 21] [--loop 256]

--mode aggregate measures the aggregate form instead (main_aggregate below):
  python tools/bench_msgs.py --mode aggregate [--registry 4000] [--n 4096] [--reps 21] [--loop 256]
"""

import argparse
import hashlib
import json
import os
import statistics
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

ORDER = 65000549695646603732796438742359905742570406053903786389881062969044166799969


def hashable_messages(n, size=32):
    out, i = [], 0
    while len(out) < n:
        m = hashlib.sha256(b"bench-msgs:%d" % i).digest()[:size]
        if 0 < int.from_bytes(hashlib.sha256(m).digest(), "big") < ORDER:
            out.append(m)
        i += 1
    return out


def aggregate_requests(n_reg, n, seed, full):
    """Config 3's level mix (bench.make_aggregate_batch: a random node's random
    non-empty level, bitset density U[0.5, 1.0]) or, full, n full-registry
    multisignatures: (reqs, words, the sum of the set bits' secret keys per
    request, the registry's secret keys)."""
    from handel_amd.engine import REQ_DTYPE
    from handel_amd.partitioner import bits_to_words, level_sizes

    rng = np.random.default_rng(seed)
    ks = [int.from_bytes(hashlib.sha256(b"bench-agg-key:%d" % i).digest(), "big") % ORDER or 1 for i in range(n_reg)]
    limbs = np.array([[(k >> (32 * j)) & 0xFFFFFFFF for j in range(8)] for k in ks], dtype=np.int64)
    reqs, words, sums = [], [], []
    nodes = rng.integers(0, n_reg, size=n)
    for i in range(n):
        if full:
            lo, hi = 0, n_reg
        else:
            levels = level_sizes(int(nodes[i]), n_reg)
            _, lo, hi = levels[rng.integers(len(levels))]
        bits = rng.random(hi - lo) < rng.uniform(0.5, 1.0)
        bits[rng.integers(hi - lo)] = True
        col = limbs[lo:hi][bits].sum(axis=0)
        sums.append(sum(int(v) << (32 * j) for j, v in enumerate(col)) % ORDER)
        reqs.append((lo, hi - lo, hi - lo, len(words)))
        words.extend(int(x) for x in bits_to_words(bits))
    return np.array(reqs, dtype=REQ_DTYPE), np.array(words, dtype=np.uint64), sums, ks


def main_aggregate(args):
    """--mode aggregate: the cost of giving every AGGREGATE request its own
    message (hg_verify_aggregate_msgs_device). Prints ONE JSON line.

      (a) n requests on n distinct hashable 32-byte messages, the hash beside
          the fold (hg_set_fold_overlap 1) and before it (0)
      (b) the same requests on one message through hg_verify_aggregate_device,
          the context pinned to level 0: the same fold and two-pairing check
      (c) the route before: hg_verify_aggregate_msg with n = 1 per message on
          LOOP messages (host calls, wall clock)
      (d) the hash kernels alone: SUBMIT - AGGREGATE - VERIFY phase time
          (hg_timing_read_phase) of (a) in the sequential order minus (b)'s

    (a) and (b) are device-resident calls timed with HIP events on one stream,
    warm, REPS times each, the three variants alternating; medians, minima and
    maxima are reported, for config 3's level mix and for full-registry
    multisignatures. Every signature is valid and the codes are checked."""
    import torch

    from handel_amd import _lib
    from handel_amd.engine import Engine

    n, n_reg = args.n, args.registry
    dev = torch.device("cuda:0")
    torch.zeros(1, device=dev)
    e = Engine(device=0, flavor="go")
    msgs = hashable_messages(n)
    h = [int.from_bytes(hashlib.sha256(m).digest(), "big") for m in msgs]
    pool, off, ln = e.pack_messages(msgs)
    t = lambda a, dt=torch.uint8: torch.frombuffer(bytearray(bytes(a)), dtype=dt).to(dev)  # noqa: E731
    d_pool, d_off, d_len = t(pool.tobytes()), t(off.tobytes(), torch.int32), t(ln.tobytes(), torch.int32)
    d_codes = torch.full((n,), -1, dtype=torch.int32, device=dev)
    s = torch.cuda.Stream(dev)
    res = {"bench": "verify_aggregate_msgs", "n": n, "registry": n_reg, "reps": args.reps, "message_bytes": 32}
    spread = lambda v: {"median_ms": round(statistics.median(v), 4), "min_ms": round(min(v), 4),  # noqa: E731
                        "max_ms": round(max(v), 4)}
    for mix, full in (("level_mix", False), ("full_registry", True)):
        reqs, words, sums, ks = aggregate_requests(n_reg, n, seed=3, full=full)
        if not full:
            assert not e.registry_load(e.keygen(b"".join(k.to_bytes(32, "big") for k in ks))).any()
            assert e.set_message(msgs[0]) == 0
            e.set_aggregate_level(0)
        # sig_i = (sum sk) H(msg_i) = (sum sk * h_i) G1: one fixed-base launch signs the batch
        sigs_a = e.debug_g1_base_mul([k * hi % ORDER for k, hi in zip(sums, h)])
        sigs_b = e.debug_g1_base_mul([k * h[0] % ORDER for k in sums])
        d_reqs, d_words, d_sa, d_sb = t(reqs.tobytes()), t(words.tobytes()), t(sigs_a), t(sigs_b)

        def run_a():
            e.verify_aggregate_msgs_device(d_pool.data_ptr(), len(pool), d_off.data_ptr(), d_len.data_ptr(),
                                           d_reqs.data_ptr(), n, d_words.data_ptr(), d_sa.data_ptr(),
                                           d_codes.data_ptr(), 0, s.cuda_stream)

        def run_b():
            e.verify_aggregate_device(d_reqs.data_ptr(), n, d_words.data_ptr(), d_sb.data_ptr(), d_codes.data_ptr(), 0,
                                      s.cuda_stream)

        def timed(fn, overlap):
            e.set_fold_overlap(overlap)
            d_codes.fill_(-1)
            torch.cuda.synchronize()
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record(s)
            fn()
            b.record(s)
            b.synchronize()
            assert int((d_codes != 0).sum()) == 0, "every request of the benchmark batch is valid"
            return a.elapsed_time(b)

        variants = (("a_overlap", run_a, True), ("a_sequential", run_a, False), ("b_one_message", run_b, True))
        for _, fn, ov in variants:  # warm: the lazy table, workspaces, the side stream, code objects
            timed(fn, ov)
            timed(fn, ov)
        def rest(fn, overlap):
            """SUBMIT - AGGREGATE - VERIFY ms of one call: what runs on the
            stream besides the fold and the pairing kernel"""
            e.set_fold_overlap(overlap)
            e.timing_enable(True)
            fn()
            s.synchronize()
            ms = [e.timing_read_phase(p)[0] for p in (_lib.HG_PHASE_SUBMIT, _lib.HG_PHASE_AGGREGATE,
                                                      _lib.HG_PHASE_VERIFY)]
            e.timing_enable(False)
            return ms[0] - ms[1] - ms[2]

        times = {name: [] for name, _, _ in variants}
        rests = {name: [] for name, _, _ in variants}
        for _ in range(args.reps):
            for name, fn, ov in variants:
                times[name].append(timed(fn, ov))
            for name, fn, ov in variants:
                rests[name].append(rest(fn, ov))
        e.set_fold_overlap(True)
        out = {name: spread(v) for name, v in times.items()}
        for name, v in rests.items():
            out[name]["rest_ms"] = round(statistics.median(v), 4)
        # (d): the sequential order's rest holds the hash kernels, (b)'s does not
        out["d_hash_kernels_ms"] = round(out["a_sequential"]["rest_ms"] - out["b_one_message"]["rest_ms"], 4)
        b = out["b_one_message"]["median_ms"]
        for name in ("a_overlap", "a_sequential"):
            out[name]["minus_b_ms"] = round(out[name]["median_ms"] - b, 4)
            out[name]["over_b"] = round(out[name]["median_ms"] / b, 4)
            out[name]["requests_per_s"] = round(n / out[name]["median_ms"] * 1e3)
        out["overlap_no_slower"] = bool(out["a_overlap"]["median_ms"] <= out["a_sequential"]["median_ms"])
        res[mix] = out
        if full:
            continue
        # (c) one call per message, on the level mix's first LOOP requests
        loop = min(args.loop, n)
        one = [(msgs[i], reqs[i:i + 1].copy(), sigs_a[64 * i:64 * i + 64]) for i in range(loop)]
        for m, r, sg in one[:8]:
            e.verify_aggregate_msg(m, r, words, sg)
        t0 = time.perf_counter()
        ok = sum(int(e.verify_aggregate_msg(m, r, words, sg)[0] == 0) for m, r, sg in one)
        c_ms = (time.perf_counter() - t0) * 1e3
        assert ok == loop
        res["c_loop"] = {"messages": loop, "ms_per_message": round(c_ms / loop, 4),
                         "scaled_to_n_ms": round(c_ms / loop * n, 2)}
        assert e.set_message(msgs[0]) == 0
    e.close()
    print(json.dumps(res))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--mode", choices=("checks", "aggregate"), default="checks")
    ap.add_argument("--n", type=int, default=4096)
    ap.add_argument("--reps", type=int, default=21)
    ap.add_argument("--loop", type=int, default=256)
    ap.add_argument("--registry", type=int, default=4000, help="aggregate mode: registry keys")
    args = ap.parse_args()
    if args.mode == "aggregate":
        return main_aggregate(args)
    import torch

    from handel_amd import _lib
    from handel_amd.engine import Engine

    n = args.n
    dev = torch.device("cuda:0")
    torch.zeros(1, device=dev)
    e = Engine(device=0, flavor="go")
    msgs = hashable_messages(n)
    h = [int.from_bytes(hashlib.sha256(m).digest(), "big") for m in msgs]
    ks = [int.from_bytes(hashlib.sha256(b"bench-key:%d" % i).digest(), "big") % ORDER or 1 for i in range(n)]
    pks = e.keygen(b"".join(k.to_bytes(32, "big") for k in ks))
    # sig_i = k_i H(msg_i) = (k_i h_i) G1: one fixed-base launch signs the batch
    sigs_a = e.debug_g1_base_mul([k * hi % ORDER for k, hi in zip(ks, h)])
    sigs_b = e.debug_g1_base_mul([k * h[0] % ORDER for k in ks])
    assert e.set_message(msgs[0]) == 0
    pool, off, ln = e.pack_messages(msgs)

    t = lambda a: torch.frombuffer(bytearray(bytes(a)), dtype=torch.uint8).to(dev)  # noqa: E731
    d_pks, d_sa, d_sb, d_pool = t(pks), t(sigs_a), t(sigs_b), t(pool.tobytes())
    d_off = torch.frombuffer(bytearray(off.tobytes()), dtype=torch.int32).to(dev)
    d_len = torch.frombuffer(bytearray(ln.tobytes()), dtype=torch.int32).to(dev)
    d_codes = torch.full((n,), -1, dtype=torch.int32, device=dev)
    s = torch.cuda.Stream(dev)

    def run_a():
        e.verify_batch_msgs_device(d_pool.data_ptr(), len(pool), d_off.data_ptr(), d_len.data_ptr(), d_pks.data_ptr(),
                                   d_sa.data_ptr(), n, d_codes.data_ptr(), s.cuda_stream)

    def run_b():
        e.verify_batch_device(d_pks.data_ptr(), d_sb.data_ptr(), n, d_codes.data_ptr(), s.cuda_stream)

    def timed(fn):
        d_codes.fill_(-1)
        torch.cuda.synchronize()
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record(s)
        fn()
        b.record(s)
        b.synchronize()
        assert int((d_codes != 0).sum()) == 0, "every check of the benchmark batch is valid"
        return a.elapsed_time(b)

    def phases(fn):
        """(SUBMIT - VERIFY) ms of one call: everything but the pairing kernels"""
        e.timing_enable(True)
        fn()
        s.synchronize()
        sub, _ = e.timing_read_phase(_lib.HG_PHASE_SUBMIT)
        ver, _ = e.timing_read_phase(_lib.HG_PHASE_VERIFY)
        e.timing_enable(False)
        return sub - ver

    res = {"bench": "verify_batch_msgs", "n": n, "reps": args.reps, "message_bytes": 32}
    for form, split in (("one_kernel", False), ("split", True)):
        e.set_verify_split(split)
        for fn in (run_a, run_b):  # warm: the lazy table, workspaces, code objects
            timed(fn)
            timed(fn)
        ta, tb, pa, pb = [], [], [], []
        for _ in range(args.reps):
            ta.append(timed(run_a))
            tb.append(timed(run_b))
            pa.append(phases(run_a))
            pb.append(phases(run_b))
        a, b = statistics.median(ta), statistics.median(tb)
        res[form] = {"a_msgs_ms": round(a, 4), "b_one_message_ms": round(b, 4),
                     "a_minus_b_ms": round(a - b, 4), "a_over_b": round(a / b, 4),
                     "a_checks_per_s": round(n / a * 1e3), "b_checks_per_s": round(n / b * 1e3),
                     "d_hash_kernels_ms": round(statistics.median(pa) - statistics.median(pb), 4)}
    e.set_verify_split(False)
    # (c) one call per message
    loop = min(args.loop, n)
    one = [(msgs[i], pks[128 * i:128 * i + 128], sigs_a[64 * i:64 * i + 64]) for i in range(loop)]
    for m, p, sg in one[:8]:
        e.verify_batch_msg(m, p, sg)
    t0 = time.perf_counter()
    ok = sum(int(e.verify_batch_msg(m, p, sg)[0] == 0) for m, p, sg in one)
    c_ms = (time.perf_counter() - t0) * 1e3
    assert ok == loop
    res["c_loop"] = {"messages": loop, "ms_per_message": round(c_ms / loop, 4), "scaled_to_n_ms": round(c_ms / loop * n, 2)}
    t0 = time.perf_counter()
    for _ in range(5):
        _, codes = e.hash_messages_pool(pool, off, ln)
    res["d_hash_messages_call_ms"] = round((time.perf_counter() - t0) * 1e3 / 5, 4)
    assert not codes.any()
    res["a_beats_c"] = bool(res["one_kernel"]["a_msgs_ms"] < res["c_loop"]["scaled_to_n_ms"])
    e.close()
    print(json.dumps(res))


if __name__ == "__main__":
    main()
