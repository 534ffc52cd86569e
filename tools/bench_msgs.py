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


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=4096)
    ap.add_argument("--reps", type=int, default=21)
    ap.add_argument("--loop", type=int, default=256)
    args = ap.parse_args()
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
