#!/usr/bin/env python3
"""Exact against combined verification of aggregate requests that each carry
their own message, interleaved in one process.

A 4000-key registry; config 3's requests (tools/bench_msgs.py
aggregate_requests), each on its own hashable 32-byte message; requests,
messages and signatures resident on the device. hg_verify_aggregate_msgs_device
(the yardstick) and hg_verify_aggregate_msgs_rlc_device (group 64) run on one
context and one stream, alternating call by call. Shapes: all valid with
n = 4096, 16384 and 65536, then n = 4096 with 1 % of the signatures tampered.

Per shape: the wall time of a call from submission to an idle stream (median of
--reps, minimum too), the phases of hg_timing_read_phase for both forms, and
hg_rlc_stats. One JSON document, by default profiles/aggmsgs_rlc_bench.json.

    python tools/aggmsgs_rlc_bench.py [--out FILE] [--reps 7] [--keys 4000] [--quick]

The three Miller kernels on the same number of checks (k_mrlc_miller here,
k_verify_ml<4> and k_msgs_miller through the split forms of hg_verify_batch_device
and hg_verify_batch_msgs_device) are timed by a kernel trace in a run of its own:

    rocprofv3 --kernel-trace --stats -d DIR -- python tools/aggmsgs_rlc_bench.py --kernels
    python tools/aggmsgs_rlc_bench.py --kernel-stats DIR   # the bench, with the trace's rows in the document
"""

import argparse
import csv
import glob
import hashlib
import json
import os
import statistics
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))

import bench_msgs  # noqa: E402
from handel_amd import _lib  # noqa: E402
from handel_amd.engine import Engine  # noqa: E402

ORDER = bench_msgs.ORDER
PHASES = {"verify": _lib.HG_PHASE_VERIFY, "aggregate": _lib.HG_PHASE_AGGREGATE, "submit": _lib.HG_PHASE_SUBMIT}
KERNELS = ("k_mrlc_miller", "k_verify_ml", "k_msgs_miller", "k_msgs_verify", "k_mrlc_product", "k_mrlc_scalars",
           "k_rlc_g1_mul", "k_rlc_g1_sum", "k_hash_points", "k_sig12_fe")
GROUP = 64


class Batch:
    """n requests, their messages and signatures on the device."""

    def __init__(self, torch, dev, e, n_reg, n, seed, msgs, tampered=0):
        reqs, words, sums, _ = bench_msgs.aggregate_requests(n_reg, n, seed=seed, full=False)
        h = [int.from_bytes(hashlib.sha256(m).digest(), "big") for m in msgs[:n]]
        rng = np.random.default_rng(seed)
        bad = set(int(i) for i in rng.choice(n, size=tampered, replace=False)) if tampered else set()
        # sig_i = (sum sk) H(msg_i) = (sum sk * h_i) G1, + G1 when tampered: one fixed-base launch
        sigs = e.debug_g1_base_mul([(k * hi + (i in bad)) % ORDER for i, (k, hi) in enumerate(zip(sums, h))])
        pool, off, ln = e.pack_messages(msgs[:n])
        t = lambda a, dt=torch.uint8: torch.frombuffer(bytearray(bytes(a)), dtype=dt).to(dev)  # noqa: E731
        self.n, self.pool_len = n, len(pool)
        self.bufs = (t(pool.tobytes()), t(off.tobytes(), torch.int32), t(ln.tobytes(), torch.int32),
                     t(reqs.tobytes()), t(words.tobytes()), t(sigs))
        self.codes = torch.full((n,), -7, dtype=torch.int32, device=dev)
        self.expect = np.zeros(n, dtype=np.int32)
        self.expect[sorted(bad)] = _lib.HG_ERR_SIG_INVALID
        torch.cuda.synchronize(dev)

    def args(self):
        p, o, l, r, w, s = self.bufs
        return (p.data_ptr(), self.pool_len, o.data_ptr(), l.data_ptr(), r.data_ptr(), self.n, w.data_ptr(),
                s.data_ptr(), self.codes.data_ptr())


def timed(fn):
    t0 = time.perf_counter()
    fn()
    return (time.perf_counter() - t0) * 1e3


def phases(e, fn, reps=3):
    e.timing_enable(True)
    for p in PHASES.values():
        e.timing_read_phase(p)
    for _ in range(reps):
        fn()
    out = {}
    for name, p in PHASES.items():
        ms, cnt = e.timing_read_phase(p)
        out[name] = {"ms_per_call": round(ms / reps, 4), "intervals_per_call": cnt / reps}
    e.timing_enable(False)
    return out


def run_shape(e, stream, b, reps, name):
    def exact():
        e.verify_aggregate_msgs_device(*b.args(), 0, stream.cuda_stream)
        stream.synchronize()

    def rlc():
        e.verify_aggregate_msgs_rlc_device(*b.args(), seed=None, group=GROUP, stream=stream.cuda_stream)
        stream.synchronize()

    for _ in range(2):  # warm-up, and the verdicts
        exact()
        assert (b.codes.cpu().numpy() == b.expect).all(), name
        rlc()
        assert (b.codes.cpu().numpy() == b.expect).all(), name
    stats = e.rlc_stats()
    ex, rl = [], []
    for _ in range(reps):  # interleaved
        ex.append(timed(exact))
        rl.append(timed(rlc))
    out = {"name": name, "n": b.n, "group": GROUP, "tampered": int((b.expect != 0).sum()),
           "rlc_stats": {"groups": stats[0], "groups_failed": stats[1], "rechecked": stats[2]},
           "one_batch_ms": {"exact_median": round(statistics.median(ex), 4), "exact_min": round(min(ex), 4),
                            "rlc_median": round(statistics.median(rl), 4), "rlc_min": round(min(rl), 4)},
           "phases_exact": phases(e, exact), "phases_rlc": phases(e, rlc)}
    o = out["one_batch_ms"]
    out["rlc_over_exact"] = round(o["rlc_median"] / o["exact_median"], 3)
    print(json.dumps(out), flush=True)
    return out


def setup(args, torch):
    dev = torch.device("cuda", 0)
    torch.zeros(1, device=dev)
    e = Engine(device=0, flavor="go")
    ks = [int.from_bytes(hashlib.sha256(b"bench-agg-key:%d" % i).digest(), "big") % ORDER or 1
          for i in range(args.keys)]  # bench_msgs.aggregate_requests' keys
    assert not e.registry_load(e.keygen(b"".join(k.to_bytes(32, "big") for k in ks))).any()
    assert e.registry_non_g2() == 0
    return dev, e, ks


def kernels_mode(args):
    """The three Miller kernels on 4096 checks each, five calls per form: for a kernel trace."""
    import torch

    dev, e, ks = setup(args, torch)
    n = 4096
    msgs = bench_msgs.hashable_messages(n)
    s = torch.cuda.Stream(device=dev)
    b = Batch(torch, dev, e, args.keys, n, 11, msgs)
    # single checks on the same number of (key, signature) pairs, one message and n messages
    h = [int.from_bytes(hashlib.sha256(m).digest(), "big") for m in msgs]
    sk = [ks[i % len(ks)] for i in range(n)]
    pks = e.keygen(b"".join(k.to_bytes(32, "big") for k in sk))
    t = lambda a: torch.frombuffer(bytearray(bytes(a)), dtype=torch.uint8).to(dev)  # noqa: E731
    d_pks = t(pks)
    d_one = t(e.debug_g1_base_mul([k * h[0] % ORDER for k in sk]))
    d_own = t(e.debug_g1_base_mul([k * hi % ORDER for k, hi in zip(sk, h)]))
    assert e.set_message(msgs[0]) == 0
    e.set_verify_split(True)
    p, o, l = b.bufs[:3]
    for _ in range(5):
        e.verify_batch_device(d_pks.data_ptr(), d_one.data_ptr(), n, b.codes.data_ptr(), s.cuda_stream)
        s.synchronize()
        assert not b.codes.cpu().numpy().any()
        e.verify_batch_msgs_device(p.data_ptr(), b.pool_len, o.data_ptr(), l.data_ptr(), d_pks.data_ptr(),
                                   d_own.data_ptr(), n, b.codes.data_ptr(), s.cuda_stream)
        s.synchronize()
        assert not b.codes.cpu().numpy().any()
        e.verify_aggregate_msgs_device(*b.args(), 0, s.cuda_stream)
        e.verify_aggregate_msgs_rlc_device(*b.args(), seed=None, group=GROUP, stream=s.cuda_stream)
        s.synchronize()
        assert not b.codes.cpu().numpy().any()
    e.close()


def kernel_rows(path):
    """The named kernels' rows of a kernel trace's statistics (every *kernel_stats.csv under path)."""
    out = {}
    for f in sorted(glob.glob(os.path.join(path, "**", "*kernel_stats.csv"), recursive=True)):
        with open(f, newline="") as fh:
            for row in csv.DictReader(fh):
                name = row.get("Name", "")
                for k in KERNELS:
                    if k in name:
                        out[k] = {"calls": int(row["Calls"]), "average_us": round(float(row["AverageNs"]) / 1e3, 2),
                                  "min_us": round(float(row["MinNs"]) / 1e3, 2),
                                  "max_us": round(float(row["MaxNs"]) / 1e3, 2)}
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "aggmsgs_rlc_bench.json"))
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--keys", type=int, default=4000)
    ap.add_argument("--quick", action="store_true", help="n = 4096, all valid, only")
    ap.add_argument("--kernels", action="store_true", help="run the three Miller kernels for a kernel trace, no timing")
    ap.add_argument("--kernel-stats", help="directory of that trace: its rows go into the document")
    args = ap.parse_args()
    if args.kernels:
        return kernels_mode(args)
    import torch

    dev, e, _ = setup(args, torch)
    stream = torch.cuda.Stream(device=dev)
    big = 4096 if args.quick else 65536
    msgs = bench_msgs.hashable_messages(big)
    shapes = []
    doc = {"tool": "tools/aggmsgs_rlc_bench.py", "keys": args.keys, "reps": args.reps, "group": GROUP,
           "device": torch.cuda.get_device_name(0), "shapes": shapes}
    shapes.append(run_shape(e, stream, Batch(torch, dev, e, args.keys, 4096, 11, msgs), args.reps, "all valid"))
    if not args.quick:
        for n, seed in ((16384, 14), (big, 13)):  # 16384: between the two, to place the break-even
            shapes.append(run_shape(e, stream, Batch(torch, dev, e, args.keys, n, seed, msgs), args.reps,
                                    "all valid"))
        shapes.append(run_shape(e, stream, Batch(torch, dev, e, args.keys, 4096, 12, msgs, tampered=41), args.reps,
                                "1 % tampered"))
    if args.kernel_stats:
        doc["kernels_4096_checks"] = kernel_rows(args.kernel_stats)
    with open(args.out, "w") as f:
        json.dump(doc, f, indent=1)
        f.write("\n")
    e.close()


if __name__ == "__main__":
    main()
