#!/usr/bin/env python3
"""Exact against combined verification of independent checks on arbitrary keys,
interleaved in one process.

n distinct keys, each with a valid signature: on one message (the context's:
hg_verify_batch_device against hg_verify_batch_rlc_device) and on a hashable
32-byte message each (hg_verify_batch_msgs_device against
hg_verify_batch_msgs_rlc_device). Keys, messages and signatures are resident on
the device; the exact call (the yardstick, in the context's default form) and
the combined call (group 64) run on one context and one stream, alternating
call by call. Shapes: all valid with n = 4096, 16384 and 65536, then n = 4096
with 1 % of the signatures tampered.

Per shape and form: the wall time of a call from submission to an idle stream
(median of --reps, minimum too), the phases of hg_timing_read_phase for both
calls, and hg_batch_rlc_stats. One JSON document, by default
profiles/batch_rlc_bench.json.

    python tools/batch_rlc_bench.py [--out FILE] [--reps 7] [--quick]

The three Miller kernels on 4096 checks (k_brlc_miller here, k_verify_ml<4>
through the split form of hg_verify_batch_device, k_mrlc_miller through
hg_verify_aggregate_msgs_rlc_device) are timed by a kernel trace in a run of its
own:

    rocprofv3 --kernel-trace --stats -f csv -d DIR -- python tools/batch_rlc_bench.py --kernels
    python tools/batch_rlc_bench.py --kernel-stats DIR   # the bench, with the trace's rows in the document
"""

import argparse
import csv
import glob
import hashlib
import json
import os
import re
import statistics
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))

import aggmsgs_rlc_bench as A  # noqa: E402
import bench_msgs  # noqa: E402
from handel_amd import _lib  # noqa: E402
from handel_amd.engine import Engine  # noqa: E402

ORDER = bench_msgs.ORDER
GROUP = 64
MSG = b"batch-rlc-bench: the one message"
KERNELS = ("k_brlc_miller", "k_mrlc_miller", "k_verify_ml", "k_verify", "k_msgs_verify", "k_mrlc_product",
           "k_mrlc_scalars", "k_rlc_g1_mul", "k_rlc_g1_sum", "k_hash_points", "k_sig12_fe", "k_decode_checks",
           "k_brlc_members", "k_brlc_one_message")


def secret(i):
    return int.from_bytes(hashlib.sha256(b"batch-rlc-key:%d" % i).digest(), "big") % ORDER or 1


class Batch:
    """n checks on distinct keys, on the device: one signature set per form."""

    def __init__(self, torch, dev, e, n, seed, msgs, tampered=0):
        ks = [secret(i) for i in range(n)]
        rng = np.random.default_rng(seed)
        bad = set(int(i) for i in rng.choice(n, size=tampered, replace=False)) if tampered else set()
        h1 = int.from_bytes(hashlib.sha256(MSG).digest(), "big")
        h = [int.from_bytes(hashlib.sha256(m).digest(), "big") for m in msgs[:n]]
        # sig_i = sk_i H(msg) = (sk_i h) G1, + G1 when tampered: one fixed-base launch per form
        one = e.debug_g1_base_mul([(k * h1 + (i in bad)) % ORDER for i, k in enumerate(ks)])
        own = e.debug_g1_base_mul([(k * hi + (i in bad)) % ORDER for i, (k, hi) in enumerate(zip(ks, h))])
        pool, off, ln = e.pack_messages(msgs[:n])
        t = lambda a, dt=torch.uint8: torch.frombuffer(bytearray(bytes(a)), dtype=dt).to(dev)  # noqa: E731
        self.n, self.pool_len = n, len(pool)
        self.pks = t(e.keygen(b"".join(k.to_bytes(32, "big") for k in ks)))
        self.sigs = {"one": t(one), "msgs": t(own)}
        self.msgs = (t(pool.tobytes()), t(off.tobytes(), torch.int32), t(ln.tobytes(), torch.int32))
        self.codes = torch.full((n,), -7, dtype=torch.int32, device=dev)
        self.expect = np.zeros(n, dtype=np.int32)
        self.expect[sorted(bad)] = _lib.HG_ERR_SIG_INVALID
        torch.cuda.synchronize(dev)

    def args(self, form):
        base = (self.pks.data_ptr(), self.sigs[form].data_ptr(), self.n, self.codes.data_ptr())
        if form == "one":
            return base
        p, o, l = self.msgs
        return (p.data_ptr(), self.pool_len, o.data_ptr(), l.data_ptr()) + base


def run_shape(e, stream, b, form, reps, name):
    def exact():
        if form == "one":
            e.verify_batch_device(*b.args(form), stream.cuda_stream)
        else:
            e.verify_batch_msgs_device(*b.args(form), stream.cuda_stream)
        stream.synchronize()

    def rlc():
        if form == "one":
            e.verify_batch_rlc_device(*b.args(form), seed=None, group=GROUP, stream=stream.cuda_stream)
        else:
            e.verify_batch_msgs_rlc_device(*b.args(form), seed=None, group=GROUP, stream=stream.cuda_stream)
        stream.synchronize()

    for _ in range(2):  # warm-up, and the verdicts
        exact()
        assert (b.codes.cpu().numpy() == b.expect).all(), (name, form)
        rlc()
        assert (b.codes.cpu().numpy() == b.expect).all(), (name, form)
    stats = e.batch_rlc_stats()
    ex, rl = [], []
    for _ in range(reps):  # interleaved
        ex.append(A.timed(exact))
        rl.append(A.timed(rlc))
    out = {"name": name, "form": form, "n": b.n, "group": GROUP, "tampered": int((b.expect != 0).sum()),
           "rlc_stats": {"groups": stats[0], "groups_failed": stats[1], "rechecked": stats[2], "non_g2": stats[3]},
           "one_batch_ms": {"exact_median": round(statistics.median(ex), 4), "exact_min": round(min(ex), 4),
                            "rlc_median": round(statistics.median(rl), 4), "rlc_min": round(min(rl), 4)},
           "phases_exact": A.phases(e, exact), "phases_rlc": A.phases(e, rlc)}
    o = out["one_batch_ms"]
    out["rlc_over_exact"] = round(o["rlc_median"] / o["exact_median"], 3)
    print(json.dumps(out), flush=True)
    return out


def kernel_rows(path):
    """The named kernels' rows of a kernel trace's statistics (every *kernel_stats.csv under path)."""
    out = {}
    for f in sorted(glob.glob(os.path.join(path, "**", "*kernel_stats.csv"), recursive=True)):
        with open(f, newline="") as fh:
            for row in csv.DictReader(fh):
                for k in KERNELS:
                    if re.search(r"\b%s(?![A-Za-z0-9_])" % k, row.get("Name", "")):
                        out[k] = {"calls": int(row["Calls"]), "average_us": round(float(row["AverageNs"]) / 1e3, 2),
                                  "min_us": round(float(row["MinNs"]) / 1e3, 2),
                                  "max_us": round(float(row["MaxNs"]) / 1e3, 2)}
    return out


def kernels_mode(args):
    """The three Miller kernels on 4096 checks each, five calls per form: for a kernel trace."""
    import torch

    args.keys = 4000
    dev, e, _ = A.setup(args, torch)  # a registry, for k_mrlc_miller
    n = 4096
    msgs = bench_msgs.hashable_messages(n)
    s = torch.cuda.Stream(device=dev)
    agg = A.Batch(torch, dev, e, args.keys, n, 11, msgs)
    b = Batch(torch, dev, e, n, 11, msgs)
    assert e.set_message(MSG) == 0
    for _ in range(5):
        for split in (False, True):  # k_verify<4>, then k_verify_ml<4> and the 12-lane final exponentiation
            e.set_verify_split(split)
            e.verify_batch_device(*b.args("one"), s.cuda_stream)
            s.synchronize()
            assert not b.codes.cpu().numpy().any()
        e.set_verify_split(False)
        e.verify_batch_msgs_device(*b.args("msgs"), s.cuda_stream)
        e.verify_batch_rlc_device(*b.args("one"), seed=None, group=GROUP, stream=s.cuda_stream)
        e.verify_batch_msgs_rlc_device(*b.args("msgs"), seed=None, group=GROUP, stream=s.cuda_stream)
        s.synchronize()
        assert not b.codes.cpu().numpy().any()
        e.verify_aggregate_msgs_rlc_device(*agg.args(), seed=None, group=GROUP, stream=s.cuda_stream)
        s.synchronize()
        assert not agg.codes.cpu().numpy().any()
    e.close()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "batch_rlc_bench.json"))
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--quick", action="store_true", help="n = 4096, all valid, only")
    ap.add_argument("--kernels", action="store_true", help="run the three Miller kernels for a kernel trace, no timing")
    ap.add_argument("--kernel-stats", help="directory of that trace: its rows go into the document")
    args = ap.parse_args()
    if args.kernels:
        return kernels_mode(args)
    import torch

    dev = torch.device("cuda", 0)
    torch.zeros(1, device=dev)
    e = Engine(device=0, flavor="go")
    assert e.set_message(MSG) == 0
    stream = torch.cuda.Stream(device=dev)
    big = 4096 if args.quick else 65536
    msgs = bench_msgs.hashable_messages(big)
    shapes = []
    doc = {"tool": "tools/batch_rlc_bench.py", "reps": args.reps, "group": GROUP,
           "device": torch.cuda.get_device_name(0), "shapes": shapes}
    plan = [(4096, 11, 0, "all valid")]
    if not args.quick:
        plan += [(16384, 14, 0, "all valid"), (big, 13, 0, "all valid"), (4096, 12, 41, "1 % tampered")]
    for n, seed, tampered, name in plan:
        b = Batch(torch, dev, e, n, seed, msgs, tampered=tampered)
        for form in ("one", "msgs"):
            shapes.append(run_shape(e, stream, b, form, args.reps, name))
        del b
    if args.kernel_stats:
        doc["kernels_4096_checks"] = kernel_rows(args.kernel_stats)
    with open(args.out, "w") as f:
        json.dump(doc, f, indent=1)
        f.write("\n")
    e.close()


if __name__ == "__main__":
    main()
