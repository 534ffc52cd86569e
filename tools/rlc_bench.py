#!/usr/bin/env python3
"""Exact against combined aggregate verification, interleaved in one process.

Config 3's requests (a 4000-key registry, a random node's random level, bitset
density U[0.5, 1.0], the set keys' aggregate signature) go through
hg_verify_aggregate_device and hg_verify_aggregate_rlc_device on the same
context, same buffers, alternating call by call; the exact path is the baseline.
Batches: all valid with n = 4096 and group 16 / 64 / 256, all valid with
n = 65536, and n = 4096 with 1 % of the signatures tampered. Each shape runs one
batch at a time and with four contexts' batches in flight (one host thread per
context: the combined form reads a count back, so it blocks its caller).

Per shape: the median wall time of a call (submit to stream idle), the phases of
hg_timing_read_phase for both forms, and hg_rlc_stats. One JSON document, by
default profiles/rlc_bench.json.

    python tools/rlc_bench.py [--out FILE] [--reps 15] [--keys 4000] [--quick]
"""

import argparse
import json
import os
import statistics
import sys
import threading
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from handel_amd import _lib  # noqa: E402
from handel_amd.engine import REQ_DTYPE, Engine  # noqa: E402
from handel_amd.partitioner import bits_to_words, level_sizes  # noqa: E402

ORDER = 65000549695646603732796438742359905742570406053903786389881062969044166799969
MSG = b"rlc bench message"
P = 65000549695646603732796438742359905742825358107623003571877145026864184071783
G1_GEN = (1).to_bytes(32, "big") + (P - 2).to_bytes(32, "big")  # the generator's marshal
PHASES = {"verify": _lib.HG_PHASE_VERIFY, "aggregate": _lib.HG_PHASE_AGGREGATE, "submit": _lib.HG_PHASE_SUBMIT}


def scalars(n, seed):
    rng = np.random.default_rng(seed)
    out = bytearray()
    while len(out) < 32 * n:
        k = int.from_bytes(rng.bytes(32), "big")
        if 0 < k < ORDER:
            out += k.to_bytes(32, "big")
    return bytes(out)


def make_requests(eng, kb, n_reg, n, seed, tampered=0):
    """n config-3 requests, every signature valid but `tampered` of them (+ G1)."""
    rng = np.random.default_rng(seed)
    limbs = np.frombuffer(kb, dtype=">u4").reshape(n_reg, 8)[:, ::-1].astype(np.int64)
    reqs, words, sc = [], [], bytearray()
    nodes = rng.integers(0, n_reg, size=n)
    for i in range(n):
        levels = level_sizes(int(nodes[i]), n_reg)
        _, lo, hi = levels[rng.integers(len(levels))]
        bits = rng.random(hi - lo) < rng.uniform(0.5, 1.0)
        bits[rng.integers(hi - lo)] = True
        col = limbs[lo:hi][bits].sum(axis=0)
        k = sum(int(v) << (32 * j) for j, v in enumerate(col)) % ORDER
        reqs.append((lo, hi - lo, hi - lo, len(words)))
        words.extend(int(x) for x in bits_to_words(bits))
        sc += (k or 1).to_bytes(32, "big")
    sigs = bytearray(eng.sign(bytes(sc)))
    expect = np.zeros(n, dtype=np.int32)
    if tampered:
        idx = sorted(int(i) for i in rng.choice(n, size=tampered, replace=False))
        bad, codes = eng.combine_g1(b"".join(bytes(sigs[64 * i:64 * i + 64]) for i in idx), G1_GEN * len(idx))
        assert not codes.any()
        for j, i in enumerate(idx):
            sigs[64 * i:64 * i + 64] = bad[64 * j:64 * j + 64]
        expect[idx] = _lib.HG_ERR_SIG_INVALID
    return np.array(reqs, dtype=REQ_DTYPE), np.array(words, dtype=np.uint64), bytes(sigs), expect


class Ctx:
    """One context with the registry's tables and a batch resident on the device."""

    def __init__(self, torch, dev, reg, overlap=True):
        self.torch, self.dev = torch, dev
        self.eng = Engine(device=0, flavor="go")
        assert not self.eng.registry_load(reg).any()
        assert self.eng.prepare_aggregate_msg(MSG) == 0
        self.eng.set_fold_overlap(overlap)
        self.stream = torch.cuda.Stream(device=dev)

    def put(self, reqs, words, sigs):
        t = self.torch
        up = lambda b: t.frombuffer(bytearray(b), dtype=t.uint8).to(self.dev)  # noqa: E731
        self.n = len(reqs)
        self.bufs = (up(reqs.tobytes()), up(words.tobytes()), up(sigs))
        self.codes = t.full((self.n,), -7, dtype=t.int32, device=self.dev)
        t.cuda.synchronize(self.dev)

    def exact(self):
        r, w, s = self.bufs
        self.eng.verify_aggregate_device(r.data_ptr(), self.n, w.data_ptr(), s.data_ptr(), self.codes.data_ptr(),
                                         stream=self.stream.cuda_stream)
        self.stream.synchronize()

    def rlc(self, group):
        r, w, s = self.bufs
        self.eng.verify_aggregate_rlc_device(r.data_ptr(), self.n, w.data_ptr(), s.data_ptr(), self.codes.data_ptr(),
                                             seed=None, group=group, stream=self.stream.cuda_stream)
        self.stream.synchronize()

    def got(self):
        return self.codes.cpu().numpy()


def timed(fn):
    t0 = time.perf_counter()
    fn()
    return (time.perf_counter() - t0) * 1e3


def phases(ctx, fn, reps=3):
    ctx.eng.timing_enable(True)
    for p in PHASES.values():
        ctx.eng.timing_read_phase(p)
    for _ in range(reps):
        fn()
    out = {}
    for name, p in PHASES.items():
        ms, cnt = ctx.eng.timing_read_phase(p)
        out[name] = {"ms_per_call": round(ms / reps, 4), "intervals_per_call": cnt / reps}
    ctx.eng.timing_enable(False)
    return out


def in_flight(ctxs, fn_of, reps):
    """every context runs `reps` calls on its own thread; returns ms per batch of the whole"""
    barrier = threading.Barrier(len(ctxs) + 1)

    def work(c):
        barrier.wait()
        for _ in range(reps):
            fn_of(c)()

    ts = [threading.Thread(target=work, args=(c,)) for c in ctxs]
    for t in ts:
        t.start()
    barrier.wait()
    t0 = time.perf_counter()
    for t in ts:
        t.join()
    return (time.perf_counter() - t0) * 1e3 / (reps * len(ctxs))


def run_shape(ctxs, batch, expect, group, reps, name):
    for c in ctxs:
        c.put(*batch)
    c0 = ctxs[0]
    for _ in range(2):  # warm-up, and the verdicts
        c0.exact()
        assert (c0.got() == expect).all(), name
        c0.rlc(group)
        assert (c0.got() == expect).all(), name
    stats = c0.eng.rlc_stats()
    ex, rl = [], []
    for _ in range(reps):  # interleaved
        ex.append(timed(c0.exact))
        rl.append(timed(lambda: c0.rlc(group)))
    out = {"name": name, "n": int(c0.n), "group": group, "tampered": int((expect != 0).sum()),
           "rlc_stats": {"groups": stats[0], "groups_failed": stats[1], "rechecked": stats[2]},
           "one_batch_ms": {"exact_median": round(statistics.median(ex), 4), "exact_min": round(min(ex), 4),
                            "rlc_median": round(statistics.median(rl), 4), "rlc_min": round(min(rl), 4)},
           "phases_exact": phases(c0, c0.exact), "phases_rlc": phases(c0, lambda: c0.rlc(group))}
    if len(ctxs) > 1:
        for c in ctxs[1:]:
            c.exact(), c.rlc(group)
        out["in_flight_%d_ms_per_batch" % len(ctxs)] = {
            "exact": round(in_flight(ctxs, lambda c: c.exact, reps), 4),
            "rlc": round(in_flight(ctxs, lambda c: (lambda: c.rlc(group)), reps), 4)}
    o = out["one_batch_ms"]
    out["rlc_over_exact_one_batch"] = round(o["rlc_median"] / o["exact_median"], 3)
    print(json.dumps(out), flush=True)
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "rlc_bench.json"))
    ap.add_argument("--reps", type=int, default=15)
    ap.add_argument("--keys", type=int, default=4000)
    ap.add_argument("--contexts", type=int, default=4)
    ap.add_argument("--quick", action="store_true", help="n = 4096, group 64 only")
    args = ap.parse_args()
    import torch

    dev = torch.device("cuda", 0)
    torch.zeros(1, device=dev)
    kb = scalars(args.keys, 3)
    first = Engine(device=0, flavor="go")
    reg = first.keygen(kb)
    first.set_message(MSG)
    t0 = time.perf_counter()
    ctxs = [Ctx(torch, dev, reg) for _ in range(args.contexts)]
    build_s = time.perf_counter() - t0
    c0 = ctxs[0]
    small = make_requests(first, kb, args.keys, 4096, 11)
    shapes = []
    doc = {"tool": "tools/rlc_bench.py", "keys": args.keys, "contexts": args.contexts, "reps": args.reps,
           "table_level": c0.eng.aggregate_tables(), "torus": bool(c0.eng.aggregate_tables_torus()),
           "device": torch.cuda.get_device_name(0), "tables_build_s": round(build_s, 2), "shapes": shapes}
    for group in ((64,) if args.quick else (16, 64, 256)):
        shapes.append(run_shape(ctxs, small[:3], small[3], group, args.reps, "all valid"))
    if not args.quick:
        bad = make_requests(first, kb, args.keys, 4096, 12, tampered=41)
        shapes.append(run_shape(ctxs, bad[:3], bad[3], 64, args.reps, "1 % tampered"))
        big = make_requests(first, kb, args.keys, 65536, 13)
        for group in (64, 256):
            shapes.append(run_shape(ctxs, big[:3], big[3], group, max(3, args.reps // 3), "all valid"))
    with open(args.out, "w") as f:
        json.dump(doc, f, indent=1)
        f.write("\n")
    for c in ctxs:
        c.eng.close()
    first.close()


if __name__ == "__main__":
    main()
