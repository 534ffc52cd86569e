"""GPU suite: hg_context_bytes through a context's lifetime.

hg_context_bytes is part of the C ABI (the config-4 proxy reports it), and it
is the sum of what the context's buffer owners hold (handel_amd/csrc/hg_ctx.h,
hg_dev.h). This test walks one context through every owner at the smallest
sizes that touch it — a 64-key registry, two messages each prepared to table
level 2, a 64-request aggregate batch under each, a lane (max_batch 64) created,
used and destroyed, a store set (2 receivers, 64 packets, merge on) created and
destroyed, a table budget for one message's tables — and records the figure
after each step. Three fresh contexts in one process must give the same
sequence (nothing leaks into or out of the count), and a live lane must count.
The absolute values are not pinned here.

Run as a script it prints the sequence as one JSON line (HG_LIB selects the
library), for comparing two builds.
"""

import ctypes
import hashlib
import json
import os
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

from handel_amd.engine import REQ_DTYPE, DeviceLane, Engine, Stores  # noqa: E402

pytestmark = pytest.mark.gpu

N = 64
MESSAGES = (b"Everything that is beautiful and noble is the product of reason and calculation.", b"Get Funky Tonight")
GT_BYTES = 480  # one GT element: 12 x 10 limbs of 4 bytes
# one message's level-2 tables of 64 keys (4 windows of 2^16 products) with
# room for its level-1 tables (< 300 elements per key), not for a second set
ONE_MESSAGE_BUDGET = N // 16 * 65536 * GT_BYTES + N * 300 * GT_BYTES
STEPS = ("create", "registry", "tables A", "tables B", "batch B", "batch A", "lane", "lane destroyed", "stores",
         "stores destroyed", "budget")


def _material():
    """64 keys and, per message, each key's signature as a one-signer multisig
    over the whole registry (request i: bit i of its own bitset word)."""
    # 248-bit scalars: nonzero and below the group order
    scalars = b"".join(b"\x00" + hashlib.sha256(b"context-bytes %d" % i).digest()[1:] for i in range(N))
    e = Engine(device=0, flavor="go")
    try:
        pks = e.keygen(scalars)
        sigs = [e.sign_msg(m, scalars) for m in MESSAGES]
    finally:
        e.close()
    reqs = np.array([(0, N, N, i) for i in range(N)], dtype=REQ_DTYPE)
    words = np.array([1 << i for i in range(N)], dtype=np.uint64)
    return pks, sigs, reqs, words


def _lane_batch(e, lane, reqs, words, sigs):
    """One host-staged batch through the lane's pinned buffers."""
    L, p = e.L, [ctypes.c_void_p() for _ in range(3)]
    e._check(L.hg_lane_stage(lane.h, len(reqs), len(words), *map(ctypes.byref, p)), "hg_lane_stage")
    for dst, src in zip(p, (reqs.tobytes(), sigs, words.tobytes())):
        ctypes.memmove(dst, src, len(src))
    e._check(L.hg_lane_submit(lane.h), "hg_lane_submit")
    lane.wait()
    return [L.hg_lane_codes(lane.h)[i] for i in range(len(reqs))]


def lifetime(material):
    pks, sigs, reqs, words = material
    e = Engine(device=0, flavor="go")
    seq = []
    try:
        e.set_aggregate_level(2)
        seq.append(e.context_bytes())
        assert not e.registry_load(pks).any()
        seq.append(e.context_bytes())
        for m in MESSAGES:
            assert e.prepare_aggregate_msg(m) == 0 and e.aggregate_tables() == 2
            seq.append(e.context_bytes())
        for k in (1, 0):
            assert not e.verify_aggregate_msg(MESSAGES[k], reqs, words, sigs[k]).any()
            assert e.aggregate_tables() == 2  # the cached message kept its tables
            seq.append(e.context_bytes())
        lane = DeviceLane(e, N)
        assert _lane_batch(e, lane, reqs, words, sigs[0]) == [0] * N
        seq.append(e.context_bytes())
        lane.close()
        seq.append(e.context_bytes())
        st = Stores(e, [0, 5], N)
        st.enable_merge()
        seq.append(e.context_bytes())
        st.close()
        seq.append(e.context_bytes())
        e.set_table_budget(ONE_MESSAGE_BUDGET)
        assert e.aggregate_tables() == 2
        seq.append(e.context_bytes())
    finally:
        e.close()
    assert len(seq) == len(STEPS)
    return seq


def test_context_bytes_repeat_over_fresh_contexts():
    material = _material()
    runs = [lifetime(material) for _ in range(3)]
    print("context bytes:", dict(zip(STEPS, runs[0])))
    assert runs[1] == runs[0] and runs[2] == runs[0]
    at = dict(zip(STEPS, runs[0]))
    assert at["lane"] > at["lane destroyed"]  # a live lane's workspaces count, a destroyed one's do not
    assert at["budget"] < at["stores destroyed"]  # the budget holds one message's tables: the cached one's went
    assert all(b >= a for a, b in zip(runs[0][:6], runs[0][1:6]))  # nothing shrinks while the context only grows


if __name__ == "__main__":
    print(json.dumps(lifetime(_material())))
