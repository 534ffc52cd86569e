"""CPU suite for the standing queue (hg_stores_pool_*, handel_amd/intake.py
PoolModel): the model the GPU pool is tested against is held to
BatchedEvaluatorProcessing.read_todos with EvaluatorStore on a host Store, the
new entry points are declared, exported and bound, and they refuse a NULL
handle before touching a device."""

import ctypes
import os
import random
import re

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

POOL_SYMBOLS = ("hg_stores_pool_create", "hg_stores_pool_destroy", "hg_stores_pool_bytes",
                "hg_stores_pool_append_device", "hg_stores_pool_select_capacity", "hg_stores_pool_step_device",
                "hg_stores_pool_count", "hg_stores_pool_read", "hg_stores_pool_clear")


def _steps(nreg, receivers, rnd, steps=4, per_step=36):
    """Per step a list of (receiver, IncomingSig) in arrival order. Every
    packet arrives two or three times (its copies spread over the step), so
    equal marks are common; about half carry an individual signature."""
    from handel_amd import partitioner as HP
    from handel_amd.sigprocessing import IncomingSig, MultiSig

    out = []
    for _ in range(steps):
        arrivals = []
        for _ in range(per_step):
            r = rnd.choice(receivers)
            lv, lo, hi = rnd.choice(HP.level_sizes(r, nreg))
            size = hi - lo
            origin = lo + rnd.randrange(size)
            bits = 1 << (origin - lo)
            for j in range(size):
                if rnd.random() < rnd.choice([0.15, 0.5, 0.9]):
                    bits |= 1 << j
            has_ind = rnd.random() < 0.5
            for _ in range(rnd.choice([2, 3])):
                arrivals.append((rnd.random(), r, origin, lv, size, bits, lo, has_ind))
        arrivals.sort(key=lambda a: a[0])
        step = []
        for _, r, origin, lv, size, bits, lo, has_ind in arrivals:
            step.append((r, IncomingSig(origin, lv, MultiSig(size, bits, b""))))
            if has_ind:
                step.append((r, IncomingSig(origin, lv, MultiSig(size, 1 << (origin - lo), b""), ind=True,
                                            mapped_index=origin - lo)))
        out.append(step)
    return out


@pytest.mark.parametrize("k", [1, 3, 64])
def test_pool_model_equals_read_todos(k):
    """Four steps, three receivers at N = 64: after every step the model's
    picks and every receiver's remaining queue equal read_todos' best and
    todos, in order. The picks are stored between steps, so queued slots turn
    to mark 0 and are dropped. At k = 1 and k = 3 at least 8 (store, step)
    queues come back in another order than they arrived in."""
    from handel_amd.intake import PoolModel
    from handel_amd.sigprocessing import (BatchedEvaluatorProcessing, EvaluatorStore, IndividualSigFilter, Store)

    nreg = 64
    rnd = random.Random(2024)
    receivers = rnd.sample(range(nreg), 3)
    host = {r: Store(r, nreg, lambda a, b: a) for r in receivers}
    procs = {r: BatchedEvaluatorProcessing(lambda sps: [None] * len(sps), EvaluatorStore(host[r]), batch=k)
             for r in receivers}
    model = PoolModel(receivers)
    filters = {r: IndividualSigFilter() for r in receivers}
    picked_total = 0
    for step in _steps(nreg, receivers, rnd):
        for r, sp in step:
            procs[r].add(sp)
            if filters[r].accept(sp):
                assert model.append(r, sp)
        want = []
        for r in receivers:
            if procs[r].todos:
                done, best = procs[r].read_todos()
                assert not done
                want += [(r, sp) for sp in best]
        got = model.step(k, lambda r, sp: host[r].evaluate(sp))
        assert [(r, sp) for r, sp, _ in got] == want  # the same objects in the same order
        for r in receivers:
            assert [it for it, _ in model.queue(r)] == procs[r].todos, r
            assert all(mk > 0 for _, mk in model.queue(r))
        assert model.count() == sum(len(procs[r].todos) for r in receivers)
        for r, sp, mark in got:
            assert mark > 0
            host[r].store(sp)
        picked_total += len(got)
    assert picked_total > 0 and model.dropped >= 8
    if k < 64:
        assert model.disordered >= 8, model.disordered
        assert model.count() > 0


def test_pool_symbols_declared_exported_and_bound():
    from handel_amd import _lib
    from handel_amd import build as B

    header = open(os.path.join(ROOT, "include", "handel_gpu.h")).read()
    for name in POOL_SYMBOLS:
        assert re.search(r"\b%s\(" % name, header), f"{name} not declared in include/handel_gpu.h"
        assert name in _lib.SIGNATURES, f"{name} not bound in handel_amd/_lib.py"
    assert "typedef struct hg_pool hg_pool;" in header
    if not os.path.exists(B.LIB):
        pytest.skip("library not built")
    lib = ctypes.CDLL(B.LIB)
    for name in POOL_SYMBOLS:
        assert hasattr(lib, name), name


def test_pool_null_handles_are_refused():
    from handel_amd import _lib
    from handel_amd import build as B

    if not os.path.exists(B.LIB):
        pytest.skip("library not built")
    L = _lib.load(build_if_missing=False)
    out = ctypes.c_void_p(1)
    assert L.hg_stores_pool_create(None, 16, ctypes.byref(out)) == _lib.HG_ERR_ARG and not out.value
    L.hg_stores_pool_destroy(None)
    assert L.hg_stores_pool_bytes(None) == 0
    assert L.hg_stores_pool_select_capacity(None, 4) == 0
    assert L.hg_stores_pool_append_device(None, None, 0, 1, None, None, None, None, None, None) == _lib.HG_ERR_ARG
    assert L.hg_stores_pool_step_device(None, 1, 0, None, None, None, None, None, None, None, None) == _lib.HG_ERR_ARG
    n = ctypes.c_size_t(7)
    assert L.hg_stores_pool_count(None, ctypes.byref(n)) == _lib.HG_ERR_ARG
    assert L.hg_stores_pool_read(None, 0, 0, None, None, None, ctypes.byref(n)) == _lib.HG_ERR_ARG
    assert L.hg_stores_pool_clear(None) == _lib.HG_ERR_ARG
