"""CPU suite of the device stores' host side (handel_amd/intake.py,
hg_stores_*): the new entry points refuse NULL handles without a device, and
the selection rule the GPU tests compare against (intake.select_reference /
select_slots) is BatchedEvaluatorProcessing.read_todos on random marks with
ties, queue order included."""

import random

import pytest

from handel_amd import _lib
from handel_amd import intake as I
from handel_amd import sigprocessing as SP


def test_null_stores_are_refused_without_gpu():
    L = _lib.load(build_if_missing=False)
    A = _lib.HG_ERR_ARG
    assert L.hg_stores_create(None, None, 0, 0, None) == A
    L.hg_stores_destroy(None)
    assert L.hg_stores_update(None, None, 0, None, 0) == A
    assert L.hg_stores_read(None, 0, 1, None, None, None) == A
    assert L.hg_stores_evaluate_device(None, None, 0, 0, None, None, None, None, None) == A
    assert L.hg_stores_evaluate(None, None, 0, 0, None, None, None, None) == A
    assert L.hg_stores_select_capacity(None, 16, 4) == 0
    assert L.hg_stores_select_device(None, None, 0, None, 1, None, None, None, None, None, None, None) == A


class _Marks:
    """SigEvaluator that hands out prepared marks (keyed by object identity)."""

    def __init__(self, marks):
        self.marks = marks

    def evaluate(self, sp):
        return self.marks[id(sp)]


def _read_todos(marks, k):
    """read_todos over one queue whose i-th entry has marks[i]: (picked
    indices in pick order, re-queued indices in queue order)."""
    sps = [SP.IncomingSig(origin=i, level=1, ms=SP.MultiSig(1, 1, b"")) for i in range(len(marks))]
    proc = SP.BatchedEvaluatorProcessing(lambda sigs: [None] * len(sigs), _Marks({id(s): m for s, m in zip(sps, marks)}),
                                         batch=k)
    for s in sps:
        proc.add(s)
    done, best = proc.read_todos()
    assert not done
    return [s.origin for s in best], [s.origin for s in proc.todos]


@pytest.mark.parametrize("k", [1, 3, 64])
def test_select_reference_equals_read_todos(k):
    rnd = random.Random(100 + k)
    for trial in range(40):
        n = rnd.randrange(1, 200)
        marks = [rnd.choice([0, 0, 1, 1, 5, 5, 5, 99760, 99760, 999980, rnd.randrange(1, 12)]) for _ in range(n)]
        assert I.select_reference(marks, k) == _read_todos(marks, k), (trial, k)


@pytest.mark.parametrize("k", [1, 3, 64])
def test_select_slots_is_read_todos_per_store(k):
    """The grouped form: every store's slots in queue order through read_todos,
    the stores in order; slots without a store are never picked."""
    rnd = random.Random(7 + k)
    n, n_stores = 150, 5
    store_of_pkt = [rnd.randrange(-1, n_stores) for _ in range(n)]
    store_of_slot = store_of_pkt + store_of_pkt
    scores = [rnd.choice([-1, 0, 0, 1, 1, 7, 7, 7, 99760, rnd.randrange(1, 9)]) for _ in range(2 * n)]
    picked, rest = I.select_slots(store_of_slot, scores, n, k, n_stores)
    want_p, want_r = [], []
    for st in range(n_stores):
        slots = sorted((s for s in range(2 * n) if store_of_slot[s] == st), key=lambda s: I.queue_position(s, n))
        p, r = _read_todos([scores[s] for s in slots], k)
        want_p += [slots[i] for i in p]
        want_r += [slots[i] for i in r]
    assert (picked, rest) == (want_p, want_r)
    assert all(scores[s] > 0 for s in picked + rest)


def test_queue_position_puts_multisignature_first():
    n = 7
    for i in range(n):
        assert I.queue_position(i, n) + 1 == I.queue_position(n + i, n)  # packet i: multisig, then individual
        if i:
            assert I.queue_position(n + i - 1, n) < I.queue_position(i, n)  # after the packet before it
    assert sorted(I.queue_position(s, n) for s in range(2 * n)) == list(range(2 * n))
    # equal marks: the pick is the multisignature
    assert I.select_slots([0] * (2 * n), [3] * (2 * n), n, 1, 1)[0] == [0]
    assert I.select_slots([0] * (2 * n), [0] * n + [3] * n, n, 2, 1)[0] == [n, n + 1]
