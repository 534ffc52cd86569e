"""GPU suite: every per-thread primitive of bn256_fp.h and bn256_curve.h, run
alone on raw limbs (hg_debug_field, bn256_fprobe.hip), equals plain Python
integers on the edge corpus of tests/test_field_edges.py: word for word where
the function promises a reduced result, as a point (canonical limbs, Z == 0
exactly for infinity, else the oracle's affine point) for the group law.

One launch per op, at most 512 threads. That the corpus reaches every class of
the guarded final subtraction in every reduction, and every named exceptional
pair of the group law, is checked on the CPU (test_field_edges.py
test_rare_subtractions_are_taken, test_curve_classes_are_present_and_of_their_kind)
and asserted again here for the op under test."""

import ctypes

import numpy as np
import pytest

from tests import test_field_edges as E

pytestmark = pytest.mark.gpu

HG_ERR_ARG = 100


@pytest.mark.parametrize("op", list(E.OPS))
def test_probe_equals_integers(engine, op):
    num, wi, wo = E.OPS[op]
    cs = E.cases(op)
    assert 1 <= len(cs) <= E.MAX_CASES
    if op in E.MUL_OPS:  # the inputs reach the guarded subtraction's three classes (see the module docstring)
        tot = E.reduction_counts()
        for name in {n for c in cs for n, _ in E.reductions(op, c.args)}:
            assert all(tot[name][cl] >= 1 for cl in E.CLASSES), (name, tot[name])
    if op in E.PAIR_OPS:
        assert all(E.curve_classes(op).values()), op
    assert engine.field_words(num) == (wi, wo)
    got = engine.field_op(num, E.inputs(op))
    assert got.shape == (len(cs), wo)
    bad = [(c, m) for c, m in ((c, E.mismatch(op, c, row)) for c, row in zip(cs, got)) if m is not None]
    if bad:
        c, m = bad[0]
        pytest.fail(f"op {op} ({num}), case {cs.index(c)} ({c.label!r}), {m}; "
                    f"{len(bad)} of {len(cs)} cases differ, first {[b.label for b, _ in bad[:8]]}")


def test_refusals_leave_out_untouched(engine):
    wi, wo = E.OPS["fp_add"][1:]
    src = np.full((2, wi), 7, dtype=np.uint32)
    out = np.full((2, wo), 0xA5A5A5A5, dtype=np.uint32)
    fp_add = E.OPS["fp_add"][0]
    calls = [(-1, src.ctypes.data, 2, out.ctypes.data), (len(E.OPS), src.ctypes.data, 2, out.ctypes.data),
             (1 << 20, src.ctypes.data, 2, out.ctypes.data), (fp_add, None, 2, out.ctypes.data),
             (fp_add, src.ctypes.data, 2, None), (fp_add, src.ctypes.data, (1 << 20) + 1, out.ctypes.data)]
    for op, a, n, o in calls:
        a_w, o_w = ctypes.c_int(-77), ctypes.c_int(-78)
        rc = engine.L.hg_debug_field(engine.ctx, op, a, n, o, ctypes.byref(a_w), ctypes.byref(o_w))
        assert rc == HG_ERR_ARG, (op, n, rc)
        assert (out == 0xA5A5A5A5).all() and (a_w.value, o_w.value) == (-77, -78), (op, n)
    # n = 0 only reports the word counts, for every op
    for name, (num, wi, wo) in E.OPS.items():
        a_w, o_w = ctypes.c_int(0), ctypes.c_int(0)
        assert engine.L.hg_debug_field(engine.ctx, num, None, 0, None, ctypes.byref(a_w), ctypes.byref(o_w)) == 0
        assert (a_w.value, o_w.value) == (wi, wo), name
    assert engine.L.hg_debug_field(engine.ctx, fp_add, None, 0, None, None, None) == 0
    assert (out == 0xA5A5A5A5).all()
