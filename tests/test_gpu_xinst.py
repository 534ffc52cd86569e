"""GPU suite: every bound team-program instance of bn256_xtab.h, run alone on
raw team regions (hg_debug_xinst, bn256_xprobe.hip), equals the generator's
limb-level model (run_bound_limbs) word for word over the WHOLE region:
results, pre-pass scratch and the elements no round writes.

Per instance the thirteen regions of tests/test_xinst_edges.py go out in one
launch (12-lane waves of 5, 5 and 3 teams, 16-lane waves of 4, 4, 4 and 1: a
full and a ragged wave); the layout-S instances run in both forms (one-wave
teams and the 2-wave split teams). 145 + 28 instance-forms, 13 cases each.
That the inputs take every form of the guarded final subtraction in every
layout is checked on the CPU (test_xinst_edges.py
test_rare_subtractions_are_taken) and asserted again here."""

import ctypes

import numpy as np
import pytest

from tests import test_xinst_edges as E

pytestmark = pytest.mark.gpu

HG_ERR_ARG = 100
PARAMS = [(lay, part, 0) for lay, part in E.PARTS] + [("S", 0, 1)]


def _regions(runs, attr):
    return np.array([getattr(r, attr) for r in runs], dtype=np.uint32)


def _first_mismatch(got, want):
    case, elem, limb = (int(v[0]) for v in np.nonzero(got != want))
    return case, elem, limb


@pytest.mark.parametrize("layout,part,form", PARAMS, ids=[f"{lay}{k}-form{f}" for lay, k, f in PARAMS])
def test_probe_equals_limb_model(engine, layout, part, form):
    tot = E.taken_counts(layout)
    for f in E.FORMS:  # the inputs reach the guarded subtractions (see the module docstring)
        assert (tot[f][1] >= 1) == (layout in E.FORM_LAYOUTS[f]), (layout, f, tot[f])
    for i in E.part_instances(layout, part):
        mine = E.instance_runs(i)
        assert len(mine) == E.NCASES
        assert engine.xinst_region_elems(i, form) == E.region_elems()[layout]
        got = engine.xinst(i, _regions(mine, "mem_in"), form=form)
        want = _regions(mine, "mem_out")
        if not np.array_equal(got, want):
            c, e, l = _first_mismatch(got, want)
            bad = sorted({(int(a), int(b)) for a, b in zip(*np.nonzero((got != want).any(axis=2)))})
            pytest.fail(f"instance {E.label(i)} form {form}, case {c} ({mine[c].case!r}), element {e}, limb {l}: "
                        f"GPU 0x{int(got[c, e, l]):08x}, model 0x{int(want[c, e, l]):08x}; "
                        f"{len(bad)} (case, element) pairs differ, first {bad[:8]}")


def test_refusals_leave_out_untouched(engine):
    n_inst = len(E.G.ALL_INSTANCES)
    t_inst = E.instances("T")[0]
    s_inst = E.instances("S")[0]
    for inst, form in ((-1, 0), (n_inst, 0), (t_inst, 1), (s_inst, 2), (E.instances("D")[0], 1), (s_inst, -1)):
        elems = E.region_elems()[E.layout_of(min(max(inst, 0), n_inst - 1))]
        src = np.full((2, elems, 10), 7, dtype=np.uint32)
        out = np.full((2, elems, 10), 0xA5A5A5A5, dtype=np.uint32)
        re = ctypes.c_int(-77)
        rc = engine.L.hg_debug_xinst(engine.ctx, inst, form, src.ctypes.data, 2, out.ctypes.data, ctypes.byref(re))
        assert rc == HG_ERR_ARG, (inst, form, rc)
        assert (out == 0xA5A5A5A5).all() and re.value == -77, (inst, form)
    # n = 0 only reports the region
    re = ctypes.c_int(0)
    assert engine.L.hg_debug_xinst(engine.ctx, s_inst, 1, None, 0, None, ctypes.byref(re)) == 0
    assert re.value == E.region_elems()["S"]
