#!/usr/bin/env python3
"""Generates handel_amd/csrc/bn256_xtab.h, bn256_xprobe.h and bn256_regs.h:
lane-parallel "team programs" for a 16-lane team (bn256_xprog.h executes them),
the instance probe's dispatch and the numbers of the team's register file.
This file is the entry point and the module that tests import; the body is the
package g2sched beside it.

A source program (g2sched/programs.py) is a short list of rounds. In a round
every lane of the team computes one Fp element
    dst = sum_{slot} (sum_m ca_m * X[ra_m]) * (sum_m cb_m * X[rb_m])
with small signed integer coefficients and ONE lazy Montgomery reduction,
then stores it; all lanes run the same instruction stream (only addresses
and coefficients differ), rounds are separated by a team barrier (every
lane reads before any lane writes, so in-place programs are fine).
compile_round (xround.py) turns a round into the two-phase form the kernels
run (a pre-pass of shared linear combinations, then products and linear terms),
and bind (layouts.py) gives every call site its own table with absolute team
element indices.

Two tables say everything about a program and about a team region:
PROGRAM_TABLE (programs.py), one Program record per member of enum XProg, and
LAYOUTS (layouts.py), one Layout record per region with the instances bound on
it. Adding a program is one Program record and one instance line; adding a
layout is one Layout record with its instance list. Then run this file.

Operand index space of a source program (uint8):
    0..127    the team's LDS register file F (Fp elements)
    128..139  element e of the program's Fp12 source slot A (2k + c)
    160..171  element e of the program's Fp12 source slot B
Destination: an F register (< 128), element e of the destination Fp12
slot (128 + e), or 255 (lane idle).

The source programs are validated here by interpreting them with plain
modular arithmetic against the oracle, the compiled and the bound ones down
to the limb-level model of the reduction (limbs.py; tests/test_g2_schedule.py
repeats this in the CPU suite). Build tooling only: nothing in the product
imports it.
"""

import os
import sys
import types

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from g2sched import emit, field, layouts, limbs, programs, xround  # noqa: E402
from g2sched.emit import PROBE_GROUP_MAX, X_FETCH_WORDS, emit_regs, emit_x, emit_xprobe, probe_groups  # noqa: E402,F401
from g2sched.field import (LAZY_LIMB, NEG_MULT, NONE, NREGS, ONE_CHAIN_COMPARE_Q, ONE_CHAIN_QMAX_LIMIT,  # noqa: E402,F401
                           P, P2N, P_LIMBS, R_BITS, REDQ_Z, REG, SLOT_A, SLOT_B, Lane, comp)
from g2sched.layouts import (ALL_INSTANCES, BOUND_INSTANCES, F_BASE_CTX, LAYOUTS, PAIR_INSTANCES,  # noqa: E402,F401
                             PROBE_EXTRA_BASE, PROBE_INSTANCES, PROBE_LAYOUTS, REGION_END, SIG_T_F_BASE, SLOTS,
                             Layout, bind, check_instances, instance_rounds, probe_layout, probe_reg_base,
                             probe_region_elems, region, region_ends, run_bound, touched)
from g2sched.limbs import (MASK26, R_MONT, _csub_model, from_limbs, redq_tail_model, reduce_wide_model,  # noqa: E402,F401
                           run_bound_limbs, to_limbs, xround_limbs)
from g2sched.programs import (KARATSUBA_MIN, KARATSUBA_MIN_PROG, LAZY_PROGRAMS, LINE2_REGS,  # noqa: E402,F401
                              ONE_CHAIN_PROGRAMS, PRE_LANES, PROGRAM, PROGRAM_TABLE, PROGRAMS, REDC_FUSE, SCRATCH_CAP,
                              X_PROGRAMS, Program, run_program, validate)
from g2sched.xround import (X_SCR, X_SLOT_B, XRound, check_one_chain, check_xround, compile_all,  # noqa: E402,F401
                            compile_round, run_xprogram, run_xround, validate_x)


class _Facade(types.ModuleType):
    """Assigning a name here rebinds it in the package's modules as well, as it
    did when this file held the body: a test that wraps xround_limbs sees
    run_bound_limbs call its wrapper."""
    def __setattr__(self, name, value):
        for m in (field, programs, limbs, xround, layouts, emit):
            if hasattr(m, name):
                setattr(m, name, value)
        super().__setattr__(name, value)


sys.modules[__name__].__class__ = _Facade


if __name__ == "__main__":
    validate()
    csrc = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "handel_amd", "csrc")
    emit_regs(os.path.join(csrc, "bn256_regs.h"))
    Xp = validate_x()
    check_instances(Xp)
    nwords = emit_x(Xp, os.path.join(csrc, "bn256_xtab.h"))
    ngroups = emit_xprobe(Xp, os.path.join(csrc, "bn256_xprobe.h"))
    print(len(BOUND_INSTANCES), "instances,", nwords * 4, "table bytes,", ngroups, "probe kernels")
    for name, rounds in Xp.items():
        print(name, [(r.nv, r.nt, r.np, r.nl, r.words()) for r in rounds])
    print("validated and wrote bn256_regs.h, bn256_xtab.h, bn256_xprobe.h")
