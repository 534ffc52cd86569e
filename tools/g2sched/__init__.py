"""The team-program generator's body (tools/gen_g2_schedule.py is its entry
point and the module that tests import). Each module imports only from the
ones before it:

    field     the field's constants, the register file, the expression helpers
    programs  the source programs and THE PROGRAM TABLE (one Program per team program)
    limbs     the limb-level model of the executor's arithmetic
    xround    XRound, compile_round and its bound checks, compile_all, validate_x
    layouts   THE LAYOUT TABLE (one Layout per team region) with the instances
              bound on each, bind, the region check
    emit      the emitters of the three headers, the probe's kernel grouping
"""
