"""CPU suite: the generated team programs (tools/gen_g2_schedule.py, the
tables compiled into the HIP library) compute the points and lines of
x/crypto's lineFunctionDouble / lineFunctionAdd and the Fp12
products/squarings; and the committed headers are the ones the generator
emits."""

import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tools"))

import gen_g2_schedule as G  # noqa: E402

CSRC = os.path.join(ROOT, "handel_amd", "csrc")


def test_schedule_interpreter_matches_oracle():
    assert G.validate(seed=11)


def test_two_phase_programs_match_oracle():
    # validate_x checks every compiled round against the oracle's line
    # functions and Fp12 ops, including the column / REDC-input bounds
    X = G.validate_x(seed=5)
    G.check_instances(X, seed=7)


def test_committed_headers_are_current(tmp_path):
    out = tmp_path / "regs.h"
    G.emit_regs(str(out))
    with open(os.path.join(CSRC, "bn256_regs.h")) as f:
        assert f.read() == out.read_text()
    outx = tmp_path / "xtab.h"
    X = G.compile_all()
    G.emit_x(X, str(outx))
    with open(os.path.join(CSRC, "bn256_xtab.h")) as f:
        assert f.read() == outx.read_text()
    outp = tmp_path / "xprobe.h"
    G.emit_xprobe(X, str(outp))
    with open(os.path.join(CSRC, "bn256_xprobe.h")) as f:
        assert f.read() == outp.read_text()
