"""The pairing-form chooser (handel_amd/csrc/bn256_sigform.h) on the CPU:
tests/native/sigform_host.cpp includes that header alone, compiles with
-fsanitize=address,undefined and runs as its own process.

It walks HG_SIG12 x HG_SIG_W2 x pad x w2_max x n (240 cells, n on both sides
of 2048 and of 2^28) and compares sig_form() with the rules written out as
boolean expressions; asserts the documented rows (a context's 1024-check batch
takes the two-wave form, its 4096-check batch the padded 16-lane kernel, an
unpadded lane the 12-lane form up to 2^28 checks and the 16-lane one above);
that only the unpadded 12-lane form splits, unless HG_SIG12_SPLIT=0; that only
the 12-lane forms ask for a workspace; and config 2's bound.
"""

import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_sig_form_rules_under_sanitizers(tmp_path):
    exe = str(tmp_path / "sigform_host")
    subprocess.check_call(["g++", "-O1", "-g", "-std=c++17", "-Wall", "-Wextra", "-Werror",
                           "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                           "-I", os.path.join(ROOT, "handel_amd", "csrc"),
                           os.path.join(ROOT, "tests", "native", "sigform_host.cpp"), "-o", exe])
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1")
    r = subprocess.run([exe], capture_output=True, text=True, timeout=120, env=env)
    assert r.returncode == 0, r.stderr[-2000:]
    assert r.stderr == "", r.stderr[-2000:]  # no sanitizer report
    assert r.stdout == "ok\n"
