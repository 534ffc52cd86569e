"""The owners of the host code's HIP handles (handel_amd/csrc/hg_dev.h: DevBuf,
Stream, Event, HostBuf) on the CPU: tests/native/dev_owners_host.cpp compiles
the header against a stand-in runtime (tests/native/fakehip) with
-fsanitize=address,undefined and runs as its own process.

It checks that ensure() below the capacity keeps the pointer, that growth
frees the old block exactly once, that a failed ensure() leaves an empty
buffer a later one can fill, the 64-element floor, bytes(), that moves and
std::swap exchange handles without a free, and that a struct of owners
deleted after an allocation failed half-way (hg_lane_create's failure path)
leaves nothing live. LeakSanitizer runs at exit.
"""

import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_owners_under_sanitizers(tmp_path):
    exe = str(tmp_path / "dev_owners_host")
    subprocess.check_call(["g++", "-O1", "-g", "-std=c++17", "-Wall", "-Wextra", "-Werror",
                           "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                           "-I", os.path.join(ROOT, "tests", "native", "fakehip"),
                           "-I", os.path.join(ROOT, "handel_amd", "csrc"),
                           os.path.join(ROOT, "tests", "native", "dev_owners_host.cpp"), "-o", exe])
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1")
    r = subprocess.run([exe], capture_output=True, text=True, timeout=120, env=env)
    assert r.returncode == 0, r.stderr[-2000:]
    assert r.stderr == "", r.stderr[-2000:]  # no sanitizer report
    assert r.stdout == "ok\n"
