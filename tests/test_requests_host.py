"""CPU test of the request rules every aggregate entry point and kernel shares
(handel_amd/csrc/hg_requests.h: level_ok, words_ok and the host's walk over a
batch): tests/native/requests_host.cpp, a stand-alone program over that header
alone, built by the host compiler with the address and undefined-behaviour
sanitizers and run as its own process. No GPU needed."""

import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_request_rules_in_the_host_compiled_unit(tmp_path):
    exe = str(tmp_path / "requests_host")
    subprocess.check_call(["g++", "-O1", "-g", "-std=c++17", "-Wall", "-Wextra", "-Werror",
                           "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                           "-I", os.path.join(ROOT, "handel_amd", "csrc"),
                           os.path.join(ROOT, "tests", "native", "requests_host.cpp"), "-o", exe])
    r = subprocess.run([exe], capture_output=True, text=True, timeout=120,
                       env=dict(os.environ, ASAN_OPTIONS="detect_leaks=1"))
    assert r.returncode == 0, (r.stdout[-2000:], r.stderr[-2000:])
    assert r.stderr == "", r.stderr[-2000:]  # no sanitizer report
    assert r.stdout == "ok\n"


def test_the_header_includes_nothing_from_hip():
    src = open(os.path.join(ROOT, "handel_amd", "csrc", "hg_requests.h")).read()
    incs = [line.split()[1] for line in src.splitlines() if line.startswith("#include")]
    assert incs == ["<stddef.h>", "<stdint.h>", '"../../include/handel_gpu.h"'], incs
